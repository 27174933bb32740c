"""Inputs and bounds shared by tests/test_oracle_ce_optim.py (CPU) and tests/test_gpu_ce_optim_frontend.py.  Plain module,
no GPU, no pytest.  Every bound here is derived from the float64 oracles, the float32 CPU models next to them and the
precision of float32 -- never from what a kernel returned."""
import numpy as np

from oracle import optim_ref

ULP = 2.0 ** -23          # spacing of float32 at 1
SENTINEL = -12345.5       # guard bands and output gaps: any write outside the logical output changes it


# ---------------------------------------------------------------------------------------------------------------- softmax-CE
CE_REGIMES = ("spread", "peaked", "offset", "masked")
CE_GRAD_BOUND = 2e-6      # |grad - float64| <= 2e-6 * gs per element: the project's existing CE bound
CE_LOSS_REL = 1e-5        # summed loss, relative: the project's existing bound


def ce_logits(regime, rows, P, seed=0):
    """float32 [rows, P].  spread: 3 N(0,1); peaked: 30 N(0,1) (log-probs down to -200); offset: 3000 + 3 N(0,1);
    masked: spread with a third of the classes at -inf (class 0 of every row stays finite)."""
    rng = np.random.default_rng(1000 * seed + 7 * rows + P)
    z = rng.standard_normal((rows, P))
    if regime == "spread":
        x = 3.0 * z
    elif regime == "peaked":
        x = 30.0 * z
    elif regime == "offset":
        x = 3000.0 + 3.0 * z
    elif regime == "masked":
        x = 3.0 * z
        hole = rng.random((rows, P)) < 1.0 / 3.0
        hole[:, 0] = False
        x[hole] = -np.inf
    else:
        raise ValueError(regime)
    return x.astype(np.float32)


def ce_targets(x, seed=0):
    """One finite class per row, int64."""
    rng = np.random.default_rng(seed + x.shape[1])
    t = np.zeros(x.shape[0], dtype=np.int64)
    for r in range(x.shape[0]):
        t[r] = rng.choice(np.nonzero(np.isfinite(x[r]))[0])
    return t


def logprob_bound(x, lp64):
    """(bound, e_torch, floor): |log-prob - float64| <= 4 e_torch + 8 * 2^-23 * max(1, max |lp64|), e_torch = the error of
    torch's float32 CPU log_softmax on the same input -- what the reference's own float32 path delivers; the floor covers a
    device expf / logf that is a few ulp off the host's.  -inf log-probs (masked classes) are compared exactly and leave
    the maxima."""
    import torch
    fin = np.isfinite(lp64)
    t32 = torch.log_softmax(torch.from_numpy(np.ascontiguousarray(x)), dim=-1).numpy().astype(np.float64)
    assert np.array_equal(np.isneginf(t32), ~fin)
    e_torch = float(np.abs(np.where(fin, t32 - np.where(fin, lp64, 0.0), 0.0)).max())
    floor = 8.0 * ULP * max(1.0, float(np.abs(lp64[fin]).max()))
    return 4.0 * e_torch + floor, e_torch, floor


def logprob_error(got, lp64):
    """max |got - lp64| over the finite log-probs; the -inf ones must be -inf exactly, nothing may be NaN."""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(lp64)
    assert not np.isnan(got).any(), "NaN log-probs"
    assert np.array_equal(np.isneginf(got), ~fin), "-inf log-probs at other places than the oracle's"
    return float(np.abs(np.where(fin, got - np.where(fin, lp64, 0.0), 0.0)).max())


# ----------------------------------------------------------------------------------------------------------------- optimisers
OPT_STEPS = 10
# the gradient's scale by step: small after large, so that an amsgrad maximum has to survive later small gradients
OPT_SCALES = (1e-4, 1e-2, 1.0, 1e2, 1e-3, 1e-1, 10.0, 1e-4, 1e2, 1e-2)
OPT_LRS = tuple(1e-2 * min((k + 1) / 4.0, (4.0 / (k + 1)) ** 0.5) for k in range(OPT_STEPS))      # rewritten every step
OPT_MAX_NORM = {"none": 0.0, "binding": 5.0, "loose": 1e9}     # 1e9: measured, and above every norm of OPT_SCALES
NORM_REL = 1e-6
# The C ABI takes beta1 / beta2 as float32, and the update it defines is Adam with THOSE betas (the kernel forms 1 - beta and the
# bias corrections from them, consistently): the oracle gets the same two numbers.  With the double 0.999 instead, exp_avg_sq
# would differ by 1.3e-5 relative (1 - float32(0.999) against 0.001) while the parameters would not notice.
OPT_BETAS = (float(np.float32(0.9)), float(np.float32(0.999)))


def opt_problem(n, seed=0):
    """(p0 float32 [n], grads float32 [OPT_STEPS, n]); element n // 2 of every gradient is exactly zero."""
    rng = np.random.default_rng(seed + n)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = np.stack([(s * rng.standard_normal(n)).astype(np.float32) for s in OPT_SCALES])
    grads[:, n // 2] = 0.0
    return p0, grads


def run_adam(p0, grads, amsgrad, wd, grad_scale, clip, dtype, steps=OPT_STEPS):
    """The oracle's trajectory: a list over steps of dict(p, exp_avg, exp_avg_sq, max_exp_avg_sq, norm)."""
    st = optim_ref.adam_init(p0, amsgrad, dtype)
    out = []
    for k in range(steps):
        norm = optim_ref.adam_step(st, grads[k], lr=OPT_LRS[k], betas=OPT_BETAS, weight_decay=wd, max_norm=OPT_MAX_NORM[clip],
                                   grad_scale=grad_scale, dtype=dtype)
        out.append(dict(p=st["p"].copy(), exp_avg=st["exp_avg"].copy(), exp_avg_sq=st["exp_avg_sq"].copy(),
                        max_exp_avg_sq=None if st["max_exp_avg_sq"] is None else st["max_exp_avg_sq"].copy(), norm=norm))
    return out


def run_sgd(p0, grads, momentum, wd, grad_scale, clip, dtype, steps=OPT_STEPS):
    st = optim_ref.sgd_init(p0, dtype)
    out = []
    for k in range(steps):
        norm = optim_ref.sgd_step(st, grads[k], lr=OPT_LRS[k], momentum=momentum, weight_decay=wd,
                                  max_norm=OPT_MAX_NORM[clip], grad_scale=grad_scale, dtype=dtype)
        out.append(dict(p=st["p"].copy(), buf=None if st["buf"] is None else st["buf"].copy(), norm=norm))
    return out


def ulp_of(x):
    """Spacing of float32 at max |x| (at least at the smallest normal number)."""
    m = max(float(np.abs(x).max()), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(m)) - 23)


OPT_SIZES = (1, 3, 4, 5, 255, 256, 257, 1000, 2 * 4096 * 256 + 3)
# Parameters after k steps: |p - float64| <= OPT_A * k * ulp(max |p|) + OPT_B * k * lr, max |p| over the oracle's trajectory so far.
#   OPT_A = 2.2: every step rounds p once (half an ulp) and adds the rounding of the update; the float32 mode of optim_ref
#   loses at most 0.55 k ulp(max |p|) against its float64 mode over the cross product of test_oracle_ce_optim.py: times 4.
#   OPT_B = 4 * 8 * 2^-24: the update lr * q of a step is the end of about eight float32 roundings; |q| is of order one for Adam,
#   and for SGD ulp(max |p|) already follows lr * |d| because p has moved by it.
OPT_A = 2.2
OPT_B = 4 * 8 * 2.0 ** -24
# Moments (exp_avg, exp_avg_sq, max_exp_avg_sq, the momentum buffer) after k steps: OPT_MOMENT_ULPS * k * ulp(max |moment|);
# the float32 model loses at most 2.8 k ulp (exp_avg_sq with weight decay: the gradient g + wd * p carries up to an ulp of its
# own, squaring doubles it, and two more roundings follow): times 4.
OPT_MOMENT_ULPS = 11.2


def opt_size_case(n):
    """(amsgrad / momentum on?, weight_decay, grad_scale, clip) of the one variant size n runs.  The largest size runs without
    weight decay: among two million elements some have g + wd * p cancel down to Adam's eps, where m / (sqrt(v) + eps) turns an
    ulp of g into a thousandth of a step -- a property of the update, not of an implementation."""
    return (n % 2 == 1, 0.01 if n < 1000 else 0.0, 1.0, "binding")


def opt_bound(key, t64, k):
    """The bound of tensor `key` after step k (0-based) of the float64 trajectory t64 (run_adam / run_sgd)."""
    u = ulp_of(np.concatenate([np.abs(t64[j][key]).reshape(-1) for j in range(k + 1)]))
    if key == "p":
        return OPT_A * (k + 1) * u + OPT_B * (k + 1) * max(OPT_LRS[:k + 1])
    return OPT_MOMENT_ULPS * (k + 1) * u


# ------------------------------------------------------------------------------------------------------------------ front end
SIGNALS = ("noise", "quiet", "square", "tone", "zeros")
FBANK_BOUND = 2e-4        # |log-mel - logfbank64|: the project's existing fbank bound (2e-5 measured on the golden)



def fbank_tight_bound(model, want):
    """A second, tighter bound on the log-mels of one utterance, from the arithmetic: 4 times what frontend_ref.logfbank_model
    (double transform, float32 power / mel sums / logarithm) loses against logfbank64 `want` on that utterance, plus
    4 * 2^-23 * max(1, max |log-mel|) for a device logf and summation order that are a few ulp off the host's.  About 2e-5
    at log-mels of 20-30: a pre-emphasis contracted into one fused multiply-add (6.8e-5 on the tone signal, 2.2e-5 on noise)
    does not fit, which the 2e-4 above cannot see."""
    e_model = float(np.abs(model - want).max())
    return 4.0 * e_model + 4.0 * ULP * max(1.0, float(np.abs(want).max())), e_model


FBANK_SAMPLES = (2, 241, 242, 401, 402, 561, 562, 1041, 16001)       # the frame-count edges: one frame up to 401, two from 402


def signal(kind, n, seed=0):
    """float32 [n]: noise at 0.1; noise at 1e-5 (the +1 under the logarithm dominates); a full-scale +-1 square wave (period
    50 samples); a tone at the centre of FFT bin 40 plus DC 0.5; zeros."""
    rng = np.random.default_rng(seed * 100003 + n)
    t = np.arange(n)
    if kind == "noise":
        w = 0.1 * rng.standard_normal(n)
    elif kind == "quiet":
        w = 1e-5 * rng.standard_normal(n)
    elif kind == "square":
        w = np.where((t // 25) % 2 == 0, 1.0, -1.0)
    elif kind == "tone":
        w = 0.5 + 0.4 * np.sin(2 * np.pi * 40.0 * t / 512.0)
    elif kind == "zeros":
        w = np.zeros(n)
    else:
        raise ValueError(kind)
    return w.astype(np.float32)
