"""Float64 oracle of the clip + Adam / SGD update of include/pk2hip.h (pk2_grad_norm, pk2_adam_step, pk2_sgd_step;
csrc/optim.hip), numpy only -- TEST INFRASTRUCTURE ONLY.

Written from torch's definitions, in the order the reference calls them (nn.utils.clip_grad_norm_, then optimizer.step()):

    g      = grad_scale * grad                                   (the averaged gradient of several ranks)
    norm   = ||g||_2 ,  g *= min(1, max_norm / (norm + 1e-6))    clip_grad_norm_ (max_norm <= 0: not measured, no clip)
    g     += weight_decay * p                                    after clipping: the optimiser's own L2 term
  Adam:
    m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g^2 ;  vmax = max(vmax, v)   (amsgrad only)
    p -= lr / (1 - b1^t) * m / (sqrt(vmax or v) / sqrt(1 - b2^t) + eps)
  SGD:
    buf = g on the first step, momentum * buf + g afterwards (momentum != 0) ;  p -= lr * (buf or g)

`dtype=np.float32` runs the same statements with every operation rounded to float32 (the norm is summed in float64 and
rounded once, as the library does): the CPU model that calibrates the bounds of tests/edge_cases.py, applied by
tests/test_gpu_ce_optim_frontend.py.
"""
import numpy as np


def grad_norm(g):
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    return float(np.sqrt(np.dot(g, g)))


def _prepared_grad(p, g, weight_decay, max_norm, grad_scale, dtype):
    """(g ready for the update, the norm clip_grad_norm_ returns or None)"""
    f = dtype
    g = np.asarray(g, dtype=f) * f(grad_scale)
    norm = None
    if max_norm is not None and max_norm > 0:
        norm = f(grad_norm(g))
        g = g * min(f(1), f(max_norm) / (norm + f(1e-6)))
    if weight_decay != 0:
        g = g + f(weight_decay) * p
    return g, norm


def adam_init(p, amsgrad, dtype=np.float64):
    z = np.zeros(np.shape(p), dtype=dtype)
    return dict(p=np.array(p, dtype=dtype), exp_avg=z.copy(), exp_avg_sq=z.copy(),
                max_exp_avg_sq=z.copy() if amsgrad else None, step=0)


def adam_step(state, g, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.0, grad_scale=1.0,
              dtype=np.float64):
    """One clip + Adam step on `state` (adam_init) in place; returns the norm of the scaled gradient (None: not measured)."""
    f = dtype
    b1, b2 = f(betas[0]), f(betas[1])
    g, norm = _prepared_grad(state["p"], g, weight_decay, max_norm, grad_scale, f)
    state["step"] += 1
    t = state["step"]
    # (1 - beta is formed in double from the beta handed in and rounded once, as torch does.  A caller that compares with a
    # float32 ABI hands in the float32 value of beta: float32(0.999) is 0.99900001287, and 1 minus it is 1.3e-5 below 0.001)
    state["exp_avg"] = b1 * state["exp_avg"] + f(1.0 - float(betas[0])) * g
    state["exp_avg_sq"] = b2 * state["exp_avg_sq"] + f(1.0 - float(betas[1])) * g * g
    v = state["exp_avg_sq"]
    if state["max_exp_avg_sq"] is not None:
        state["max_exp_avg_sq"] = v = np.maximum(state["max_exp_avg_sq"], v)
    bc1 = f(1.0 - float(betas[0]) ** t)
    bc2_sqrt = f(np.sqrt(1.0 - float(betas[1]) ** t))
    denom = np.sqrt(v) / bc2_sqrt + f(eps)
    state["p"] = state["p"] - (f(lr) / bc1) * (state["exp_avg"] / denom)
    return norm


def sgd_init(p, dtype=np.float64):
    return dict(p=np.array(p, dtype=dtype), buf=None, step=0)


def sgd_step(state, g, lr, momentum=0.0, weight_decay=0.0, max_norm=0.0, grad_scale=1.0, dtype=np.float64):
    """One clip + SGD step on `state` (sgd_init) in place; returns the norm of the scaled gradient (None: not measured)."""
    f = dtype
    d, norm = _prepared_grad(state["p"], g, weight_decay, max_norm, grad_scale, f)
    state["step"] += 1
    if momentum != 0:
        state["buf"] = d.copy() if state["buf"] is None else f(momentum) * state["buf"] + d
        d = state["buf"]
    state["p"] = state["p"] - f(lr) * d
    return norm
