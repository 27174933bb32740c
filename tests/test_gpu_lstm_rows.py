"""LSTMAM with sequence lengths: the output layer's three products over the valid rows only (lstm._LstmAmFunction,
pk2_gemm_f32_rows / pk2_gemm_f32_tn_colsum_rows) against the same model run without lengths.

LSTMAM(80, 136, 512, 2, 0, True), T, B = 9, 3, lengths (9, 4, 2), a logits gradient that is zero in the padding.  What is held
to what:
  * valid logits and every parameter gradient: the run with lengths and the run without are each held to torch's float64
    CPU nn.LSTM + nn.Linear on the same data within FACTOR * max(e32, floor) (tests/bound_check.py; e32 from torch's float32
    CPU modules: the bound tests/test_gpu_lstm_layer.py holds a layer to against its float64 oracle), and to each other
    within the sum of the two bounds, as tests/test_gpu_lstm_xproj.py::test_model_with_and_without holds two paths;
  * output_layer.weight / .bias gradients besides: the float64 product of the valid rows of (dlogits, y), y being the
    output layer's own input of that run, within FACTOR * max(e32, floor) with e32 from the same product in float32;
  * padded logits are exactly 0 with lengths; the explicit argument and the tensor attribute give the same bits;
    PK2_OUT_ROWS=0 gives the untagged run's bits.
"""
import numpy as np
import pytest
import torch

import bound_check
from pykaldi2_amd import lstm

pytestmark = pytest.mark.gpu

T, B, LENGTHS, P = 9, 3, (9, 4, 2), 136


def run(model, x, gout, lengths=None, attr=None):
    x = x.clone()
    if attr is not None:
        x.pk2_lengths = attr
    logits = model.forward_time_major(x, lengths) if lengths is not None else model.forward_time_major(x)
    y_last = logits.grad_fn.saved[-1][1].detach().clone()         # [T, B, 2H]: the output layer's input
    (logits * gout).sum().backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters()}
    return logits.detach().cpu().numpy(), grads, y_last.cpu().numpy()


@pytest.fixture(scope="module")
def runs():
    torch.manual_seed(0)
    model = lstm.LSTMAM(80, P, 512, 2, 0, True).cuda()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, B, 80, generator=g).cuda()
    valid = (torch.arange(T)[:, None] < torch.tensor(LENGTHS)[None, :])              # [T, B]
    gout = (torch.randn(T, B, P, generator=g) * valid[:, :, None]).cuda()
    out = dict(valid=valid.numpy(), gout=gout.cpu().numpy())
    refs = []
    for dt in (torch.float64, torch.float32):
        ref_lstm = torch.nn.LSTM(80, 512, 2, bidirectional=True).to(dt)              # time-major input
        ref_out = torch.nn.Linear(1024, P).to(dt)
        sd = {n: v.detach().cpu() for n, v in model.state_dict().items()}
        ref_lstm.load_state_dict({n[5:]: v.to(dt) for n, v in sd.items() if n.startswith("lstm.")})
        ref_out.load_state_dict({n[13:]: v.to(dt) for n, v in sd.items() if n.startswith("output_layer.")})
        logits = ref_out(ref_lstm(x.cpu().to(dt))[0])
        (logits * gout.cpu().to(dt)).sum().backward()
        refs.append(dict([("lstm." + n, v.grad.numpy()) for n, v in ref_lstm.named_parameters()] +
                         [("output_layer." + n, v.grad.numpy()) for n, v in ref_out.named_parameters()] +
                         [("logits", logits.detach().numpy()[valid.numpy()])]))
    out["refs"] = refs
    run(model, x, gout)          # (discarded: the first call of a process may take another recurrence path than the later ones)
    out["plain"] = run(model, x, gout)
    out["arg"] = run(model, x, gout, lengths=LENGTHS)
    out["attr"] = run(model, x, gout, attr=LENGTHS)
    out["arg_over_attr"] = run(model, x, gout, lengths=LENGTHS, attr=(9, 9, 9))
    import os
    os.environ["PK2_OUT_ROWS"] = "0"
    try:
        out["off"] = run(model, x, gout, lengths=LENGTHS)
    finally:
        del os.environ["PK2_OUT_ROWS"]
    return out


def test_valid_logits_and_gradients_match_the_untagged_run_and_the_float64_reference(runs):
    lg0, g0, _ = runs["plain"]
    lg1, g1, _ = runs["arg"]
    v = runs["valid"]
    assert np.isfinite(lg1).all()
    assert (lg1[~v].view(np.uint32) == 0).all(), "padded logits are not exactly 0"
    assert np.abs(lg0[~v]).max() > 0            # (the untagged run computes them: the test can tell the two apart)
    r64, r32 = runs["refs"]
    plain, tagged = dict(g0, logits=lg0[v]), dict(g1, logits=lg1[v])
    problems = []
    for name in r64:
        unit, _, _ = bound_check.unit(r64[name], r32[name])
        e0 = float(np.abs(plain[name].astype(np.float64) - r64[name]).max())
        e1 = float(np.abs(tagged[name].astype(np.float64) - r64[name]).max())
        diff = float(np.abs(tagged[name].astype(np.float64) - plain[name]).max())
        print("lstm_rows | %s | tagged-untagged %.3g | unit %.3g | untagged/f64 %.3f | tagged/f64 %.3f" % (name, diff, unit, e0 / unit,
                                                                                                       e1 / unit))
        if not np.isfinite(tagged[name]).all():
            problems.append("%s: not finite" % name)
        if not e1 <= bound_check.FACTOR * unit:
            problems.append("%s: with lengths %.3g from float64 > %.3g" % (name, e1, bound_check.FACTOR * unit))
        if not diff <= 2 * bound_check.FACTOR * unit:
            problems.append("%s: with and without lengths differ by %.3g > %.3g" % (name, diff, 2 * bound_check.FACTOR * unit))
    assert not problems, "\n".join(problems)


def test_output_layer_gradients_match_the_float64_product_of_the_valid_rows(runs):
    v = runs["valid"]
    dl = runs["gout"][v]                                                            # [15, P]
    for key in ("plain", "arg"):
        _, g, y = runs[key]
        yv = y[v]                                                                    # [15, 2H]
        ref64 = {"w": dl.astype(np.float64).T @ yv.astype(np.float64), "b": dl.astype(np.float64).sum(0)}
        ref32 = {"w": dl.T @ yv, "b": dl.sum(0, dtype=np.float32)}
        got = {"w": g["output_layer.weight"], "b": g["output_layer.bias"]}
        failures, ratios = bound_check.compare(got, ref64, ref32, ("w", "b"))
        print(key, "ratios", ratios)
        assert not failures, (key, failures)


def test_argument_attribute_and_switch_give_the_expected_bits(runs):
    # bits: the logits and the output layer's weight gradient (plain stores).  The bias gradients and the recurrences' weight
    # gradients are added with float atomics, i.e. in arrival order: two runs of the SAME call may differ in the last bit, so
    # those are held to the floor of tests/bound_check.py
    def same(a, b):
        tol = bound_check.FACTOR * 2.0 ** -23
        return (np.array_equal(a[0], b[0]) and np.array_equal(a[1]["output_layer.weight"], b[1]["output_layer.weight"]) and
                all(np.abs(a[1][n].astype(np.float64) - b[1][n]).max() <= tol * np.abs(a[1][n]).max() for n in a[1]))
    assert same(runs["arg"], runs["attr"]), "explicit lengths and the tensor attribute differ"
    assert same(runs["arg"], runs["arg_over_attr"]), "the explicit argument did not take precedence over the attribute"
    assert same(runs["plain"], runs["off"]), "PK2_OUT_ROWS=0 is not the untagged run"


def test_bad_lengths_are_refused():
    model = lstm.LSTMAM(80, P, 64, 1, 0, True).cuda()
    x = torch.zeros(T, B, 80, device="cuda")
    for bad in ((9, 4), (10, 4, 2), (-1, 4, 2)):
        with pytest.raises(ValueError):
            model.forward_time_major(x, bad)
