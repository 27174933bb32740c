"""transformer.BandMask through the public interface: a two-layer TransformerAM (dim_model 128; nheads 2 = head size 64,
nheads 1 = head size 128) with T = 70, B = 2, ragged lengths, no dropout.  The banded kernels against the same model given
the band as its dense [T, T] mask (the existing fused kernels), held to the bound tests/test_gpu_transformer_h128.py uses
for fused against batched GEMMs: 2e-5 on the output, 1e-4 on the parameter gradients, the Frobenius rule (5e-3 of the
gradient's norm) for a gradient moved by a flipped ReLU mask."""
import pytest
import torch

from pykaldi2_amd import transformer

pytestmark = pytest.mark.gpu

T, B, FRAMES = 70, 2, [70, 53]
BAND = transformer.BandMask(20, 2, 8)


def run(nheads, call):
    """Output and parameter gradients of call(model, x) -> [T, B, P] on a fresh model of fixed seed."""
    torch.manual_seed(3)
    m = transformer.TransformerAM(24, 128, nheads, 256, 2, 0.0, 19).cuda().train()
    x = torch.randn(T, B, 24, device="cuda")
    y = call(m, x)
    w = torch.randn(T, B, 19, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    (y * w).sum().backward()
    return y.detach().cpu(), {n: p.grad.detach().cpu() for n, p in m.named_parameters()}


def key_padding():
    kpm = torch.ones(B, T, dtype=torch.bool)
    for b, n in enumerate(FRAMES):
        kpm[b, :n] = False
    return kpm


@pytest.fixture(scope="module", params=[2, 1], ids=["head64", "head128"])
def dense(request):
    """(nheads, output, gradients) with BAND as a dense mask: computed once per head size."""
    mp = pytest.MonkeyPatch()
    mp.setenv("PK2_ATTN_FUSED", "all")
    yield (request.param,) + run(request.param, lambda m, x: m(x, BAND.dense(T), key_padding()))
    mp.undo()


def assert_close(y1, g1, y0, g0):
    assert torch.isfinite(y1).all()
    assert (y1 - y0).abs().max().item() < 2e-5 * max(1.0, y0.abs().max().item())
    for n in g0:
        e = (g1[n] - g0[n]).abs().max().item()
        if e < 1e-4 * max(1e-2, g0[n].abs().max().item()):
            continue
        f = (g1[n] - g0[n]).norm().item()
        print("relu_flip | %s | max %.3e | frobenius %.3e of %.3e" % (n, e, f, g0[n].norm().item()))
        assert f < 5e-3 * max(1e-6, g0[n].norm().item()), (n, e, f, g0[n].norm().item())


@pytest.mark.parametrize("route", ["forward", "padded_forward"])
def test_band_mask_equals_its_dense_mask(dense, route):
    nheads, y0, g0 = dense
    assert transformer.attention_is_fused(128 // nheads)
    if route == "forward":
        y1, g1 = run(nheads, lambda m, x: m(x, BAND, key_padding()))
    else:
        y1, g1 = run(nheads, lambda m, x: transformer.padded_forward(m, x, FRAMES, look_ahead=2, left_context=20,
                                                                      chunk=8).transpose(0, 1))
    assert_close(y1, g1, y0, g0)


def test_look_ahead_alone_keeps_the_dense_route():
    """padded_forward with no new argument is a direct call with the dense tril mask: the output bit for bit.  The parameter
    gradients are sums of float atomics (split products, column sums), which two runs of ONE route do not reproduce bit for
    bit either: they are held to the bound above."""
    tri = torch.tril(torch.ones(T, T), diagonal=3)
    mask = torch.zeros(T, T).masked_fill(tri == 0, float("-inf"))
    y0, g0 = run(2, lambda m, x: m(x, mask, key_padding()))
    y1, g1 = run(2, lambda m, x: transformer.padded_forward(m, x, FRAMES, look_ahead=3).transpose(0, 1))
    assert torch.equal(y0, y1)
    assert_close(y1, g1, y0, g0)
