"""TransformerAM at head size 128 (the transformer command lines' default -dim_model 512 -nheads 4 is 512 / 4): the fused
kernels of csrc/attention128.hip under the model, against the batched-GEMM form and against torch on the CPU, and the
memory the fused form exists for.  Every test sets PK2_ATTN_FUSED itself (all / 0), so none depends on which head sizes
are fused by default."""
import copy

import pytest
import torch

import test_gpu_transformer as TT
from pykaldi2_amd import transformer

pytestmark = pytest.mark.gpu


def test_attention_is_fused_follows_the_switch(monkeypatch):
    monkeypatch.setenv("PK2_ATTN_FUSED", "all")
    assert transformer.attention_is_fused(64) is True and transformer.attention_is_fused(128) is True
    assert transformer.attention_is_fused(16) is False
    monkeypatch.setenv("PK2_ATTN_FUSED", "0")
    assert transformer.attention_is_fused(64) is False and transformer.attention_is_fused(128) is False
    assert transformer.attention_is_fused(16) is False
    for mode in (None, "1"):                   # the default set: head size 64 always, never an unserved size
        if mode is None:
            monkeypatch.delenv("PK2_ATTN_FUSED")
        else:
            monkeypatch.setenv("PK2_ATTN_FUSED", mode)
        assert transformer.attention_is_fused(64) is True and transformer.attention_is_fused(16) is False
        assert transformer.attention_is_fused(128) is (128 in transformer.DEFAULT_FUSED_HEAD_SIZES)


@pytest.mark.parametrize("T,B,look,drop", [(77, 3, 5, 0.0), (77, 3, 5, 0.1), (32, 1, -1, 0.0), (130, 2, -1, 0.2),
                                           (200, 4, -1, 0.0), (200, 4, 3, 0.1)])
def test_fused_attention_equals_the_batched_gemm_form_at_head_size_128(T, B, look, drop, monkeypatch):
    """tests/test_gpu_transformer.py: test_fused_attention_equals_the_batched_gemm_form with C, H = 256, 2: same (T, B,
    look, drop) list, same ragged padding for B = 4, same seeds, same tolerances (2e-5 on the outputs, 1e-4 on the
    parameter gradients).  A parameter whose gradient exceeds 1e-4 because an activation within rounding of zero flipped its
    ReLU mask between the two forms is judged by the Frobenius rule of test_convolution_as_one_product_against_three
    (5e-3 of the gradient's norm) instead."""
    C, H = 256, 2

    def run(fused):
        monkeypatch.setenv("PK2_ATTN_FUSED", "all" if fused else "0")
        assert transformer.attention_is_fused(C // H) is fused
        torch.manual_seed(3)
        m = transformer.TransformerAM(24, C, H, 256, 2, drop, 19).cuda().train()
        x = torch.randn(T, B, 24, device="cuda")
        kpm = torch.zeros(B, T, dtype=torch.bool, device="cuda")
        for i in range(1, B):
            kpm[i, T - 3 * i:] = True
        if B == 4:       # ragged minibatch: whole key tiles of padding behind short utterances, one valid key only, a hole
            kpm[1, 33:] = True
            kpm[2, 1:] = True
            kpm[3, 40:150] = True
        src_mask = None
        if look > -1:
            tri = torch.tril(torch.ones(T, T), diagonal=look)
            src_mask = tri.float().masked_fill(tri == 0, float("-inf")).masked_fill(tri == 1, 0.0).cuda()
        torch.manual_seed(11)            # the dropout seeds are drawn from torch's generator
        y = m(x, src_mask, kpm)
        w = torch.randn(T, B, 19, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        (y * w).sum().backward()
        return y.detach().cpu(), {n: p.grad.detach().cpu() for n, p in m.named_parameters()}

    y1, g1 = run(True)
    y0, g0 = run(False)
    assert torch.isfinite(y1).all()
    assert (y1 - y0).abs().max().item() < 2e-5 * max(1.0, y0.abs().max().item())
    for n in g0:
        e = (g1[n] - g0[n]).abs().max().item()
        if e < 1e-4 * max(1e-2, g0[n].abs().max().item()):
            continue
        f = (g1[n] - g0[n]).norm().item()          # a flipped ReLU mask: a few elements move, the gradient as a whole does not
        print("relu_flip | %s | max %.3e | frobenius %.3e of %.3e" % (n, e, f, g0[n].norm().item()))
        assert f < 5e-3 * max(1e-6, g0[n].norm().item()), (n, e, f, g0[n].norm().item())


def test_transformer_h128_matches_torch_cpu(monkeypatch):
    """tests/test_gpu_transformer.py: test_transformer_matches_torch_cpu at head size 128, fused, with its tolerances."""
    monkeypatch.setenv("PK2_ATTN_FUSED", "all")
    cfg = dict(D=24, C=256, H=2, FF=128, L=2, P=37, T=70, B=3, look=2)
    assert transformer.attention_is_fused(cfg["C"] // cfg["H"])
    torch.manual_seed(0)
    m = transformer.TransformerAM(cfg["D"], cfg["C"], cfg["H"], cfg["FF"], cfg["L"], 0.0, cfg["P"])
    for lp in m.transformer.layers:          # break the deep-copy symmetry of the default init
        for p in lp.parameters():
            p.data.add_(0.02 * torch.randn_like(p))
    ref = copy.deepcopy(m).eval()
    T, B = cfg["T"], cfg["B"]
    x = torch.randn(T, B, cfg["D"])
    lens = [T] + [max(1, T - 4 - 2 * i) for i in range(B - 1)]
    kpm = torch.ones(B, T)
    for i, n in enumerate(lens):
        kpm[i, :n] = 0
    kpm = kpm.bool()
    tri = torch.tril(torch.ones(T, T), diagonal=cfg["look"])
    src_mask = tri.float().masked_fill(tri == 0, float("-inf")).masked_fill(tri == 1, 0.0)
    w = torch.randn(T, B, cfg["P"])
    for i, n in enumerate(lens):
        w[n:, i] = 0        # padded query rows carry no gradient (their loss is ignored in the reference)
    want = TT._reference_forward(ref, x, src_mask, kpm)
    (want * w).sum().backward()
    m = m.cuda().train()
    got = m(x.cuda(), src_mask.cuda(), kpm.cuda())
    valid = torch.zeros(T, B, dtype=torch.bool)
    for i, n in enumerate(lens):
        valid[:n, i] = True
    err = (got.cpu() - want.detach())[valid].abs().max().item()
    assert err < 2e-4 * max(1.0, want.detach()[valid].abs().max().item()), err
    (got * w.cuda()).sum().backward()
    refg = dict(ref.named_parameters())
    for name, p in m.named_parameters():
        g, rg = p.grad.cpu(), refg[name].grad
        e = (g - rg).abs().max().item()
        assert e < 5e-4 * max(1e-2, rg.abs().max().item()), (name, e, rg.abs().max().item())


def test_fused_attention_keeps_the_scores_out_of_memory(monkeypatch):
    """The memory the fused form exists for.  T = 512, B = 2, H = 2, 2 layers: the unfused forward keeps L B H T^2 floats =
    8 MiB of probabilities for the backward pass (and its backward allocates a further T^2 tensor, dP); the fused form
    keeps lse instead, 8 KB per layer.  Everything else the two runs allocate is the same, so the peaks differ by at
    least the scores: this follows from the allocation lists and is no measurement."""
    T, B, C, H, L = 512, 2, 256, 2, 2
    scores = L * B * H * T * T * 4
    assert scores == 8 << 20
    torch.manual_seed(1)
    m = transformer.TransformerAM(24, C, H, 128, L, 0.0, 19).cuda().train()
    x = torch.randn(T, B, 24, device="cuda")
    w = torch.randn(T, B, 19, device="cuda")
    peak = {}
    for mode in ("0", "all"):                      # unfused, then fused
        monkeypatch.setenv("PK2_ATTN_FUSED", mode)
        assert transformer.attention_is_fused(C // H) is (mode == "all")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        y = m(x)
        (y * w).sum().backward()
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated()
        del y
    print("attention128_peak_bytes | unfused %d | fused %d | scores %d" % (peak["0"], peak["all"], scores))
    assert peak["0"] - peak["all"] >= 0.9 * scores, peak
