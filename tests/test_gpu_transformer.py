"""TransformerAM on libpk2hip.so against the reference PyTorch CPU computation: the parameter containers are
the torch modules the reference instantiates, so their own CPU forward (looped layer by layer as SURVEY.md 8c
prescribes for torch >= 2) is the reference."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gemm_ref as G
from pykaldi2_amd import transformer

pytestmark = pytest.mark.gpu


def _reference_forward(m, x, src_mask, kpm):
    h = m.input_layer(x)
    for lp in m.transformer.layers:
        h = lp.encoder_layer(h, src_mask, kpm)
        h = F.relu(lp.conv1d(h.permute(1, 2, 0))).permute(2, 0, 1)
    return m.output_layer(m.transformer.norm(h))


@pytest.mark.parametrize("cfg", [dict(D=20, C=64, H=4, FF=128, L=2, P=37, T=11, B=3, look=2),
                                 dict(D=80, C=512, H=8, FF=2048, L=2, P=301, T=48, B=2, look=-1)])
def test_transformer_matches_torch_cpu(cfg, monkeypatch):
    # Default GEMM schedule (round 6): products of the forward form x W^T are never cut into atomically added K slices, so the
    # forward pass is bitwise reproducible and no ReLU mask can flip between runs (round 5 ran this test with
    # PK2_GEMM_SPLITK=1 because sliced FFN products failed it in ~15 % of its runs).
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
    src_mask = None
    if cfg["look"] > -1:
        tri = torch.tril(torch.ones(T, T), diagonal=cfg["look"])
        src_mask = tri.float().masked_fill(tri == 0, float("-inf")).masked_fill(tri == 1, 0.0)
    w = torch.randn(T, B, cfg["P"])
    for i, n in enumerate(lens):
        w[n:, i] = 0        # padded query rows carry no gradient (their loss is ignored in the reference)
    want = _reference_forward(ref, x, src_mask, kpm)
    (want * w).sum().backward()
    m = m.cuda().train()
    got = m(x.cuda(), src_mask.cuda() if src_mask is not None else None, kpm.cuda())
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


@pytest.mark.parametrize("T,B,look,drop", [(77, 3, 5, 0.0), (77, 3, 5, 0.1), (32, 1, -1, 0.0), (130, 2, -1, 0.2),
                                           (200, 4, -1, 0.0), (200, 4, 3, 0.1)])
def test_fused_attention_equals_the_batched_gemm_form(T, B, look, drop, monkeypatch):
    """Head size 64: csrc/attention.hip (scores in registers, backward by recomputation, probabilities dropped with the
    counter-based mask indexed like the [B*H][T][T] matrix) against the unfused form with the same seeds: outputs and
    every parameter gradient; T not a multiple of the 32-wide tiles, look-ahead mask, padded keys."""
    C, H = 128, 2

    def run(fused):
        monkeypatch.setenv("PK2_ATTN_FUSED", "1" if fused else "0")
        torch.manual_seed(3)
        m = transformer.TransformerAM(24, C, H, 256, 2, drop, 19).cuda().train()
        x = torch.randn(T, B, 24, device="cuda")
        kpm = torch.zeros(B, T, dtype=torch.bool, device="cuda")
        for i in range(1, B):
            kpm[i, T - 3 * i:] = True
        if B == 4:       # ragged minibatch: whole key tiles of padding behind short utterances (the fused kernels end their loops at
            kpm[1, 33:] = True       # the last valid key's tile), one valid key only, padding with a hole in it
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
        assert e < 1e-4 * max(1e-2, g0[n].abs().max().item()), (n, e, g0[n].abs().max().item())


def test_transformer_state_dict_keys_and_init_follow_torch():
    torch.manual_seed(3)
    m = transformer.TransformerAM(80, 512, 8, 2048, 2, 0.1, 5768)
    keys = list(m.state_dict().keys())
    assert keys[0] == "pos_encoder.pe" and "transformer.layers.1.encoder_layer.self_attn.in_proj_weight" in keys
    assert "transformer.layers.0.conv1d.weight" in keys and keys[-2:] == ["transformer.norm.weight", "transformer.norm.bias"]
    n = sum(p.numel() for p in m.parameters())
    assert n == 3001480 + 3939328 * 2
    # all layers start as copies of one initialised layer (nn.TransformerEncoder deep copies)
    a, b = m.transformer.layers[0], m.transformer.layers[1]
    assert torch.equal(a.conv1d.weight, b.conv1d.weight)


@pytest.mark.parametrize("P,param_grads", [(600, True), (6048, False)], ids=["P600_all_links", "P6048_full_width"])
def test_12_layer_transformer_into_lf_mmi_matches_torch_cpu_and_the_chain_oracle(P, param_grads, monkeypatch):
    """BASELINE configs[4]: the 12-layer TransformerAM (dim 512, 8 heads, FFN 2048, conv k=3; reference
    bin/train_transformer_se.py:128,243-258 model call with a key-padding mask) feeding ChainObjtiveBatch
    (ops/ops.py:243-280).  Three links, each against its own reference: logits vs the torch CPU forward of the same
    modules; objective and d objf / d logits vs the LF-MMI oracle on those logits; parameter gradients of the
    composition vs torch CPU autograd fed with the oracle's gradient.  T = 60 subsampled frames.  P = 600 runs all three
    links; P = 6048 (the configuration's full output width) the logits and objective / derivative links."""
    from oracle import chain_ref as R
    from pykaldi2_amd import chain, ops, synth
    torch.manual_seed(0)
    T, B, L = 60, 2, 12
    m = transformer.TransformerAM(80, 512, 8, 2048, L, 0.0, P)
    for lp in m.transformer.layers:
        for p in lp.parameters():
            p.data.add_(0.02 * torch.randn_like(p))
    ref = copy.deepcopy(m).eval()
    rng = np.random.default_rng(5)
    sups = [chain.Supervision(synth.numerator_fst_from_alignment(synth.pdf_alignment(rng, n, P)), label_dim=P) for n in (180, 133)]
    lens = [s.frames_per_sequence for s in sups]
    assert lens == [60, 45]
    x = torch.randn(T, B, 80)
    kpm = torch.ones(B, T, dtype=torch.bool)
    for i, n in enumerate(lens):
        kpm[i, :n] = False
    g = synth.den_graph_arcs(2000, 60000, P, seed=3, loop_pdf_differs=True)
    den = chain.DenominatorGraph(g, P)
    dref = R.DenGraphRef(g["num_states"], g["src"], g["dst"], g["pdf"], g["prob"], 0, P)
    opts = chain.ChainTrainingOptions(leaky_hmm_coefficient=1e-4, xent_regularize=0.1)
    # device: model -> LF-MMI -> backward
    md = m.cuda().train()
    logits = md(x.cuda(), None, kpm.cuda())                             # [T, B, P]
    logits.retain_grad()
    loss = ops.ChainObjtiveBatch.apply(logits.transpose(0, 1), den, sups, opts)
    loss.backward()
    dlogits = logits.grad.detach().cpu()                                # = -d objf / d logits (ops/ops.py:276-280)
    # (1) logits vs torch CPU
    want = _reference_forward(ref, x, None, kpm)
    got = logits.detach().cpu()
    for i, n in enumerate(lens):
        err = (got[:n, i] - want.detach()[:n, i]).abs().max().item()
        assert err < 2e-4 * max(1.0, want.detach()[:n, i].abs().max().item()), (i, err)
    # (2) objective / derivative vs the oracle, on the device's own logits
    total, grad_o = 0.0, torch.zeros(T, B, P, dtype=torch.float64)
    for i, n in enumerate(lens):
        s = sups[i]
        fst = R.NumFstRef(s.num_states, s.src, s.dst, s.pdf, s.arc_weight, s.final_states, s.final_weights, s.state_time)
        objf, dg, _ = R.chain_objf_and_deriv(got[:n, i].double().numpy(), dref, fst, leaky=1e-4, xent_regularize=0.1)
        total += objf
        grad_o[:n, i] = torch.from_numpy(dg)
    assert abs(loss.item() - total) <= 1e-3 * abs(total), (loss.item(), total)
    assert (dlogits.double() + grad_o).abs().max().item() < 1e-4
    if not param_grads:
        return
    # (3) parameter gradients of the composition: torch CPU autograd fed with the gradient the device put at the logits
    # (checked against the oracle above), with the same modules in float64 as the truth and the reference's float32 CPU
    # run beside it.  In float32 a ReLU input that is ~0 can land on the other side of the kink than in float64 (FFN and
    # conv ReLUs of 12 layers x 120 rows x 2560 units); one such flip moves the gradients of everything upstream of it by
    # ~1e-3 of their size -- in the device run AND in the reference's float32 run, at different layers (measured:
    # device 1e-6 for layers 1..11 and 5e-3 at layer 0; torch float32 CPU 1e-3 from layer 5 down).  So: every tensor
    # within 3e-2 of the truth in relative Frobenius norm, and the tensors no flip can reach (output layer, final norm:
    # behind the last ReLU) within 1e-5.
    (want * dlogits).sum().backward()
    ref64 = copy.deepcopy(ref).double()
    for p_ in ref64.parameters():
        p_.grad = None
    want64 = _reference_forward(ref64, x.double(), None, kpm)
    (want64 * dlogits.double()).sum().backward()
    g32, g64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    e_dev, e_cpu = [], []
    names = [n for n, _ in md.named_parameters()]
    for name, p in md.named_parameters():
        truth = g64[name].grad
        scale = max(1e-12, truth.norm().item())
        e_dev.append((p.grad.cpu().double() - truth).norm().item() / scale)
        e_cpu.append((g32[name].grad.double() - truth).norm().item() / scale)
        assert e_dev[-1] < 3e-2, (name, e_dev[-1], e_cpu[-1])
    e_dev, e_cpu = np.array(e_dev), np.array(e_cpu)
    print("12-layer transformer + LF-MMI: objective %.4f (oracle %.4f); parameter gradients vs float64 (relative Frobenius "
          "error per tensor): device median %.1e max %.1e, %d of %d tensors < 1e-4; reference float32 CPU median %.1e max "
          "%.1e, %d < 1e-4" % (loss.item(), total, np.median(e_dev), e_dev.max(), (e_dev < 1e-4).sum(), len(e_dev),
                               np.median(e_cpu), e_cpu.max(), (e_cpu < 1e-4).sum()))
    for n_, e_ in zip(names, e_dev):
        if n_.startswith("output_layer.") or n_.startswith("transformer.norm."):
            assert e_ < 1e-5, (n_, e_)


@pytest.mark.parametrize("tag", ["small", "heads16"])
def test_transformer_matches_reference_golden(golden, tag):
    """tests/golden/transformer.npz is written by tools/gen_golden.py::gen_transformer, which IMPORTS the reference's
    models/transformer.py (TransformerAM, TransformerEncoderLayerWithConv1d) and runs its layers on CPU: the reference's
    own state_dict loads with strict=True, logits and all parameter gradients match (head size 64 = fused attention with a
    look-ahead mask; head size 16 = the batched-GEMM attention; padded keys in both)."""
    g = golden("transformer")
    D, C, H, FF, L, P, T, B, look = (int(v) for v in g[tag + "_cfg"])
    m = transformer.TransformerAM(D, C, H, FF, L, 0.0, P)
    sd = {k[len(tag) + 7:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag + "_param_")}
    sd["pos_encoder.pe"] = m.state_dict()["pos_encoder.pe"]
    assert np.abs(sd["pos_encoder.pe"][:8].numpy() - g[tag + "_pe_head"]).max() < 1e-6      # (libm of the box)
    m.load_state_dict(sd, strict=True)
    lens = [int(v) for v in g[tag + "_lens"]]
    kpm = torch.ones(B, T)
    for i, n in enumerate(lens):
        kpm[i, :n] = 0
    src_mask = None
    if look > -1:
        tri = torch.tril(torch.ones(T, T), diagonal=look)
        src_mask = tri.float().masked_fill(tri == 0, float("-inf")).masked_fill(tri == 1, 0.0).cuda()
    m = m.cuda().train()
    got = m(torch.from_numpy(g[tag + "_x"]).cuda(), src_mask, kpm.bool().cuda())
    want = torch.from_numpy(g[tag + "_logits"])
    valid = torch.zeros(T, B, dtype=torch.bool)
    for i, n in enumerate(lens):
        valid[:n, i] = True
    err = (got.cpu() - want)[valid].abs().max().item()
    assert err < 2e-4 * max(1.0, want[valid].abs().max().item()), err
    (got * torch.from_numpy(g[tag + "_w"]).cuda()).sum().backward()
    for name, p in m.named_parameters():
        rg = torch.from_numpy(g[tag + "_grad_" + name])
        e = (p.grad.cpu() - rg).abs().max().item()
        assert e < 5e-4 * max(1e-2, rg.abs().max().item()), (name, e, rg.abs().max().item())


def _tr_run(L, T, B, P, seed=0, FF=2048):
    torch.manual_seed(seed)
    m = transformer.TransformerAM(80, 512, 8, FF, L, 0.0, P)
    for lp in m.transformer.layers:
        for p in lp.parameters():
            p.data.add_(0.02 * torch.randn_like(p))
    m = m.cuda().train()
    x = torch.randn(T, B, 80).cuda()
    kpm = torch.zeros(B, T, dtype=torch.bool)
    kpm[-1, T - 7:] = True
    w = torch.randn(T, B, P).cuda()
    w[T - 7:, -1] = 0
    y = m(x, None, kpm.cuda())
    (y * w).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), {n: p.grad.detach().cpu() for n, p in m.named_parameters()}


def test_default_schedule_forward_is_bitwise_reproducible_and_gradients_repeat():
    """VERDICT r5 #6a / ADVICE r5: the product's DEFAULT GEMM schedule (no PK2_GEMM_SPLITK), 12 layers, P = 6048, five runs of
    the same forward + backward.  The forward pass holds no atomically added slices, so the logits are equal bit for bit;
    the weight gradients and the dX products keep their K slices (float atomics: summation order varies), which may move a
    gradient by rounding noise only -- measured run-to-run spread up to 1.7e-6 of a tensor's maximum, bound 2e-5 (a flipped
    ReLU mask element, the round-5 failure, moves a tensor by 2e-3..2e-2 of its maximum)."""
    runs = [_tr_run(12, 60, 2, 6048) for _ in range(5)]
    y0, g0 = runs[0]
    assert torch.isfinite(y0).all()
    worst = 0.0
    for y, g in runs[1:]:
        assert torch.equal(y, y0)
        for n in g0:
            spread = (g[n] - g0[n]).abs().max().item() / max(1e-6, g0[n].abs().max().item())
            worst = max(worst, spread)
            assert spread < 2e-5, (n, spread)
    print("run-to-run gradient spread over 5 runs: %.2e of a tensor's maximum" % worst)


def test_side_stream_on_and_off_give_the_same_gradients(monkeypatch):
    """the backward pass runs its weight-gradient products on a side stream behind event fences by default
    (PK2_TR_SIDE_STREAM=1); a missing fence would show as a gradient computed from a buffer that is being overwritten."""
    monkeypatch.setenv("PK2_TR_SIDE_STREAM", "1")
    y1, g1 = _tr_run(4, 90, 3, 300)
    monkeypatch.setenv("PK2_TR_SIDE_STREAM", "0")
    y0, g0 = _tr_run(4, 90, 3, 300)
    assert torch.equal(y1, y0)
    for n in g0:
        e = (g1[n] - g0[n]).abs().max().item()
        assert e < 5e-6 * max(1e-6, g0[n].abs().max().item()), (n, e)


@pytest.mark.parametrize("arith", [0, 1], ids=["f32", "bf16x3"])
@pytest.mark.parametrize("M,N,K", [(2276, 2048, 512), (130, 96, 72), (2276, 512, 1536), (300, 2048, 512)])
def test_gemm_act_epilogues_equal_the_product_followed_by_the_row_pass(M, N, K, arith):
    """pk2_gemm_f32_act: act 1 = ReLU behind x W^T + b (models/transformer.py:60, linear1 -> F.relu), act 2 = the ReLU's
    backward mask (kept where the forward activation > 0) behind the dX product, with and without beta = 1 -- the same
    arithmetic as pk2_gemm_f32 followed by pk2_relu_fwd / pk2_relu_bwd, so bit-equal to that pair."""
    import ctypes
    from pykaldi2_amd import _lib
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    sp = _lib.stream_ptr()
    prev = L.pk2_gemm_get_arith()
    _lib.check(L.pk2_gemm_set_arith(arith))
    try:
        g = torch.Generator(device="cuda").manual_seed(M + N + K)
        A = torch.randn(M, K, device="cuda", generator=g)
        W = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5
        b = torch.randn(N, device="cuda", generator=g)
        two, one = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
        _lib.check(L.pk2_gemm_f32(0, 1, M, N, K, 1.0, p(A), K, p(W), K, 0.0, p(two), N, p(b), sp))
        _lib.check(L.pk2_relu_fwd(p(two), two.numel(), sp))
        _lib.check(L.pk2_gemm_f32_act(0, 1, M, N, K, 1.0, p(A), K, p(W), K, 0.0, p(one), N, p(b), 1, None, 0, sp))
        assert torch.equal(one, two)
        ref = torch.relu(A.double().cpu() @ W.double().cpu().t() + b.double().cpu())
        assert (one.cpu().double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
        rms_b, max_b = G.STAT_BOUND["f32" if arith == 0 else "bf16x3"]
        rms, mx = G.err_units(one.cpu().numpy(), A.cpu().numpy(), W.cpu().numpy().T, bias=b.cpu().numpy(), want=ref.numpy())
        assert rms <= rms_b and mx <= 2 * max_b, (rms, mx)
        # backward mask, beta = 0 and beta = 1 (the residual sum the attention block's last dX product adds into)
        Wd = torch.randn(K, N, device="cuda", generator=g) / K ** 0.5
        gate = torch.randn(M, N, device="cuda", generator=g)
        base = torch.randn(M, N, device="cuda", generator=g)
        for beta in (0.0, 1.0):
            two, one = base.clone(), base.clone()
            _lib.check(L.pk2_gemm_f32(0, 0, M, N, K, 1.0, p(A), K, p(Wd), N, beta, p(two), N, None, sp))
            _lib.check(L.pk2_relu_bwd(p(gate), p(two), two.numel(), sp))
            _lib.check(L.pk2_gemm_f32_act(0, 0, M, N, K, 1.0, p(A), K, p(Wd), N, beta, p(one), N, None, 2, p(gate), N, sp))
            assert torch.equal(one, two), beta
        assert L.pk2_gemm_f32_act(0, 0, M, N, K, 1.0, p(A), K, p(Wd), N, 0.0, p(one), N, None, 2, None, N, sp) != 0     # act 2 needs a gate
    finally:
        _lib.check(L.pk2_gemm_set_arith(prev))


def test_relu_in_the_product_epilogues_changes_no_bit(monkeypatch):
    """PK2_TR_FUSE_RELU=1 (default: ReLU / ReLU' in the epilogues of linear1, of linear2's dX and of the attention block's last
    dX product) against the separate row passes: same logits, same gradients."""
    monkeypatch.setenv("PK2_TR_SIDE_STREAM", "0")
    monkeypatch.setenv("PK2_TR_FUSE_RELU", "1")
    y1, g1 = _tr_run(4, 90, 3, 300)
    monkeypatch.setenv("PK2_TR_FUSE_RELU", "0")
    y0, g0 = _tr_run(4, 90, 3, 300)
    assert torch.equal(y1, y0)
    for n in g0:
        e = (g1[n] - g0[n]).abs().max().item()
        assert e < 5e-6 * max(1e-6, g0[n].abs().max().item()), (n, e)


@pytest.mark.parametrize("rows,C", [(2276, 512), (37, 512), (1000, 256), (513, 1024), (300, 80)])
def test_layernorm_backward_matches_float64(rows, C):
    """pk2_layernorm_bwd against oracle/attention_ref.py::layernorm_bwd in float64 (itself held to autograd in
    tests/test_oracle_attention.py) on the float32 tensors the kernel reads, under the bound of tests/bound_check.py:
    4 * max(error of the float32 oracle, 2^-23 * max |tensor|), where this test used to allow 2e-5 * max(1, max |gradient|) --
    the new bound is asserted to be the tighter one at every shape.  dgamma / dbeta are accumulated onto what the buffers
    hold, so they are held to (what they held) + (the gradient).  (Round 6: a one-launch form -- rows per wave, partial
    parameter gradients added by the last workgroup to arrive -- passed this test and was dropped: 40 us per call against 8.7
    for the two launches; the agent-scope release in front of the arrival counter writes the XCD's dirty L2 lines back.)"""
    import ctypes
    import bound_check
    from oracle import attention_ref
    from pykaldi2_amd import _lib
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    sp = _lib.stream_ptr()
    torch.manual_seed(rows + C)
    s = (torch.randn(rows, C, dtype=torch.float64) * 2 + 0.3).float()
    gamma = torch.randn(C, dtype=torch.float64).float()
    dy = torch.randn(rows, C, dtype=torch.float64).float()
    mean = s.double().mean(1).float()
    rstd = (1.0 / torch.sqrt(s.double().var(1, unbiased=False) + 1e-5)).float()
    host = [t.numpy() for t in (dy, s, mean, rstd, gamma)]
    r64, r32 = (attention_ref.layernorm_bwd(*host, dtype=dt) for dt in (np.float64, np.float32))
    dev = lambda t: t.cuda().contiguous()      # noqa: E731
    s_d, dy_d, mean_d, rstd_d, gamma_d = dev(s), dev(dy), dev(mean), dev(rstd), dev(gamma)
    names = ("ds", "dgamma", "dbeta")
    for rep in range(2):
        ds = torch.full((rows, C), float("nan"), device="cuda")
        dg0, db0 = torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
        dg, db = dg0.clone(), db0.clone()
        _lib.check(L.pk2_layernorm_bwd(p(dy_d), p(s_d), p(mean_d), p(rstd_d), p(gamma_d), rows, C, p(ds), p(dg), p(db), sp))
        was = (np.zeros((rows, C), np.float32), dg0.cpu().numpy(), db0.cpu().numpy())
        ref64 = {n: w.astype(np.float64) + v for n, w, v in zip(names, was, r64)}
        ref32 = {n: w + v for n, w, v in zip(names, was, r32)}
        got = dict(ds=ds.cpu().numpy(), dgamma=dg.cpu().numpy(), dbeta=db.cpu().numpy())
        failures, ratios = bound_check.compare(got, ref64, ref32, names)
        for n in names:
            print("attention_ratio | layernorm_bwd-%dx%d-rep%d | %s | %.3f" % (rows, C, rep, n, ratios[n]))
            # never looser than the bound this test had: 2e-5 * max(1, max |gradient|)
            assert bound_check.FACTOR * bound_check.unit(ref64[n], ref32[n])[0] <= 2e-5 * max(1.0, float(np.abs(r64[names.index(n)]).max())), n
        assert failures == [], (rep, failures)


@pytest.mark.parametrize("arith", [0, 1], ids=["f32", "bf16x3"])
@pytest.mark.parametrize("R,B,C", [(2276, 4, 512), (90, 3, 64), (7, 7, 64), (301, 1, 128)])
def test_segmented_product_is_the_three_tap_convolution(R, B, C, arith):
    """pk2_gemm_f32_seg over three row-shifted views of a zero-padded [B + R + B, C] buffer against F.conv1d(k = 3,
    padding = 1) in float64 (time-major rows: frame t of utterance b is row t B + b), forward (+ bias + ReLU) and the
    transposed product of the input gradient (negative segment stride); R = B is a one-frame minibatch: only padding
    either side."""
    import ctypes
    from pykaldi2_amd import _lib
    L = _lib.lib()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)        # noqa: E731
    sp = _lib.stream_ptr()
    prev = L.pk2_gemm_get_arith()
    _lib.check(L.pk2_gemm_set_arith(arith))
    try:
        torch.manual_seed(R + B + C)
        T = R // B
        conv = torch.nn.Conv1d(C, C, 3, padding=1).double()
        x = torch.randn(T, B, C, dtype=torch.float64, requires_grad=True)
        want = F.relu(conv(x.permute(1, 2, 0))).permute(2, 0, 1)              # [T, B, C]
        dy = torch.randn(T, B, C, dtype=torch.float64)
        pre = conv(x.permute(1, 2, 0)).permute(2, 0, 1)
        pre.backward(dy)
        Wp = conv.weight.detach().permute(2, 0, 1).contiguous().float().cuda()        # [3][Cout][Cin]
        bias = conv.bias.detach().float().cuda()
        xp = torch.zeros(R + 2 * B, C, device="cuda")
        xp[B:B + R] = x.detach().reshape(R, C).float().cuda()
        y = torch.empty(R, C, device="cuda")
        _lib.check(L.pk2_gemm_f32_seg(0, 1, R, C, C, 3, 1.0, p(xp), C, B * C, p(Wp), C, C * C, 0.0, p(y), C, p(bias), 1, None, 0, sp))
        scale = max(1.0, want.abs().max().item())
        assert (y.cpu().double() - want.detach().reshape(R, C)).abs().max().item() < 2e-5 * scale
        # in units of sum |x w| + |bias| over the three taps, against the float32 operands the device multiplied
        xh, Wh, bh = xp.cpu().numpy(), Wp.cpu().numpy(), bias.cpu().numpy()
        Acat = np.concatenate([xh[j * B:j * B + R] for j in range(3)], 1)
        Bcat = np.concatenate([Wh[j].T for j in range(3)], 0)
        rms_b, max_b = G.STAT_BOUND["f32" if arith == 0 else "bf16x3"]
        rms, mx = G.err_units(y.cpu().numpy(), Acat, Bcat, bias=bh, want=np.maximum(G.gemm_exact(Acat, Bcat, bias=bh), 0.0))
        assert rms <= rms_b and mx <= 2 * max_b, (rms, mx)
        dcp = torch.zeros(R + 2 * B, C, device="cuda")
        dcp[B:B + R] = dy.reshape(R, C).float().cuda()
        dx = torch.empty(R, C, device="cuda")
        _lib.check(L.pk2_gemm_f32_seg(0, 0, R, C, C, 3, 1.0, p(dcp, 2 * B * C), C, -B * C, p(Wp), C, C * C, 0.0, p(dx), C, None, 0,
                                      None, 0, sp))
        gx = x.grad.reshape(R, C)
        assert (dx.cpu().double() - gx).abs().max().item() < 2e-5 * max(1.0, gx.abs().max().item())
    finally:
        _lib.check(L.pk2_gemm_set_arith(prev))


def test_convolution_as_one_product_against_three(monkeypatch):
    """PK2_TR_FUSE_CONV=1 (default) against the three accumulated products + ReLU pass: logits within the products' rounding
    (one accumulator over K = 3 C instead of three sums added in f32), gradients likewise."""
    monkeypatch.setenv("PK2_TR_SIDE_STREAM", "0")
    monkeypatch.setenv("PK2_TR_FUSE_CONV", "1")
    y1, g1 = _tr_run(4, 90, 3, 300)
    monkeypatch.setenv("PK2_TR_FUSE_CONV", "0")
    y0, g0 = _tr_run(4, 90, 3, 300)
    assert (y1 - y0).abs().max().item() < 2e-5 * max(1.0, y0.abs().max().item())
    for n in g0:       # (Frobenius norm: an activation within rounding of zero may flip its ReLU mask between the two forms)
        e = (g1[n] - g0[n]).norm().item()
        assert e < 5e-3 * max(1e-6, g0[n].norm().item()), (n, e)


_ATTN_SKIP_SNIPPET = r"""
import ctypes, sys, numpy as np, torch
sys.path.insert(0, %r)
from pykaldi2_amd import _lib
L = _lib.lib(); sp = _lib.stream_ptr()
p = lambda t: ctypes.c_void_p(t.data_ptr())
T, B, H, d = 200, 4, 2, 64
C = H * d
g = torch.Generator(device="cuda").manual_seed(7)
qkv = torch.randn(T, B, 3 * C, device="cuda", generator=g)
lens = [200, 33, 1, 150]
kpm = torch.zeros(B, T, dtype=torch.uint8, device="cuda")
for b, n in enumerate(lens):
    kpm[b, n:] = 1
kpm[3, 40:100] = 1                                 # padding with a hole behind it
dctx = torch.randn(T, B, C, device="cuda", generator=g)
for b, n in enumerate(lens):
    dctx[min(T, n + 5):, b] = 0.0                  # no loss term reaches frames far behind an utterance's end
ctx = torch.empty(T, B, C, device="cuda"); lse = torch.empty(B * H, T, device="cuda")
_lib.check(L.pk2_attention_fwd(p(qkv), T, B, H, d, 0.125, None, p(kpm), 0.1, 99, p(ctx), p(lse), sp))
dqkv = torch.full((T, B, 3 * C), float("nan"), device="cuda"); dsum = torch.empty(B * H, T, device="cuda")
_lib.check(L.pk2_attention_bwd(p(qkv), p(ctx), p(dctx), p(lse), T, B, H, d, 0.125, None, p(kpm), 0.1, 99, p(dqkv), p(dsum), sp))
torch.cuda.synchronize()
np.savez(sys.argv[1], ctx=ctx.cpu().numpy(), lse=lse.cpu().numpy(), dqkv=dqkv.cpu().numpy())
"""


def test_attention_padding_shortcuts_change_no_bit(tmp_path):
    """PK2_ATTN_SKIP_PAD (read once per process, hence two child processes): loops that end at the last valid key tile and
    backward kernels that leave all-zero output-gradient tiles out, against kernels that walk everything -- ctx, lse and
    dqkv equal bit for bit (ragged lengths, a one-key utterance, padding with a hole, dropout on the probabilities)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for mode in ("0", "3"):
        out = str(tmp_path / ("attn_%s.npz" % mode))
        env = dict(os.environ, PK2_ATTN_SKIP_PAD=mode)
        r = subprocess.run([sys.executable, "-c", _ATTN_SKIP_SNIPPET % root, out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(out))
    for k in ("ctx", "lse", "dqkv"):
        a, b = outs[0][k], outs[1][k]
        assert np.isfinite(b[np.isfinite(a)]).all()
        assert np.array_equal(a, b, equal_nan=True), k
    assert np.isfinite(outs[1]["dqkv"]).all()       # every element written
