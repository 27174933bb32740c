"""LSTMAM -- drop-in for reference models/lstm.py:33-61 running on libpk2hip.so.

Same constructor, same ``state_dict`` keys (``lstm.weight_ih_l{k}[_reverse]``,
``lstm.weight_hh_l{k}[_reverse]``, ``lstm.bias_ih_l{k}[_reverse]``,
``lstm.bias_hh_l{k}[_reverse]``, ``output_layer.{weight,bias}``), same default
initialisation (parameters are created and initialised in the reference's order,
so ``torch.manual_seed(s)`` gives bit-identical weights), same semantics:
``forward(x[B,T,D]) -> logits[B,T,P]`` = Linear(LSTM(x)) with h0 = c0 = 0,
gate order i,f,g,o, every sequence run over all T frames (no packing).  The
reference's own forward has a typo (``self_output_layer``, models/lstm.py:59);
the intended computation is implemented.

All arithmetic is in libpk2hip.so: f32 MFMA GEMMs for the input / output
projections and every weight gradient, per-step recurrent MFMA kernels with the
gate math fused.  Parameters live in one flat buffer (and gradients in another)
so the optimiser and the gradient all-reduce each see a single contiguous
array; within a layer the two directions' matrices are adjacent, so both
directions share one GEMM.
"""
import math
import ctypes
import os

import torch
import torch.nn as nn

from . import _lib


def _gemm(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias=None, alpha=1.0, beta=0.0):
    _lib.check(_lib.lib().pk2_gemm_f32(int(ta), int(tb), M, N, K, alpha, A, lda, B, ldb, beta, C, ldc,
                                       bias, _lib.stream_ptr()))


def _p(t, off_floats=0):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * off_floats)


class _LSTMParams(nn.Module):
    """Parameter container with nn.LSTM's names, creation order and initialisation."""

    def __init__(self, input_size, hidden_size, num_layers, bidirectional):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.num_layers, self.bidirectional = num_layers, bidirectional
        D = 2 if bidirectional else 1
        H = hidden_size
        for layer in range(num_layers):
            for d in range(D):
                in_size = input_size if layer == 0 else H * D
                sfx = "_reverse" if d == 1 else ""
                self.register_parameter("weight_ih_l%d%s" % (layer, sfx), nn.Parameter(torch.empty(4 * H, in_size)))
                self.register_parameter("weight_hh_l%d%s" % (layer, sfx), nn.Parameter(torch.empty(4 * H, H)))
                self.register_parameter("bias_ih_l%d%s" % (layer, sfx), nn.Parameter(torch.empty(4 * H)))
                self.register_parameter("bias_hh_l%d%s" % (layer, sfx), nn.Parameter(torch.empty(4 * H)))
        stdv = 1.0 / math.sqrt(H) if H > 0 else 0
        for w in self.parameters():  # nn.LSTM.reset_parameters
            nn.init.uniform_(w, -stdv, stdv)


class _LinearParams(nn.Module):
    """nn.Linear's parameters and initialisation."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1 / math.sqrt(in_features) if in_features > 0 else 0
        nn.init.uniform_(self.bias, -bound, bound)


_row_map_cache = {}


def row_map_host(lengths, T, B):
    """(perm, Mv): perm is an int32 array of all T * B row indices of a time-major [T * B, .] matrix -- first the Mv rows
    t * B + b with t < lengths[b] (the frames that are not padding) in ascending order, then the padded rows in ascending
    order.  perm[:Mv] is the row map of pk2_gemm_f32_rows / pk2_gemm_f32_tn_colsum_rows, perm[Mv:] what pk2_rows_zero clears."""
    import numpy as np
    lens = np.asarray(lengths, dtype=np.int64)
    if lens.shape != (B,) or (lens < 0).any() or (lens > T).any():
        raise ValueError("lengths: one frame count in [0, T] per sequence (B = %d, T = %d): %r" % (B, T, list(lengths)))
    valid = (np.arange(T)[:, None] < lens[None, :]).reshape(-1)
    return np.concatenate([np.flatnonzero(valid), np.flatnonzero(~valid)]).astype(np.int32), int(valid.sum())


def _row_map(lengths, T, B, dev):
    """The device copy of row_map_host: the host array is built once per (lengths, T, B) and kept in pinned memory (a
    training run draws its minibatch lengths from a few thousand values of T and the bench from four); every step copies
    it non-blocking (4 T B bytes: 9 KB for the bench minibatch) in front of the forward's kernels.  (map, Mv) or None when
    nothing is padded."""
    key = (tuple(int(v) for v in lengths), T, B)
    hit = _row_map_cache.get(key)
    if hit is None:
        if len(_row_map_cache) >= 4096:
            _row_map_cache.clear()
        perm, mv = row_map_host(key[0], T, B)
        hit = _row_map_cache[key] = (torch.from_numpy(perm).pin_memory(), mv)
    host, mv = hit
    if mv == T * B or mv == 0:
        return None
    return host.to(dev, non_blocking=True), mv


def _p32(t, off_ints=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off_ints)


class _LstmAmFunction(torch.autograd.Function):
    """x_tm [T,B,Din] (time-major) -> logits_tm [T,B,P].  lengths (or None): frames per sequence -- the output layer's
    three products then run over the rows t * B + b, t < lengths[b], only (LSTMAM.forward_time_major)."""

    @staticmethod
    def forward(ctx, x_tm, model, lengths, *params):
        m = model
        T, B, Din = x_tm.shape
        H, D, Lr = m.hidden_size, m.num_dirs, m.num_layers
        dev = x_tm.device
        L = _lib.lib()
        sp = _lib.stream_ptr()
        rows = T * B
        saved = []
        seeds = []
        inp = x_tm.contiguous()
        for l in range(Lr):
            w_ih, w_hh, b_ih, b_hh = m._layer_views(l)
            in_size = inp.shape[-1]
            y = torch.empty(T, B, D * H, device=dev, dtype=torch.float32)
            gates = torch.empty(D, T, B, 4 * H, device=dev, dtype=torch.float32)
            cells = torch.empty(D, T, B, H, device=dev, dtype=torch.float32)
            nws = L.pk2_lstm_fwd_workspace_floats(B, H, D)
            ws = torch.empty(nws, device=dev, dtype=torch.float32) if nws else None
            # the one-launch recurrence of a few sequences multiplies inp by W_ih itself (lstm_fwd_seq2_xproj); where it does
            # not, the product is a GEMM in front of the recurrence as before
            gx_done = ctypes.c_int32(0)
            _lib.check(L.pk2_lstm_layer_fwd_xproj(None, _p(w_hh), _p(b_hh), B, T, H, D, _p(y), _p(gates), _p(cells),
                                                  _p(ws) if ws is not None else None, _p(inp), in_size, _p(w_ih), _p(b_ih),
                                                  ctypes.byref(gx_done), sp))
            if not gx_done.value:
                gx = torch.empty(T, B, D * 4 * H, device=dev, dtype=torch.float32)
                _gemm(0, 1, rows, D * 4 * H, in_size, _p(inp), in_size, _p(w_ih), in_size, _p(gx), D * 4 * H,
                      bias=_p(b_ih))
                _lib.check(L.pk2_lstm_layer_fwd(_p(gx), _p(w_hh), _p(b_hh), B, T, H, D, _p(y), _p(gates), _p(cells),
                                                _p(ws) if ws is not None else None, sp))
            saved.append((inp, y, gates, cells))
            inp = y
            if m.dropout > 0 and m.training and l + 1 < Lr:
                # nn.LSTM semantics: dropout on the outputs of every layer but the last; the recurrence
                # itself keeps reading the undropped h (y).  The seed comes from torch's CPU generator.
                seed = int(torch.empty((), dtype=torch.int64).random_().item()) & 0x7FFFFFFFFFFFFFFF
                seeds.append(seed)
                inp = torch.empty_like(y)
                _lib.check(L.pk2_dropout_f32(_p(y), _p(inp), y.numel(), float(m.dropout), seed, sp))
            else:
                seeds.append(None)
        P = m.output_size
        logits = torch.empty(T, B, P, device=dev, dtype=torch.float32)
        # the output layer is the one part of a BLSTM whose padded rows nobody reads (the layers below need them: the reverse
        # direction starts inside the padding): with lengths its product runs over the valid rows, the others are set to 0
        rm = _row_map(lengths, T, B, dev) if lengths is not None and os.environ.get("PK2_OUT_ROWS", "1") != "0" else None
        if rm is not None:
            rmap, mv = rm
            _lib.check(L.pk2_gemm_f32_rows(1, rows, P, D * H, 1.0, _p(inp), D * H, _p(m.output_layer.weight), D * H, 0.0,
                                           _p(logits), P, _p(m.output_layer.bias), _p32(rmap), mv, sp))
            _lib.check(L.pk2_rows_zero(_p(logits), P, P, _p32(rmap, mv), rows - mv, sp))
        else:
            _gemm(0, 1, rows, P, D * H, _p(inp), D * H, _p(m.output_layer.weight), D * H, _p(logits), P,
                  bias=_p(m.output_layer.bias))
        ctx.row_map = rm
        ctx.model = m
        ctx.saved = saved
        ctx.seeds = seeds
        ctx.shape = (T, B, Din)
        ctx.need_dx = x_tm.requires_grad
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        m = ctx.model
        T, B, Din = ctx.shape
        H, D, Lr, P = m.hidden_size, m.num_dirs, m.num_layers, m.output_size
        L = _lib.lib()
        sp = _lib.stream_ptr()
        rows = T * B
        dev = dlogits.device
        dlogits = dlogits.contiguous()
        gflat = m._grad_flat()
        # ONE memset of the flat gradient buffer, then every gradient product accumulates (beta = 1): a split-K GEMM no longer
        # needs its own zeroing launch (gemm_prescale_kernel), a column sum no scale_vec launch, and the bias gradients can
        # be added from inside the backward recurrence (pk2_lstm_layer_bwd_bias)
        gflat.zero_()
        views = m._grad_views(gflat)
        y_last = ctx.saved[-1][1]
        # The serial chain is  dlogits -> dy -> recurrence(l=L-1) -> dy -> recurrence(l=L-2) ...; the
        # weight / bias gradients hang off it and could overlap it on a side stream (PK2_SIDE_STREAM=1).
        # Measured on MI355X / ROCm 7.2: a second active stream slows the graph-replayed step chains of
        # the main stream by ~25 % (52.6 vs 48.5 ms per step), more than the overlap returns, so the
        # default keeps everything on the caller's stream.
        main = torch.cuda.current_stream(dev)
        side = m._side_stream(dev) if os.environ.get("PK2_SIDE_STREAM") == "1" else main

        def on_side(fn, *tensors):
            ev = torch.cuda.Event()
            ev.record(main)
            with torch.cuda.stream(side):
                side.wait_event(ev)
                fn()
            for t_ in tensors:
                t_.record_stream(side)

        # output layer: dy = dlogits W (critical path), dW = dlogits^T y, db = colsum(dlogits)
        gw, gb = views["output_layer.weight"], views["output_layer.bias"]
        dy = torch.empty(T, B, D * H, device=dev, dtype=torch.float32)
        rm = ctx.row_map
        if rm is not None:
            # rows of dlogits beyond a sequence's length are not read: dy is exactly 0 there, as it is for the zero rows a
            # loss writes (the backward recurrences below run over every row)
            rmap, mv = rm
            _lib.check(L.pk2_gemm_f32_rows(0, rows, D * H, P, 1.0, _p(dlogits), P, _p(m.output_layer.weight), D * H, 0.0,
                                           _p(dy), D * H, None, _p32(rmap), mv, sp))
            _lib.check(L.pk2_rows_zero(_p(dy), D * H, D * H, _p32(rmap, mv), rows - mv, sp))
        else:
            _gemm(0, 0, rows, D * H, P, _p(dlogits), P, _p(m.output_layer.weight), D * H, _p(dy), D * H)

        def out_grads():
            # weight and bias gradient in one launch (round 6: the column sums ride in the product's operand loader)
            if rm is not None and os.environ.get("PK2_OUT_ROWS_WGRAD", "map") == "pack":
                # (the measured alternative, DESIGN 4.2l: gather the valid rows, then today's product over K = Mv)
                dl_p = torch.empty(mv, P, device=dev, dtype=torch.float32)
                y_p = torch.empty(mv, D * H, device=dev, dtype=torch.float32)
                _lib.check(L.pk2_rows_pack(_p(dlogits), P, P, _p32(rmap), mv, _p(dl_p), P, _lib.stream_ptr()))
                _lib.check(L.pk2_rows_pack(_p(y_last), D * H, D * H, _p32(rmap), mv, _p(y_p), D * H, _lib.stream_ptr()))
                _lib.check(L.pk2_gemm_f32_tn_colsum(P, D * H, mv, 1.0, _p(dl_p), P, _p(y_p), D * H, 1.0, _p(gw), D * H, _p(gb),
                                                    _lib.stream_ptr()))
            elif rm is not None:
                _lib.check(L.pk2_gemm_f32_tn_colsum_rows(P, D * H, rows, 1.0, _p(dlogits), P, _p(y_last), D * H, 1.0, _p(gw),
                                                         D * H, _p(gb), _p32(rmap), mv, _lib.stream_ptr()))
            else:
                _lib.check(L.pk2_gemm_f32_tn_colsum(P, D * H, rows, 1.0, _p(dlogits), P, _p(y_last), D * H, 1.0, _p(gw), D * H,
                                                    _p(gb), _lib.stream_ptr()))
            m._bucket_ready("output_layer")
        on_side(out_grads, dlogits, y_last)
        scratch = torch.empty(L.pk2_lstm_bwd_scratch_floats(B, H, D), device=dev, dtype=torch.float32)
        dx = None
        for l in range(Lr - 1, -1, -1):
            inp, y, gates, cells = ctx.saved[l]
            in_size = inp.shape[-1]
            w_ih, w_hh, b_ih, b_hh = m._layer_views(l)
            gw_ih, gw_hh, gb_ih, gb_hh = m._layer_views(l, gflat)
            dgx = torch.empty(T, B, D * 4 * H, device=dev, dtype=torch.float32)
            bias_done = ctypes.c_int32(0)       # (the one-launch recurrence sums its d gates over the frames on the way)
            # ... and keeps its slices of dW_hh in MFMA accumulators (lstm_bwd_seq2_wgrad): the recurrence reads the undropped y
            whh_done = ctypes.c_int32(0)
            nws = L.pk2_lstm_bwd_wgrad_workspace_floats(B, H, D)
            wgrad_ws = torch.empty(nws, device=dev, dtype=torch.float32) if nws else None
            _lib.check(L.pk2_lstm_layer_bwd_wgrad(_p(dy), _p(w_hh), _p(gates), _p(cells), _p(y), B, T, H, D, _p(dgx), _p(scratch),
                                                  _p(gb_ih), _p(gb_hh), _p(gw_hh), _p(wgrad_ws) if nws else None,
                                                  ctypes.byref(bias_done), ctypes.byref(whh_done), sp))
            G = D * 4 * H

            def layer_grads(dgx=dgx, inp=inp, y=y, in_size=in_size, gw_ih=gw_ih, gw_hh=gw_hh, gb_ih=gb_ih,
                            gb_hh=gb_hh, l=l, bias_done=bool(bias_done.value), whh_done=bool(whh_done.value)):
                # dW_ih (both directions at once) = dgx^T inp; the bias gradients (b_ih and b_hh receive the same sum) with it
                # unless the one-launch recurrence has summed them already
                if not bias_done:
                    _lib.check(L.pk2_gemm_f32_tn_colsum(G, in_size, rows, 1.0, _p(dgx), G, _p(inp), in_size, 1.0, _p(gw_ih), in_size,
                                                        _p(gb_ih), _lib.stream_ptr()))
                    gb_hh.copy_(gb_ih)
                else:
                    _gemm(1, 0, G, in_size, rows, _p(dgx), G, _p(inp), in_size, _p(gw_ih), in_size, beta=1.0)
                # dW_hh[d] = sum_t dg_d[t]^T h_d[t-1] (reverse direction: h_d[t+1]); time-major => row shift by B
                # (unless the recurrence has added it on the way)
                if T > 1 and not whh_done:
                    k = (T - 1) * B
                    if D == 2:
                        # both directions in one batched launch (matrix 1 = matrix 0 + these strides: the reverse
                        # direction pairs dg[t] with h[t+1])
                        _lib.check(L.pk2_gemm_f32_batched(1, 0, 4 * H, H, k, 1.0, _p(dgx, B * G), G, 4 * H - B * G, 0,
                                                          _p(y), D * H, B * D * H + H, 0, 1.0, _p(gw_hh), H,
                                                          4 * H * H, 0, 2, 1, _lib.stream_ptr()))
                    else:
                        _gemm(1, 0, 4 * H, H, k, _p(dgx, B * G), G, _p(y), D * H, _p(gw_hh), H, beta=1.0)
                m._bucket_ready("lstm.l%d" % l)
            # critical path first (next layer's dy), weight gradients on the side stream
            if l > 0 or ctx.need_dx:
                dprev = torch.empty(T, B, in_size, device=dev, dtype=torch.float32)
                ev = torch.cuda.Event()
                ev.record(main)
                _gemm(0, 0, rows, in_size, G, _p(dgx), G, _p(w_ih), in_size, _p(dprev), in_size)
                with torch.cuda.stream(side):
                    side.wait_event(ev)
                    layer_grads()
                for t_ in (dgx, inp, y):
                    t_.record_stream(side)
                if l > 0:
                    dy = dprev
                    if ctx.seeds[l - 1] is not None:  # same mask and scale as the forward dropout of layer l-1
                        _lib.check(L.pk2_dropout_f32(_p(dy), _p(dy), dy.numel(), float(m.dropout), ctx.seeds[l - 1], sp))
                else:
                    dx = dprev
            else:
                on_side(layer_grads, dgx, inp, y)
        main.wait_stream(side)
        # Parameter gradients are published directly as views of the flat gradient buffer
        # (p.grad = gradient of THIS backward, which is what zero_grad -> backward -> step needs);
        # autograd gets None for them so nothing is copied or double-counted.
        params = dict(m.named_parameters())
        for name in m._param_names:
            p, v = params[name], views[name]
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                p.grad = v
        ctx.saved = None
        return (dx, None, None) + (None,) * len(m._param_names)


class LSTMAM(nn.Module):
    def __init__(self, input_size, output_size, hidden_size, num_layers, dropout, bidirectional):
        super().__init__()
        self.input_size = input_size
        self.output_size = output_size
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        self.dropout = dropout
        self.bidirectional = bidirectional
        self.num_dirs = 2 if bidirectional else 1
        # same creation order as the reference (output layer first, then the LSTM)
        self.output_layer = _LinearParams(hidden_size * self.num_dirs, output_size)
        self.lstm = _LSTMParams(input_size, hidden_size, num_layers, bidirectional)
        self._param_names = [n for n, _ in self.named_parameters()]
        self._flat = None
        self._gflat = None
        self._layout = None
        self._bucket_hook = None

    # ---- flat parameter / gradient storage -------------------------------------------
    def _flat_order(self):
        """Flat layout: output layer, then per layer [w_ih f,r][w_hh f,r][b_ih f,r][b_hh f,r]."""
        order = ["output_layer.weight", "output_layer.bias"]
        sfx = ["", "_reverse"][:self.num_dirs]
        for l in range(self.num_layers):
            for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                for s in sfx:
                    order.append("lstm.%s_l%d%s" % (kind, l, s))
        return order

    def _ensure_flat(self):
        params = dict(self.named_parameters())
        first = params["output_layer.weight"]
        if self._flat is not None and self._flat.device == first.device and all(
                params[n].data_ptr() == self._flat.data_ptr() + 4 * off for n, (off, _) in self._layout.items()):
            return
        order = self._flat_order()
        layout, off = {}, 0
        for n in order:
            cnt = params[n].numel()
            layout[n] = (off, cnt)
            off += (cnt + 63) // 64 * 64  # 256-byte aligned segments
        flat = torch.zeros(off, dtype=torch.float32, device=first.device)
        for n in order:
            o, cnt = layout[n]
            flat[o:o + cnt].copy_(params[n].data.reshape(-1))
            params[n].data = flat[o:o + cnt].view(params[n].shape)
        self._flat, self._layout = flat, layout
        self._gflat = None
        self._buckets = {}
        names = order
        def span(prefixes):
            sel = [layout[n] for n in names if any(n.startswith(p) for p in prefixes)]
            lo = min(o for o, _ in sel)
            hi = max((o + c + 63) // 64 * 64 for o, c in sel)
            return lo, hi
        self._buckets["output_layer"] = span(["output_layer."])
        for l in range(self.num_layers):
            self._buckets["lstm.l%d" % l] = span(["lstm.%s_l%d" % (k, l) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")])

    def flat_parameters(self):
        """(flat_param, flat_grad) 1-D tensors covering every parameter (fused optimiser / all-reduce)."""
        self._ensure_flat()
        return self._flat, self._grad_flat()

    def _grad_flat(self):
        self._ensure_flat()
        if self._gflat is None or self._gflat.device != self._flat.device:
            self._gflat = torch.zeros_like(self._flat)
        return self._gflat

    def _grad_views(self, gflat):
        params = dict(self.named_parameters())
        return {n: gflat[o:o + c].view(params[n].shape) for n, (o, c) in self._layout.items()}

    def _layer_views(self, l, flat=None):
        """(w_ih [D*4H,in], w_hh [D*4H,H], b_ih [D*4H], b_hh [D*4H]) of layer l, both directions adjacent."""
        flat = self._flat if flat is None else flat
        D, H = self.num_dirs, self.hidden_size
        in_size = self.input_size if l == 0 else H * D
        def seg(kind, cols):
            o, _ = self._layout["lstm.%s_l%d" % (kind, l)]
            n = D * 4 * H * cols
            return flat[o:o + n].view(D * 4 * H, cols) if cols > 1 else flat[o:o + D * 4 * H]
        return seg("weight_ih", in_size), seg("weight_hh", H), seg("bias_ih", 1), seg("bias_hh", 1)

    def _side_stream(self, dev):
        """The stream of the weight-gradient products under PK2_SIDE_STREAM=1; with PK2_SIDE_CU_PER_XCD=k a stream whose
        kernels only get the first k CUs of every XCD (pk2_stream_create_cu_mask), so that they share fewer CUs with the
        one-launch recurrences of the main stream (measured, round 5)."""
        st = getattr(self, "_side", None)
        if st is None or st.device != dev:
            k = int(os.environ.get("PK2_SIDE_CU_PER_XCD", "0"))
            if k > 0:
                h = ctypes.c_void_p()
                with torch.cuda.device(dev):
                    _lib.check(_lib.lib().pk2_stream_create_cu_mask(k, ctypes.byref(h)))
                st = torch.cuda.ExternalStream(h.value, device=dev)
                self._side_handle = h        # (lives as long as the model)
            else:
                st = torch.cuda.Stream(device=dev)
            self._side = st
        return st

    def _bucket_ready(self, name):
        if self._bucket_hook is not None:
            lo, hi = self._buckets[name]
            self._bucket_hook(name, self._gflat[lo:hi])

    # ---- forward ---------------------------------------------------------------------
    def forward_time_major(self, x_tm, lengths=None):
        """x_tm [T,B,D] -> logits [T,B,P] (time-major, the kernels' native layout).

        lengths: frames per sequence (B integers in [0, T]), or None.  Taken from the argument first, else from the
        attribute ``pk2_lengths`` of the tensor object x_tm (FbankExtractor.pad_roll_subsample records it there), else every
        row is computed as before.  With lengths the output layer and its three gradient products run over the rows
        t < lengths[b] only:  logits[t, b] is 0 for t >= lengths[b] (not W y + bias), and the rows of the logits' gradient
        beyond a sequence's length are IGNORED (treated as zero, whatever they hold).  The LSTM layers themselves still run
        over all T frames of every sequence, as nn.LSTM does on a padded batch, so the valid logits are what they are
        without lengths.  A caller whose loss reads logits of padded frames passes no lengths and an untagged tensor
        (``x_tm.detach()`` or any torch operation drops the attribute).  PK2_OUT_ROWS=0 (read per call) ignores lengths."""
        if lengths is None:
            lengths = getattr(x_tm, "pk2_lengths", None)
        if lengths is not None:
            lengths = tuple(int(v) for v in lengths)
            if len(lengths) != x_tm.shape[1] or min(lengths) < 0 or max(lengths) > x_tm.shape[0]:
                raise ValueError("lengths: one frame count in [0, T] per sequence, got %r for x_tm %r" % (lengths, tuple(x_tm.shape)))
        _lib.require_gpu()
        assert x_tm.is_cuda and x_tm.dtype == torch.float32
        self._ensure_flat()
        D, H = self.num_dirs, self.hidden_size
        for l in range(self.num_layers):  # adjacency of the two directions is what the GEMMs rely on
            in_size = self.input_size if l == 0 else H * D
            assert (4 * H * in_size) % 64 == 0 and (4 * H * H) % 64 == 0 and (4 * H) % 64 == 0
        params = [p for _, p in self.named_parameters()]
        return _LstmAmFunction.apply(x_tm, self, lengths, *params)

    def forward(self, data):
        """data [B,T,D] -> logits [B,T,P], contiguous like the reference's (callers do
        ``prediction.view(-1, P)``, bin/train_ce.py:189).  The copy out of the kernels' time-major
        layout is skipped by callers that use forward_time_major()."""
        x_tm = data.transpose(0, 1).contiguous()
        return self.forward_time_major(x_tm).transpose(0, 1).contiguous()
