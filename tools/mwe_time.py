"""N-best / MWE timing on the `bench.py --se` minibatch: 8 LibriSpeech-shaped utterances (data.SyntheticSource, seed 7) through
the untrained 3x512 BLSTM, P = 5768, the 20000-word synthetic HCLG, beam 13 / lattice beam 7 / max_active 7000 / acoustic
scale 0.1 -- the lattices `lat_fb_alpha_beta_lin` works on in the bench.  num_paths 16, reference mode and `distinct`.
Prints one JSON line with the device time of LatticeBatch.nbest's kernels and of LatticeBatch.mwe per call (median of
--reps, events around a synchronise).  Run it under `rocprofv3 --kernel-trace --stats -- python tools/mwe_time.py` for the
per-kernel split."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import _lib, data, fbank, lattice, lstm, se, synth  # noqa: E402


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    PS, N, dev = 5768, 8, torch.device("cuda")
    words = int(os.environ.get("PK2_SE_WORDS", "20000"))
    torch.manual_seed(0)
    model = lstm.LSTMAM(80, PS, 512, 3, 0.0, True).to(dev).eval()
    fb = fbank.FbankExtractor()
    _, tm = synth.alignment_model(PS)
    o = lattice.LatticeFasterDecoderOptions(beam=13.0, lattice_beam=7.0, max_active=7000, min_active=200)
    rec = lattice.MappedLatticeFasterRecognizer(tm, synth.decoding_graph_arcs(words, PS, seed=0), acoustic_scale=0.1,
                                                decoder_opts=o)
    src = data.SyntheticSource(PS, seed=7, rank=0, world=1, with_tids=True)
    utts = [src.draw() for _ in range(N)]
    wav = torch.from_numpy(np.concatenate([u[0] for u in utts])).to(dev)
    with torch.no_grad():
        feats, frames, row_off = fb(wav, [u[0].shape[0] for u in utts])
        x = fb.pad_roll_subsample(feats, row_off, frames, shift=0, subsample=1, time_major=True)
        pred = model.forward_time_major(x).transpose(0, 1) - se.log_prior_from_counts(np.ones(PS)).to(dev)
    lens = [int(t) for t in frames]
    lat = rec.decode_batch(pred.contiguous(), lens)
    rng = np.random.default_rng(7)
    texts = [synth.word_transcript(rng, T, words) for T in lens]
    out = dict(frames=lens, tokens=int(np.sum(lat.num_tokens)), links=int(np.sum(lat.num_links)), num_paths=16)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(float(np.median(ms)), 3), round(float(np.min(ms)), 3), round(float(np.max(ms)), 3)

    for distinct in (False, True):
        cfg = dict(lm_weight=1.0, am_weight=0.1, phone_level=False, rand_path=False, num_paths=16, equal_weight=False,
                   distinct=distinct)
        K, cap = 16, 2 * max(lens) + 8
        bufs = [torch.empty(s, dtype=torch.int32, device=dev) for s in ((N,), (N, K), (N, K), (N, K, cap), (N, K, max(lens)))]
        cost = torch.empty(N, K, dtype=torch.float32, device=dev)

        def nbest():        # the kernels of LatticeBatch.nbest without its read-back
            lat._nbest_call(_lib.lib().pk2_lattice_nbest, K, 1.0, 0.1, "words", distinct, _lib.ptr(bufs[0]), _lib.ptr(bufs[1]),
                            _lib.ptr(cost), _lib.ptr(bufs[2]), _lib.ptr(bufs[3]), _lib.ptr(bufs[4]), _lib.stream_ptr(dev))

        med, lo, hi = timed(nbest)
        mmed, mlo, mhi = timed(lambda: lat.mwe(texts, cfg))
        loss, _ = lat.mwe(texts, cfg)
        hyps = [len(h) for h in lat.nbest(K, 1.0, 0.1, "words", distinct)]
        out["distinct" if distinct else "reference"] = dict(nbest_ms=med, nbest_ms_min=lo, nbest_ms_max=hi, mwe_ms=mmed,
                                                           mwe_ms_min=mlo, mwe_ms_max=mhi, hypotheses=hyps,
                                                           loss=[round(float(v), 4) for v in loss.cpu()])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
