"""Teacher-student timing on the `bench.py --se` minibatch: 8 LibriSpeech-shaped utterances (data.SyntheticSource, seed 7) through
the untrained 3x512 BLSTM, P = 5768, the 20000-word synthetic HCLG, beam 13 / lattice beam 7 / max_active 7000 / acoustic
scale 0.1 -- the lattices `lat_fb_alpha_beta_lin` works on in the bench.  The student's log-likelihoods come from a second
untrained model (seed 1), time-major as the BLSTM leaves them.  On ONE decoded batch it times, per call (median / min / max of
--reps, events around a synchronise): LatticeBatch.mmi (the chain of the bench step), LatticeBatch.teacher_student,
LatticeBatch.rescore and LatticeBatch.posteriors, all at lattice_scale(1.0, 0.2).  teacher_student leaves the lattice rescored
with the same student scores every time (old_acoustic_scale 0), so every repetition works on lattices of the same shape; the
mmi chain is timed first, on the teacher's scores.  Prints one JSON line and, with --out FILE, writes it there too
(profiles/ts_time.txt).  Run it under `rocprofv3 --kernel-trace --stats -- python tools/ts_time.py` for the per-kernel split."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import data, fbank, lattice, lstm, se, synth  # noqa: E402


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    PS, N, dev = 5768, 8, torch.device("cuda")
    words = int(os.environ.get("PK2_SE_WORDS", "20000"))
    fb = fbank.FbankExtractor()
    tm = lattice.TransitionModel.from_arrays(synth.transition_model_arrays(PS))      # (as bench.py --se)
    o = lattice.LatticeFasterDecoderOptions(beam=13.0, lattice_beam=7.0, max_active=7000, min_active=200)
    rec = lattice.MappedLatticeFasterRecognizer(tm, synth.decoding_graph_arcs(words, PS, seed=0), acoustic_scale=0.1,
                                                decoder_opts=o)
    src = data.SyntheticSource(PS, seed=7, rank=0, world=1, with_tids=True)
    utts = [src.draw() for _ in range(N)]
    wav = torch.from_numpy(np.concatenate([u[0] for u in utts])).to(dev)
    prior = se.log_prior_from_counts(np.ones(PS)).to(dev)
    preds = []
    with torch.no_grad():
        feats, frames, row_off = fb(wav, [u[0].shape[0] for u in utts])
        x = fb.pad_roll_subsample(feats, row_off, frames, shift=0, subsample=1, time_major=True)
        for seed in (0, 1):
            torch.manual_seed(seed)
            model = lstm.LSTMAM(80, PS, 512, 3, 0.0, True).to(dev).eval()
            preds.append(model.forward_time_major(x).transpose(0, 1) - prior)
            del model
    pred_T, pred_S = preds
    lens = [int(t) for t in frames]
    lat = rec.decode_batch(pred_T, lens)
    ali = [u[2] for u in utts]
    out = dict(frames=lens, tokens=int(np.sum(lat.num_tokens)), links=int(np.sum(lat.num_links)), reps=reps)

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
        return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3),
                    max_ms=round(float(np.max(ms)), 3))

    out["mmi"] = timed(lambda: lat.mmi(ali, 1.0, 0.2, True))
    out["posteriors"] = timed(lambda: lat.posteriors(1.0, 0.2))
    out["teacher_student"] = timed(lambda: lat.teacher_student(pred_S, 1.0, 0.2, 0.0))
    out["rescore"] = timed(lambda: lat.rescore(pred_S, 0.0))
    fresh = rec.decode_batch(pred_T, lens)
    loss, _ = fresh.teacher_student(pred_S, 1.0, 0.2, 0.0)
    out["loss"] = [round(float(v), 4) for v in loss.cpu()]
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
