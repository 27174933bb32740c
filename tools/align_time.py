"""Forced-alignment timing on a bench-size minibatch (bench.py --se: 8 LibriSpeech-shaped utterances at 100 fps, P = 5768,
the synthetic lexicon of a 20000-word HCLG): host compile time per utterance and device Viterbi time per launch / per frame,
for the LDS and the global-memory path.  One JSON line.  Run it under `rocprofv3 --kernel-trace --stats -- python ...` for
the kernel's own time."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import chain, synth  # noqa: E402


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    P, words, N = 5768, int(os.environ.get("PK2_SE_WORDS", "20000")), 8
    tree, tm = synth.alignment_model(P)
    aligner = chain.MappedAligner.from_models(tm, tree, synth.lexicon_arcs(words, P, seed=0), beam=10.0, transition_scale=1.0,
                                              self_loop_scale=0.1, acoustic_scale=0.1)
    rng = np.random.default_rng(7)
    frames = [int(d * 100) for d in synth.utterance_durations(rng, N)]
    texts = [synth.word_transcript(rng, T, words) for T in frames]
    t0 = time.perf_counter()
    for _ in range(reps):
        graphs = aligner.compile(texts, frames)
    compile_ms = (time.perf_counter() - t0) * 1e3 / reps
    x = (2.0 * torch.randn(N, max(frames), P, device="cuda")).float()
    out = dict(frames=frames, words=[len(t) for t in texts], states=graphs.num_states, arcs=graphs.num_arcs,
               compile_ms_per_utt=round(compile_ms / N, 3))
    for lds in ("1", "0"):
        os.environ["PK2_ALIGN_LDS"] = lds
        chain.align_viterbi(graphs, x, 0.1, 10.0)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, _, status = chain.align_viterbi(graphs, x, 0.1, 10.0)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        out["lds" if lds == "1" else "global"] = dict(uses_lds=graphs.uses_lds(), launch_ms=round(float(np.median(ms)), 3),
                                                      us_per_frame=round(float(np.median(ms)) * 1e3 / max(frames), 3),
                                                      status=status.cpu().tolist())
    t0 = time.perf_counter()
    for _ in range(reps):
        r = aligner.align_batch(x, frames, texts)
    out["align_batch_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 3)
    out["aligned"] = sum(v is not None for v in r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
