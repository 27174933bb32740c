"""Numerator timing on the lengths of the LF-MMI bench minibatch: 4 utterances of 146 / 539 / 569 / 159 subsampled frames,
P = 6048, logits N(0, 2).

  (a) the alignment-free numerator (csrc/chain_num_graph.hip): seeded transcripts (synth.word_transcript) over the
      synthetic lexicon and monophone model of `train_chain.py -e2e -synthetic`; chain.num_graph_forward_backward, timed
      per call with events (median / min / max of --reps) and, per utterance alone, to see what the longest costs;
  (b) the alignment-based numerator (csrc/chain_num.hip) on supervisions of the same lengths built from synthetic
      alignments as bench.py builds them, inside chain.compute_chain_objf_and_deriv over a small denominator graph, with
      PK2_NUM_SIDE=1 so that its two launches (num_scores, num_fwd_bwd) are launches of their own;
  and the host time of both supervision builders (chain.graph_supervisions; chain.supervision_from_alignment x 4).

The per-launch kernel times come from the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o ng -- python tools/num_graph_time.py
Prints one JSON line; with --out FILE writes it there too."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import chain, synth  # noqa: E402

FRAMES = [146, 539, 569, 159]
P = 6048


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.normal(0, 2, size=(4, max(FRAMES), P)).astype(np.float32)).to(dev)

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
        return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), max_ms=round(float(np.max(ms)), 3))

    def host_ms(fn):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            t.append(1e3 * (time.perf_counter() - t0))
        return r, round(float(np.median(t)), 3)

    out = dict(frames=FRAMES, P=P, reps=reps)
    # (a) graphs of seeded transcripts
    tree, tm = synth.alignment_model(P)
    aligner = chain.MappedAligner.from_models(tm, tree, synth.lexicon_arcs(200, P, seed=0))
    text_rng = np.random.default_rng(1)
    texts = [synth.word_transcript(text_rng, T, 200) for T in FRAMES]
    gs, out["graph_build_host_ms"] = host_ms(lambda: chain.graph_supervisions(aligner, texts, FRAMES))
    assert gs.status == [0, 0, 0, 0], gs.errors
    out["words"] = [len(t) for t in texts]
    out["states"], out["arcs"] = gs.graphs.num_states, gs.graphs.num_arcs
    grad = torch.zeros_like(x)
    out["num_graph_call"] = timed(lambda: chain.num_graph_forward_backward(gs, x, grad=grad))
    out["us_per_frame_of_longest"] = round(1e3 * out["num_graph_call"]["median_ms"] / max(FRAMES), 3)
    alone = []
    for n, T in enumerate(FRAMES):
        one = chain.graph_supervisions(aligner, [texts[n]], [T])
        xn, gn = x[n:n + 1, :T], grad[n:n + 1, :T]
        alone.append(timed(lambda: chain.num_graph_forward_backward(one, xn, grad=gn))["median_ms"])
    out["num_graph_call_alone_ms"] = alone
    # (b) alignment-based supervisions of the same lengths, as bench.py builds them
    ctree, ctm = synth.chain_model(P, seed=0)
    caligner, sopts = chain.MappedAligner(ctm), chain.SupervisionOptions()
    alis = [synth.phone_tid_alignment(rng, 3 * T, ctm)[0] for T in FRAMES]
    sups, out["alignment_build_host_ms"] = host_ms(
        lambda: [chain.supervision_from_alignment(caligner, ctree, ctm, sopts, a) for a in alis])
    assert [s.frames_per_sequence for s in sups] == FRAMES
    den = chain.DenominatorGraph(synth.den_graph_arcs(400, 6000, P, seed=0, loop_pdf_differs=True), P)
    opts = chain.ChainTrainingOptions(leaky_hmm_coefficient=1e-4, xent_regularize=0.1)
    os.environ["PK2_NUM_SIDE"] = "1"
    for _ in range(reps + 1):
        chain.compute_chain_objf_and_deriv(opts, den, sups, x)
    torch.cuda.synchronize()
    del os.environ["PK2_NUM_SIDE"]
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
