"""The lattice oracle on the device (WordLatticeBatch.oracle, ws_oracle_kernel in csrc/lattice_oracle.hip)
against the int64 restatement tests/oracle_ref.py on identical packed lattices.  Everything is an integer and every
comparison is ==: errors, the split into insertions, deletions and substitutions, the words and the arcs of the path.
Every device buffer of the calls is sentinel poisoned and surrounded by checked guard elements (score._DEBUG_GUARD)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mbr_ref as R  # noqa: E402
import oracle_ref as O  # noqa: E402
import test_gpu_score as GS  # noqa: E402  (its hand-made lattices)
from pykaldi2_amd import _lib, kaldi_io, lattice, score, synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("errors", "ins", "dele", "sub", "words", "arcs", "packed_arcs")


@pytest.fixture(autouse=True)
def poisoned_buffers():
    score._DEBUG_GUARD = True
    yield
    score._DEBUG_GUARD = False


def compare(lats, refs, skip_words=None, **kw):
    """One oracle() call on the lattices against the restatement, lattice by lattice; returns (packed, records)."""
    packed = [p if isinstance(p, score.PackedLattice) else score.pack_lattice(p) for p in lats]
    batch = score.WordLatticeBatch(packed)
    recs = batch.oracle(refs, **kw) if skip_words is None else batch.oracle(refs, skip_words=skip_words, **kw)
    assert len(recs) == len(packed)
    for P, ref, rec in zip(packed, refs, recs):
        want = O.oracle(P, ref, skip_words or ())
        assert rec["status"] == 0
        for f in FIELDS:
            assert rec[f] == want[f], (f, rec[f], want[f])
        assert rec["errors"] == rec["ins"] + rec["dele"] + rec["sub"]
    return packed, recs


def fan(n):
    """n one-word chains side by side: a level of n states and an end state with n incoming arcs."""
    return R.paths_lattice([([1 + k % 7], 1.0 / n) for k in range(n)])


@pytest.mark.parametrize("R_", (0, 1, 63, 64, 65, 127, 128, 129, 1023))
def test_reference_lengths_at_the_lane_chunk_edges(R_):
    rng = np.random.default_rng(R_)
    lats = [R.random_lattice(8, 4, 5, seed=s) for s in (0, 1)]
    refs = [rng.integers(1, 7, R_).tolist() for _ in lats]
    if R_ >= 8:                                              # the lattice's own words somewhere inside: matches far from j = 0
        for k, w in enumerate(R.posteriors(score.pack_lattice(lats[1]), R.SETTINGS[0])["words"][:4]):
            refs[1][R_ // 2 + k] = int(w)
    compare(lats, refs)


def test_reference_beyond_the_capacity_is_status_2_and_leaves_the_neighbours_alone():
    rng = np.random.default_rng(7)
    lats = [score.pack_lattice(R.random_lattice(8, 4, 5, seed=s)) for s in (0, 1, 2)]
    refs = [rng.integers(1, 7, n).tolist() for n in (5, score.MAX_POSITIONS + 1, 70)]
    recs = score.WordLatticeBatch(lats).oracle(refs)
    assert recs[1] == dict(errors=-1, ins=0, dele=0, sub=0, words=[], arcs=[], packed_arcs=[], status=2)
    for n in (0, 2):
        assert recs[n] == score.WordLatticeBatch([lats[n]]).oracle([refs[n]])[0] and recs[n]["status"] == 0
        assert recs[n]["errors"] == O.oracle(lats[n], refs[n])["errors"]


@pytest.mark.parametrize("name", ("single_arc", "all_epsilon", "parallel", "skips_levels", "level16", "level17", "level1030",
                                  "fan_in70"))
def test_shape_edges(name):
    lat = dict(single_arc=lambda: R.paths_lattice([([4], 1.0)]), all_epsilon=GS.all_epsilon, parallel=GS.parallel_arcs,
               skips_levels=lambda: R.random_lattice(8, 4, 5, seed=3), level16=lambda: fan(16), level17=lambda: fan(17),
               level1030=lambda: fan(1030), fan_in70=lambda: GS.fan_in(70, 1))[name]()
    P = score.pack_lattice(lat)
    refs = dict(single_arc=[[4], [5], [], [4, 4]], all_epsilon=[[], [3]], parallel=[[4, 6], [9], [4, 5, 6]],
                level16=[[3, 9, 2]], level17=[[9, 3, 2]], level1030=[[9, 2, 3]]).get(name, [[1, 2, 3], [2, 5, 1, 4, 3, 2, 2, 1]])
    if name == "skips_levels":
        lev = np.repeat(np.arange(P.depth + 1), np.diff(P.level_off))
        assert (lev[P.dst] - lev[P.src] > 1).any()
    if name.startswith("level"):
        n = int(name[5:])
        assert P.level_off[2] - P.level_off[1] == n and P.in_off[P.S] - P.in_off[P.S - 1] == n and len(refs[0]) == 3
    if name == "fan_in70":
        assert int(np.diff(P.in_off).max()) == 70
    if name == "parallel":
        assert P.src[0] == P.src[1] and P.dst[0] == P.dst[1]
    _, recs = compare([P] * len(refs), refs)
    if name == "all_epsilon":
        assert recs[0]["words"] == [] and recs[0]["errors"] == 0 and recs[1]["errors"] == 1 and recs[1]["dele"] == 1
    if name == "single_arc":
        assert [r["errors"] for r in recs] == [0, 1, 1, 1] and recs[0]["arcs"] == [0]


def test_ties_between_arcs_and_between_edit_types_follow_the_rule():
    cases = [([([5], 0.5), ([6], 0.5)], [7]),               # two arcs, both a substitution: the lower packed arc
             ([([6], 0.5), ([5], 0.5)], [7]),
             ([([2], 1.0)], [1, 2]),                          # match + deletion
             ([([1, 2], 1.0)], [2]),                          # insertion + match, not substitution + insertion
             ([([1], 1.0)], [2, 3]),                          # substitution + deletion: the arc before the deletion
             ([([1, 1], 1.0)], [1]),                          # which of two equal words matches
             ([([1, 2], 0.5), ([2, 1], 0.5)], [1, 1]),        # two paths of one error each, a substitution either way
             ([([1, 2, 3], 0.4), ([1, 3], 0.3), ([3], 0.3)], [1, 4, 3]),
             ([([0, 1], 0.5), ([1, 0], 0.5)], [1])]           # epsilon arcs: free steps on either side of the match
    packed, recs = compare([R.paths_lattice(c[0]) for c in cases], [c[1] for c in cases])
    assert recs[0]["words"] == [5] and recs[1]["words"] == [6] and recs[0]["sub"] == recs[1]["sub"] == 1
    assert [(r["ins"], r["dele"], r["sub"]) for r in recs[2:6]] == [(0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 0, 0)]
    assert recs[5]["packed_arcs"] == O.oracle(packed[5], [1])["packed_arcs"]


@pytest.mark.parametrize("shape", R.SHAPES)
def test_invariants_on_the_generator_lattices(shape):
    P = score.pack_lattice(R.random_lattice(*shape, seed=0))
    batch = score.WordLatticeBatch([P])
    rng = np.random.default_rng(11)
    ref = rng.integers(1, shape[2] + 2, P.depth).tolist()
    hyps = [w for w, _ in batch.best_path(score.sweep())[0]]
    rec = batch.oracle([ref])[0]
    want = O.oracle(P, ref)
    assert all(rec[f] == want[f] for f in FIELDS)
    assert all(rec["errors"] <= R.edit_distance(h, ref) for h in {tuple(h) for h in hyps})
    for h in {tuple(h) for h in hyps}:                      # a reference that is a path's words: nothing to correct
        r0 = batch.oracle([list(h)])[0]
        assert r0["errors"] == 0 and r0["words"] == list(h) and (r0["ins"], r0["dele"], r0["sub"]) == (0, 0, 0)


def test_skip_words():
    lat = R.paths_lattice([([3, 7, 4], 0.5), ([3, 5], 0.5)])
    _, plain = compare([lat], [[3, 4]])
    _, skipped = compare([lat], [[3, 4]], skip_words=(7,))
    _, empty = compare([lat], [[3, 4]], skip_words=())
    assert plain[0]["errors"] == 1 and skipped[0]["errors"] == 0 and skipped[0]["words"] == [3, 4] and empty == plain
    _, both = compare([lat], [[3, 7, 4]], skip_words=(7,))
    assert both[0]["errors"] == 1 and both[0]["dele"] == 1
    big = R.random_lattice(20, 8, 8, seed=0)
    ref = np.random.default_rng(2).integers(1, 9, 20).tolist()
    _, a = compare([big], [ref], skip_words=(2, 5))
    _, b = compare([big], [ref])
    assert a[0]["errors"] != b[0]["errors"] or a[0]["words"] != b[0]["words"]
    batch = score.WordLatticeBatch([big])                    # the labels are cached per skip set
    batch.oracle([ref], skip_words=(5, 2)); batch.oracle([ref], skip_words=[2, 5, 5]); batch.oracle([ref])
    assert sorted(batch._labels) == [(), (2, 5)]


def test_batches_runs_launch_splits_and_single_calls_give_the_same_bytes():
    rng = np.random.default_rng(5)
    shapes = [R.SHAPES[k % 6] for k in range(35)]
    lats = [score.pack_lattice(R.random_lattice(*s, seed=k)) for k, s in enumerate(shapes)]
    lens = [(0, 3, P.depth, 70, 130, 17, 31)[k % 7] for k, P in enumerate(lats)]
    refs = [rng.integers(1, s[2] + 2, n).tolist() for s, n in zip(shapes, lens)]
    _, whole = compare(lats, refs)
    batch = score.WordLatticeBatch(lats)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    one = max(int(_lib.lib().pk2_wordlat_oracle_workspace_bytes(batch._h, n, 1, _lib.ptr(off[n:n + 2]))) for n in range(35))
    mb = 2.5 * one / (1 << 20)
    assert len(batch._oracle_chunks(off, mb)) >= 3 and len(batch._oracle_chunks(off, 4096)) == 1
    assert batch.oracle(refs, workspace_mb=mb) == whole and batch.oracle(refs) == whole
    for n, P in enumerate(lats):
        assert score.WordLatticeBatch([P]).oracle([refs[n]])[0] == whole[n]


def test_refusals():
    P = score.pack_lattice(R.random_lattice(8, 4, 5, seed=0))
    batch = score.WordLatticeBatch([P, P], names=["utt7", "utt8"])
    with pytest.raises(ValueError, match="lattice utt8: reference word 0"):
        batch.oracle([[1, 2], [3, 0]])
    with pytest.raises(ValueError, match="2 lattices"):
        batch.oracle([[1]])
    # the C ABI (host arrays stand for the device pointers: nothing may touch them)
    L = _lib.lib()
    i = np.zeros(256, np.int32)
    ip = _lib.ptr(i)
    off = np.asarray([0, 3, 8], np.int64)
    need = int(L.pk2_wordlat_oracle_workspace_bytes(batch._h, 0, 2, _lib.ptr(off)))
    assert need >= 4 * (P.S * 4 + P.S * 6) and need % 8 == 0
    assert L.pk2_wordlat_oracle_workspace_bytes(batch._h, 0, 3, _lib.ptr(off)) == 0
    assert L.pk2_wordlat_oracle_workspace_bytes(batch._h, 0, 2, _lib.ptr(np.asarray([0, 3, 2], np.int64))) == 0
    assert L.pk2_wordlat_oracle_workspace_bytes(batch._h, 0, 2, None) == 0

    def call(first=0, count=2, ref_off=off, work_bytes=need, ws=P.depth, ps=P.depth, label=ip, errors=ip, work=ip):
        return L.pk2_wordlat_oracle(batch._h, first, count, label, ip, ip, _lib.ptr(ref_off), work, work_bytes, errors, ip, ip, ws,
                                    ip, ip, ps, ip, ip, None)
    assert call(label=None) == -1 and b"null" in L.pk2_last_error()
    assert call(errors=None) == -1 and call(work=None) == -1 and b"null" in L.pk2_last_error()
    assert call(first=1, count=2) == -1 and call(first=-1) == -1 and call(count=0) == -1 and b"lattices" in L.pk2_last_error()
    assert call(ref_off=np.asarray([0, 3, 2], np.int64)) == -1 and b"ref_off" in L.pk2_last_error()
    assert call(ref_off=np.asarray([-1, 3, 8], np.int64)) == -1 and b"ref_off" in L.pk2_last_error()
    assert call(ws=P.depth - 1) == -1 and b"word_stride" in L.pk2_last_error()
    assert call(ps=P.depth - 1) == -1 and b"path_stride" in L.pk2_last_error()
    assert call(work_bytes=need - 8) == -1 and b"workspace" in L.pk2_last_error()
    assert not i.any()


def test_decoder_lattices_and_the_command_line_end_to_end(tmp_path):
    """Two synthetic utterances through the recogniser and the determiniser, written as an archive; bin/score.py -oracle in a
    fresh process against the Python call and the restatement on the lattices read back."""
    Pn = 60
    g = synth.decoding_graph_arcs(40, Pn, seed=4, max_phones=3)
    tm = synth.transition_model_arrays(Pn)
    rec = lattice.MappedLatticeFasterRecognizer(lattice.TransitionModel.from_arrays(tm), g, 0.2,
                                                lattice.LatticeFasterDecoderOptions(beam=10.0, lattice_beam=4.0))
    rng = np.random.default_rng(3)
    lens = [40, 31]
    ll = np.zeros((2, max(lens), Pn), np.float32)
    for n, T in enumerate(lens):
        ll[n, :T] = 2.0 * rng.standard_normal((T, Pn))
    lat = rec.decode_batch(torch.from_numpy(ll).cuda(), lens)
    dets = [lat.compact_lattice(n, determinize=True) for n in range(2)]
    with kaldi_io.CompactLatticeWriter("ark:" + str(tmp_path / "lat.ark")) as w:
        for n, d in enumerate(dets):
            w["synth-%d" % n] = d
    read = dict(kaldi_io.read_compact_lattice_ark(str(tmp_path / "lat.ark")))
    packed = [score.pack_lattice(read["synth-%d" % n]) for n in range(2)]
    vocab = sorted({int(x) for P in packed for x in P.word_ids[1:]})
    assert len(vocab) >= 2
    unk = vocab[0]
    sym = {0: "<eps>", **{v: ("<UNK>" if v == unk else "W%d" % v) for v in vocab}}
    (tmp_path / "words.txt").write_text("".join("%s %d\n" % (s, i) for i, s in sym.items()))
    # references: the best path with one word replaced by a word outside words.txt, one by <UNK>, and one more appended
    batch = score.WordLatticeBatch(packed)
    refs = []
    for n in range(2):
        words = [sym[x] for x in batch.best_path([(1.0, 0.1, 0.0)])[n][0][0]]
        refs.append((words[:1] + ["OUTSIDE"] + words[2:] + ["<UNK>", "W%d" % vocab[-1]]))
    (tmp_path / "text").write_text("".join("synth-%d %s\n" % (n, " ".join(r)) for n, r in enumerate(refs)) + "synth-9 W1 W2\n")

    def run(out, flags):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "score.py"), "-lat_file", str(tmp_path / "lat.ark"),
                            "-words_txt", str(tmp_path / "words.txt"), "-ref_text", str(tmp_path / "text"), "-out_dir",
                            str(tmp_path / out), "-min_lmwt", "9", "-max_lmwt", "10", "-word_ins_penalty", "0.0"] + flags,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout.strip().splitlines()
    plain, withor = run("plain", []), run("oracle", ["-oracle"])
    assert withor[-1] == plain[-1] and withor[-1].startswith("best: ") and withor[:-2] + withor[-1:] == plain
    for name in os.listdir(tmp_path / "plain"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "oracle" / name).read_bytes()
    assert sorted(os.listdir(tmp_path / "oracle")) == sorted(os.listdir(tmp_path / "plain") + ["oracle.txt", "result_oracle"])
    # the Python call with the ids the command line gives: words.txt's, fresh ones above them for the others
    ids = {s: i for i, s in sym.items()}
    ids["OUTSIDE"] = max(sym) + 1
    id_refs = [[ids[x] for x in r] for r in refs]
    recs = batch.oracle(id_refs, skip_words=(unk,))
    tot = {f: sum(r[f] for r in recs) for f in ("errors", "ins", "dele", "sub")}
    tot["errors"] += 2; tot["dele"] += 2                      # synth-9 has no lattice
    ref_words = sum(len(r) for r in refs) + 2
    af = [score.lattice_depth(P) for P in packed]
    assert [a[1] for a in af] == lens
    m = re.fullmatch(r"oracle: errors=(\d+) ref_words=(\d+) WER=([\d.]+)% ins=(\d+) del=(\d+) sub=(\d+) depth=([\d.]+)", withor[-2])
    assert m, withor[-2]
    assert [int(m.group(k)) for k in (1, 2, 4, 5, 6)] == [tot["errors"], ref_words, tot["ins"], tot["dele"], tot["sub"]]
    assert m.group(3) == "%.2f" % (100.0 * tot["errors"] / ref_words)
    assert m.group(7) == "%.2f" % (sum(a[0] for a in af) / sum(lens))
    lines = (tmp_path / "oracle" / "result_oracle").read_text().splitlines()
    hyp = (tmp_path / "oracle" / "oracle.txt").read_text().splitlines()
    for n, (P, r) in enumerate(zip(packed, recs)):
        want = O.oracle(P, id_refs[n], (unk,))
        assert all(r[f] == want[f] for f in FIELDS) and unk not in r["words"] and r["errors"] >= 2
        key, words = "synth-%d" % n, " ".join(sym[x] for x in r["words"])
        assert hyp[n] == (key + " " + words).rstrip()
        assert lines[4 * n:4 * n + 4] == [("reco: %s %s" % (key, words)), "ref: %s %s" % (key, " ".join(refs[n])),
                                          "%s err: %d ref_len: %d" % (key, r["errors"], len(refs[n])),
                                          "%s ins: %d del: %d sub: %d" % (key, r["ins"], r["dele"], r["sub"])]
