"""MBR system combination on the device (pykaldi2_amd.score.CombinedBatch, csrc/lattice_combine.hip)
against the float64 restatement tests/combine_ref.py (combine: the rule; test_combine_host.py holds it against MBR decoding
of the explicit union lattice) on identical packed lattices.  Every device buffer of the calls is NaN / sentinel poisoned and
surrounded by checked guard elements (score._DEBUG_GUARD).

Tolerances are those of DESIGN.md 7.13, derived there: risk, confidences and bin posteriors are sums of at most
K A (Q + 1) <= 1e5 products with a few 2^-53 relative error each on values <= Q: 1e-9 absolute.  Words, iterations, status
and the starting system must be equal wherever the restatement's margins make them well defined (test_gpu_score's
conditions); every fixed case asserts those conditions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combine_ref as CR  # noqa: E402
import mbr_ref as R  # noqa: E402
from pykaldi2_amd import score  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = list(range(15)) + [23]          # seed 15 with SETTINGS[1] has a tie margin of 3.4e-13 and is left out by the issue
MAX_ERR = {}
_CASES, _REF = {}, {}


@pytest.fixture(autouse=True)
def poisoned_buffers():
    score._DEBUG_GUARD = True
    yield
    score._DEBUG_GUARD = False


def packed_case(seed):
    if seed not in _CASES:
        lats, w = CR.case(seed)
        _CASES[seed] = ([score.pack_lattice(lat) for lat in lats], [float(x) for x in w])
    return _CASES[seed]


def ref(Ps, weights, st, **kw):
    key = (tuple(id(P) for P in Ps), tuple(weights), tuple(st[:3]), tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = (Ps, CR.combine(Ps, weights, st, **kw))
    return _REF[key][1]


def conditions_hold(o):
    m = o["margins"]
    return m["sum"] <= 1e-12 and m["tie"] >= 1e-12 and m["argmax"] >= 1e-6 and m["best_path"] >= 1e-9


def chain(words):
    return R.paths_lattice([(list(words), 1.0)])


def note(name, value):
    MAX_ERR[name] = max(MAX_ERR.get(name, 0.0), float(value))


def check(rec, want, bins=0, tol=1e-9):
    assert rec["words"] == want["words"] and rec["iterations"] == want["iterations"] and rec["status"] == want["status"]
    assert rec["system"] == want["system"]
    assert abs(rec["risk"] - want["risk"]) <= tol
    note("risk", abs(rec["risk"] - want["risk"]))
    if len(want["words"]):
        assert np.abs(rec["conf"] - want["conf"]).max() <= tol
        note("conf", np.abs(rec["conf"] - want["conf"]).max())
    if bins:
        assert len(rec["bins"]) == len(want["bins"])
        for got, exp in zip(rec["bins"], want["bins"]):
            assert [w for w, _ in got] == [w for w, _ in exp]
            assert max(abs(a[1] - b[1]) for a, b in zip(got, exp)) <= tol
            note("bins", max(abs(a[1] - b[1]) for a, b in zip(got, exp)))


def run_group(Ps, weights, settings=R.SETTINGS, bins=2, **kw):
    """One group through the device and the restatement; the restatement's conditions are asserted, not used as a filter."""
    recs = score.CombinedBatch([[P] for P in Ps], weights=weights).mbr(settings, bins=bins, **kw)[0]
    for st, rec in zip(settings, recs):
        want = ref(Ps, weights, st, bins=bins, **kw)
        assert conditions_hold(want), want["margins"]
        check(rec, want, bins)
    return recs


# ---- 1. generator cases ----
@pytest.mark.parametrize("seed", SEEDS)
def test_generator_cases_against_the_restatement(seed):
    Ps, w = packed_case(seed)
    run_group(Ps, w)
    print("seed %d: %d systems of depth %s; largest errors so far: %s" % (seed, len(Ps), [P.depth for P in Ps], MAX_ERR))


def test_the_generator_cases_cover_every_shape():
    depths = {P.depth for s in SEEDS for P in packed_case(s)[0]}
    assert {s % 8 for s in SEEDS} == set(range(8)) and min(depths) <= 3 and max(depths) >= 70


# ---- 2. hand-made lattices ----
def test_hand_made_lattices():
    a, b, c, x, y = 1, 2, 3, 7, 8
    S1 = score.pack_lattice(R.paths_lattice([([a, b], 0.6), ([a, c], 0.4)]))
    S2 = score.pack_lattice(R.paths_lattice([([x, y], 0.4), ([a, b], 0.35), ([a, c], 0.25)]))
    st = [(1.0, 1.0, 0.0)]
    r = score.combine([[S1], [S2]], st)[0][0]
    assert r["words"] == [a, b] and r["iterations"] == 1 and r["status"] == 0 and r["system"] == 0
    assert abs(r["risk"] - 0.725) <= 1e-6 and np.abs(r["conf"] - [0.8, 0.475]).max() <= 1e-6
    cb = score.CombinedBatch([[S1], [S2]], weights=(0.1, 0.9))
    r = cb.mbr(st)[0][0]
    assert r["words"] == [a, b] and r["iterations"] == 2 and r["status"] == 0 and r["system"] == 1
    assert abs(r["risk"] - 0.985) <= 1e-6 and np.abs(r["conf"] - [0.64, 0.375]).max() <= 1e-6
    words, cost, system = cb.best_path(st)[0][0]
    assert words == [x, y] and system == 1 and abs(cost + np.log(0.4)) <= 1e-6
    # max_iter = 1 where two E-steps are needed: not converged, the first hypothesis with its own statistics
    one = cb.mbr(st, max_iter=1)[0][0]
    want = CR.combine([S1, S2], (0.1, 0.9), st[0], max_iter=1)
    assert one["status"] == 1 and one["iterations"] == 1 and one["words"] == [x, y] == want["words"] and one["system"] == 1
    assert abs(one["risk"] - want["risk"]) <= 1e-9 and np.abs(one["conf"] - want["conf"]).max() <= 1e-9
    assert np.abs(one["conf"] - 0.36).max() <= 1e-6
    # decode_mbr = False with bins: one E-step on the first hypothesis, no update
    conf = cb.mbr(st, decode_mbr=False, bins=3)[0][0]
    want = CR.combine([S1, S2], (0.1, 0.9), st[0], decode_mbr=False, bins=3)
    assert conf["status"] == 0 and conf["iterations"] == 1 and conf["words"] == [x, y]
    check(conf, want, bins=3)


# ---- 3. a group of one system is pk2_wordlat_mbr of that lattice, bit for bit ----
def _same(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra["words"] == rb["words"] and ra["iterations"] == rb["iterations"] and ra["status"] == rb["status"]
        assert ra["risk"] == rb["risk"] and np.array_equal(ra["conf"], rb["conf"]) and ra.get("bins") == rb.get("bins")


def test_one_system_gives_the_bits_of_wordlat_mbr():
    lats = [R.random_lattice(*shape, seed=0) for shape in ((3, 2, 3), (8, 4, 5), (20, 8, 8), (33, 5, 4), (70, 6, 5))]
    lats += [chain(range(1, n + 1)) for n in (15, 16, 31, 32)]
    Ps = [score.pack_lattice(lat) for lat in lats]
    single = score.WordLatticeBatch(Ps).mbr(R.SETTINGS, bins=2)
    comb = score.CombinedBatch([Ps]).mbr(R.SETTINGS, bins=2)
    for a, b in zip(comb, single):
        _same(a, b)
        assert all(r["system"] == 0 for r in a)
    assert [2 * len(row[0]["words"]) + 2 for row in comb[-4:]] == [32, 34, 64, 66]


# ---- 4. kernel edges ----
def test_two_lane_chunks_and_the_lane_group_switch():
    for n, positions in ((32, 66), (7, 16), (8, 18)):
        s1, s2 = chain(range(1, n + 1)), chain(list(range(1, n)) + [40])
        Ps = [score.pack_lattice(s1), score.pack_lattice(s2)]
        recs = run_group(Ps, [0.6, 0.4], settings=R.SETTINGS[:1])
        assert recs[0]["words"] == list(range(1, n + 1)) and 2 * len(recs[0]["words"]) + 2 == positions
        assert abs(recs[0]["risk"] - 0.4) <= 1e-9 and abs(recs[0]["conf"][-1] - 0.6) <= 1e-9


def test_depth_3_and_depth_40_in_one_group():
    Ps = [score.pack_lattice(R.random_lattice(3, 2, 3, seed=0)), score.pack_lattice(R.random_lattice(40, 12, 10, seed=0))]
    assert [P.depth for P in Ps] == [4, 41]        # the arcs into the end state are a level of their own
    for w in ([0.5, 0.5], [0.999, 0.001]):
        run_group(Ps, w)


def test_disjoint_vocabularies():
    S1 = score.pack_lattice(R.paths_lattice([([1, 2, 3], 0.7), ([1, 3], 0.3)]))
    S2 = score.pack_lattice(R.paths_lattice([([11, 12], 0.55), ([13], 0.45)]))
    recs = run_group([S1, S2], [0.45, 0.55], settings=[(1.0, 1.0, 0.0)], bins=4)
    assert set(recs[0]["words"]) <= {1, 2, 3, 11, 12, 13}


def test_a_system_missing_for_one_utterance():
    P0, w0 = packed_case(2)
    P1, _ = packed_case(3)
    sysA, sysB = [P0[0], P1[0]], [P0[1], None]
    cb = score.CombinedBatch([sysA, sysB], weights=[w0[0], w0[1]])
    res = cb.mbr(R.SETTINGS, bins=2)
    alone = score.WordLatticeBatch([P1[0]]).mbr(R.SETTINGS, bins=2)[0]
    for g, st in enumerate(R.SETTINGS):
        want = ref([P0[0], P0[1]], [w0[0], w0[1]], st, bins=2)
        assert conditions_hold(want), want["margins"]
        check(res[0][g], want, 2)
    _same(res[1], alone)                              # the weights are renormalised over the one system present
    assert all(r["system"] == 0 for r in res[1])
    sysB2 = [None, P1[1]]                             # the second system alone for the second utterance: its index is 1
    r2 = score.CombinedBatch([[P0[0], None], sysB2]).mbr(R.SETTINGS[:1])
    assert r2[1][0]["system"] == 1 and r2[0][0]["system"] == 0


def test_a_lattice_combined_with_itself():
    for seed in (3, 4, 6):
        P = packed_case(seed)[0][0]
        single = score.WordLatticeBatch([P]).mbr(R.SETTINGS)[0]
        twice = score.CombinedBatch([[P], [P]], weights=[0.3, 0.7]).mbr(R.SETTINGS)[0]
        for a, b in zip(twice, single):
            assert a["words"] == b["words"] and a["iterations"] == b["iterations"] and a["status"] == b["status"]
            assert abs(a["risk"] - b["risk"]) <= 1e-12 and (not len(b["words"]) or np.abs(a["conf"] - b["conf"]).max() <= 1e-12)


# ---- 5. the same bits ----
def _same_c(a, b):
    _same(a, b)
    assert [r["system"] for r in a] == [r["system"] for r in b]


def test_runs_batches_and_launch_splits_give_the_same_bits():
    groups = [packed_case(s) for s in (2, 3, 4, 8, 10, 11)]
    K = 3
    systems = [[Ps[k] if k < len(Ps) else None for Ps, _ in groups] for k in range(K)]
    cb = score.CombinedBatch(systems, weights=[0.5, 0.3, 0.2])
    whole, again = cb.mbr(R.SETTINGS, bins=2), cb.mbr(R.SETTINGS, bins=2)
    for u, (Ps, _) in enumerate(groups):
        _same_c(whole[u], again[u])
        alone = score.CombinedBatch([[P] for P in Ps], weights=[0.5, 0.3, 0.2][:len(Ps)])
        _same_c(whole[u], alone.mbr(R.SETTINGS, bins=2)[0])
    G = len(R.SETTINGS)
    size = score._lib.lib().pk2_wordlat_combine_workspace_bytes
    sizes = [int(size(cb.batch._h, u, 1, G, 2)) for u in range(6)]
    assert min(sizes) > 0
    # six equal groups of two systems under a budget that holds two of them: three launches
    A, B = groups[1][0][:2]
    same6 = score.CombinedBatch([[A] * 6, [B] * 6], weights=[0.5, 0.5])
    one = int(size(same6.batch._h, 0, 1, G, 0))
    mb = 2.3 * one / (1 << 20)
    assert len(same6._chunks(G, 0, mb)) == 3 and len(same6._chunks(G, 0, 4096)) == 1
    for ra, rb in zip(same6.mbr(R.SETTINGS), same6.mbr(R.SETTINGS, workspace_mb=mb)):
        _same_c(ra, rb)
    with pytest.raises(ValueError, match="workspace_mb"):
        same6.mbr(R.SETTINGS, workspace_mb=0.0001)


# ---- 6. scale ----
def test_12_groups_of_3_systems_times_33_settings_in_one_call():
    rng = np.random.default_rng(7)
    groups = [[score.pack_lattice(R.random_lattice(3, 2, 3, seed=100 * u + k)) for k in range(3)] for u in range(12)]
    weights = [float(x) for x in rng.random(3) + 0.2]
    settings = score.sweep()
    cb = score.CombinedBatch([[g[k] for g in groups] for k in range(3)], weights=weights)
    res = cb.mbr(settings)
    assert len(res) == 12 and all(len(row) == 33 for row in res) and len(cb._chunks(33, 0, 4096)) == 1
    left_out = 0
    for Ps, row in zip(groups, res):
        for st, rec in zip(settings, row):
            want = CR.combine(Ps, weights, st)
            if conditions_hold(want):
                assert rec["words"] == want["words"] and rec["status"] == want["status"] and rec["system"] == want["system"]
                assert abs(rec["risk"] - want["risk"]) <= 1e-9
            else:
                left_out += 1
    print("pairs left out by the conditions: %d of %d" % (left_out, 12 * 33))
    assert left_out <= 0.02 * 12 * 33


# ---- 7. refusals ----
def test_refusals():
    P = score.pack_lattice(chain([1, 2]))
    for systems, kw in (([], {}), ([[P]] * 9, {}), ([[P], [P]], dict(weights=[1.0])), ([[P], [P]], dict(weights=[1.0, 2.0, 3.0])),
                        ([[P], [P]], dict(weights=[1.0, 0.0])), ([[P], [P]], dict(weights=[1.0, -2.0])),
                        ([[P], [P]], dict(weights=[1.0, float("inf")])), ([[P], [P]], dict(weights=[1.0, float("nan")])),
                        ([[P, None], [P, None]], {}), ([[P, P], [P]], {})):
        with pytest.raises(ValueError):
            score.CombinedBatch(systems, **kw)
    cb = score.CombinedBatch([[P], [P]])
    with pytest.raises(ValueError, match="times"):
        cb.mbr(R.SETTINGS, times=True)
    for kw in (dict(max_iter=0), dict(max_iter=1.5), dict(bins=9), dict(bins=-1), dict(max_iter=score.COMBINE_MAX_ITER + 1)):
        with pytest.raises(ValueError):
            cb.mbr(R.SETTINGS, **kw)
    with pytest.raises(ValueError):
        cb.mbr([(1.0, float("inf"), 0.0)])
    with pytest.raises(ValueError):
        score.combine([[P]], R.SETTINGS, weights=[0.0])


def test_the_abi_refuses_invalid_groups():
    """pk2_wordlat_set_groups / pk2_wordlat_combine validate every index on the host: PK2_ERR_INVALID, nothing launched."""
    P = score.pack_lattice(chain([1, 2]))
    Q = score.pack_lattice(chain([2, 5]))
    batch = score.WordLatticeBatch([P, Q])
    L, ptr = score._lib.lib(), score._lib.ptr
    good = score.pack_groups([[P, Q]], [[1.0, 3.0]])

    def set_groups(**over):
        H = dict(good, **over)
        return L.pk2_wordlat_set_groups(batch._h, len(H["group_off"]) - 1, ptr(H["group_off"]), ptr(H["wn"]), ptr(H["log_wn"]),
                                        ptr(H["uvoc_off"]), ptr(H["uvoc"]), ptr(H["map"]))

    assert L.pk2_wordlat_combine_workspace_bytes(batch._h, 0, 1, 3, 0) == 0        # no groups yet
    bad_map = good["map"].copy(); bad_map[1] = 7
    swapped = good["map"].copy(); swapped[[1, 2]] = swapped[[2, 1]]
    for over in (dict(group_off=np.asarray([0, 1], np.int32)), dict(wn=np.asarray([0.25, 0.5])),
                 dict(wn=np.asarray([0.0, 1.0])), dict(log_wn=np.asarray([0.0, 0.0])),
                 dict(uvoc=np.asarray([0, 2, 1, 5], np.int32)), dict(uvoc=np.asarray([1, 2, 3, 5], np.int32)),
                 dict(map=bad_map), dict(map=swapped), dict(map=np.full(8, -1, np.int32))):
        assert set_groups(**over) != 0
    assert set_groups() == 0
    assert L.pk2_wordlat_combine_workspace_bytes(batch._h, 0, 2, 3, 0) == 0        # one group only
    assert L.pk2_wordlat_combine_workspace_bytes(batch._h, 0, 1, 65, 0) == 0
    assert L.pk2_wordlat_combine_workspace_bytes(batch._h, 0, 1, 3, 0) > 0
