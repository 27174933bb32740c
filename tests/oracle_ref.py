"""Plain int64 restatement of the lattice oracle (pykaldi2_amd/csrc/lattice_oracle.hip) on the packed
lattice of pykaldi2_amd.score.pack_lattice: the smallest edit distance between a reference and any path of the lattice
(Kaldi's lattice-oracle), the path that reaches it under one fixed tie rule, and an enumeration of all paths for small
lattices.  This file is the authority for the tie rule; the kernel follows it.

    lab[a]  0 for an epsilon arc or an arc whose word is skipped (free), otherwise the word's local id
    ref[j]  local ids, -1 for a word the lattice does not contain (it never matches)

    D[0][j] = j
    C[n][j] = min over the incoming arcs a = (s -> n) of
                lab[a] == 0:  D[s][j]
                lab[a] != 0:  min(D[s][j] + 1, D[s][j-1] + (lab[a] != ref[j-1]))      (insertion; match / substitution)
    D[n][j] = min over k <= j of C[n][k] + (j - k)                                     (deletions)
    errors  = D[S-1][R]
"""
import numpy as np

INF = 0x3FFFFFFF


def labels(P, skip_words=()):
    """lab of every packed arc: the local word id, 0 for epsilon and for the GLOBAL word ids in skip_words."""
    skip = np.isin(P.word_ids, np.asarray(list(skip_words), np.int64))
    return np.where(skip[P.word], 0, P.word).astype(np.int64)


def local_ref(P, ref):
    """Global word ids -> the lattice's local ids, -1 for a word the lattice does not contain."""
    ref = np.asarray(ref, np.int64).reshape(-1)
    k = np.minimum(np.searchsorted(P.word_ids, ref), P.W - 1)
    return np.where(P.word_ids[k] == ref, k, -1).astype(np.int64)


def table(P, lab, ref):
    """D, int64 (S, R + 1)."""
    ref = np.asarray(ref, np.int64).reshape(-1)
    R = ref.size
    j = np.arange(R + 1)
    D = np.zeros((P.S, R + 1), np.int64)
    D[0] = j
    for n in range(1, P.S):
        C = np.full(R + 1, INF, np.int64)
        for a in range(P.in_off[n], P.in_off[n + 1]):
            row = D[P.src[a]]
            if lab[a] == 0:
                cand = row
            else:
                cand = row + 1
                cand[1:] = np.minimum(cand[1:], row[:-1] + (ref != lab[a]))
            C = np.minimum(C, cand)
        D[n] = np.minimum.accumulate(C - j) + j
    return D


def backtrace(P, lab, ref, D):
    """The oracle path from (S-1, R) back to (0, 0): at (n, j) the incoming arcs of n in ascending packed index, for each
    first the diagonal (lab != 0, j >= 1, D[s][j-1] + (lab != ref[j-1]) == D[n][j]), then the free step (lab == 0,
    D[s][j] == D[n][j]), then the insertion (lab != 0, D[s][j] + 1 == D[n][j]); the first arc that fits is taken; if none
    fits the step is a deletion to (n, j-1).  Returns dict(errors, ins, dele, sub, arcs (packed), words (local ids))."""
    ref = np.asarray(ref, np.int64).reshape(-1)
    n, j = P.S - 1, ref.size
    arcs, words, ins, dele, sub = [], [], 0, 0, 0
    while (n, j) != (0, 0):
        cur, step = int(D[n, j]), None
        for a in range(P.in_off[n], P.in_off[n + 1]):
            s, l = int(P.src[a]), int(lab[a])
            if l != 0 and j >= 1 and D[s, j - 1] + (l != ref[j - 1]) == cur:
                step = (a, s, j - 1)
                sub += int(l != ref[j - 1])
            elif l == 0 and D[s, j] == cur:
                step = (a, s, j)
            elif l != 0 and D[s, j] + 1 == cur:
                step = (a, s, j)
                ins += 1
            if step is not None:
                break
        if step is None:
            assert j >= 1 and D[n, j - 1] + 1 == cur, (n, j)
            dele += 1
            j -= 1
            continue
        arcs.append(step[0])
        if lab[step[0]] != 0:
            words.append(int(lab[step[0]]))
        n, j = step[1], step[2]
    arcs.reverse()
    words.reverse()
    return dict(errors=int(D[P.S - 1, ref.size]), ins=ins, dele=dele, sub=sub, arcs=arcs, words=words)


def oracle(P, ref, skip_words=()):
    """The record of WordLatticeBatch.oracle for one lattice and a reference of GLOBAL word ids: errors, ins, dele, sub,
    words (global ids), arcs (indices into the input lattice's arcs; the arcs packing made of the finals left out) and
    packed_arcs."""
    lab, r = labels(P, skip_words), local_ref(P, ref)
    out = backtrace(P, lab, r, table(P, lab, r))
    out["packed_arcs"] = out.pop("arcs")
    # the arcs into the end state are exactly those packing made of the final weights
    out["arcs"] = [int(P.orig_arc[a]) for a in out["packed_arcs"] if P.dst[a] != P.S - 1]
    out["words"] = [int(P.word_ids[w]) for w in out["words"]]
    return out


def paths(P, lab):
    """Every start -> end path as (packed arcs, labels != 0 in path order); small lattices only."""
    out = []

    def walk(n, arcs):
        if n == P.S - 1:
            out.append((list(arcs), [int(lab[a]) for a in arcs if lab[a] != 0]))
            return
        for k in range(P.out_off[n], P.out_off[n + 1]):
            a = int(P.out_idx[k])
            arcs.append(a)
            walk(int(P.dst[a]), arcs)
            arcs.pop()
    walk(0, [])
    return out
