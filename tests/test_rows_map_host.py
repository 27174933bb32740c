"""Host side of the output layer's row map (no GPU): lstm.row_map_host builds the map the row-mapped products take, and
fbank.row_lengths -- what FbankExtractor.pad_roll_subsample records on its result -- never falls short of the rows a chain
supervision of the same utterance reads."""
import numpy as np
import pytest

from pykaldi2_amd import chain, fbank, synth
from pykaldi2_amd.lstm import row_map_host


@pytest.mark.parametrize("T,B,lengths,want_valid", [
    (7, 3, (7, 3, 1), [0, 1, 2, 3, 4, 6, 7, 9, 12, 15, 18]),
    (5, 3, (5, 5, 5), list(range(15))),
    (7, 3, (2, 1, 1), [0, 1, 2, 3]),
    (4, 2, (0, 3), [1, 3, 5]),
])
def test_row_map_lists_the_first_len_b_steps_of_every_sequence_ascending(T, B, lengths, want_valid):
    perm, mv = row_map_host(lengths, T, B)
    assert perm.dtype == np.int32 and perm.shape == (T * B,)
    assert mv == sum(lengths) == len(want_valid)
    assert perm[:mv].tolist() == want_valid
    assert (np.diff(perm[:mv]) > 0).all() and (np.diff(perm[mv:]) > 0).all()          # both parts ascend
    assert sorted(perm.tolist()) == list(range(T * B))                                 # valid + padded = every row once
    for b, n in enumerate(lengths):                                                    # sequence b: exactly its first n time steps
        assert sorted(r // B for r in perm[:mv] if r % B == b) == list(range(n))


def test_row_map_rejects_bad_lengths():
    for bad in ((8, 1, 1), (7, 3), (-1, 2, 2)):
        with pytest.raises(ValueError):
            row_map_host(bad, 7, 3)


def test_recorded_lengths_follow_shift_and_subsample():
    assert fbank.row_lengths([10, 7, 1], 0, 1) == (10, 7, 1)
    assert fbank.row_lengths([10, 7, 1], 0, 3) == (4, 3, 1)
    assert fbank.row_lengths([10, 7, 1], -2, 3) == (4, 3, 1)       # the supervision's count, not the rolled frames' (3, 2, 0)
    assert fbank.row_lengths([10, 7, 1], 2, 3) == (4, 3, 1)        # frames land at times 2 .. f + 1; capped at T' = 4
    assert fbank.row_lengths([12, 7], 2, 3) == (4, 3)


def test_supervision_frames_never_exceed_the_recorded_lengths():
    """synth.minibatch batches as bench.py draws them, shifts 0, -1, -2 (bench.py: shift = -(epoch % 3), subsample 3): the
    supervision of an utterance of f frames covers ceil(f / 3) rows whatever the shift, while the rolled features fill only
    ceil((f + shift) / 3) -- the recorded length is the larger of the two."""
    P = 120
    tree, tm = synth.chain_model(P, seed=0)
    aligner, sopts = chain.MappedAligner(tm), chain.SupervisionOptions()
    rng = np.random.default_rng(3)
    shorter = 0
    for _ in range(3):
        mb = synth.minibatch(rng, 4, P, ali_model=tm)
        frames = [fbank.num_frames(w.shape[0]) for w, _ in mb]
        sups = [chain.supervision_from_alignment(aligner, tree, tm, sopts, a) for _, a in mb]
        out_t = (max(frames) - 1) // 3 + 1
        for shift in (0, -1, -2):
            rec = fbank.row_lengths(frames, shift, 3)
            for f, s, r in zip(frames, sups, rec):
                assert s.frames_per_sequence <= r <= out_t, (f, shift, s.frames_per_sequence, r)
                shorter += -(-(f + shift) // 3) < s.frames_per_sequence
    assert shorter > 0, "no utterance whose rolled features end before its supervision: the case the rule exists for did not occur"
