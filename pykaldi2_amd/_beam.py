"""What the beam searches of ctc.py and transducer.py share on the host."""
import numpy as np
import torch


def limit(value, hi, name, who):
    """value as an int if it is a whole number in 1..hi (and no bool), ValueError "<who>: <name> ... outside 1..hi" otherwise."""
    if isinstance(value, bool) or int(value) != value or not 1 <= value <= hi:
        raise ValueError("%s: %s %r outside 1..%d" % (who, name, value, hi))
    return int(value)


def nbest_lists(tokens, lens, scores, nbest):
    """The tensors of a beam_search_raw in ONE copy to the host: per utterance a list of at most nbest (token list, score)."""
    N, B, T = tokens.shape
    flat = torch.cat([tokens.reshape(N, -1).double(), lens.double(), scores], dim=1).cpu().numpy()      # (int32 is exact in float64)
    tok, ln, sc = flat[:, :B * T].reshape(N, B, T).astype(np.int64), flat[:, B * T:B * T + B].astype(np.int64), flat[:, B * T + B:]
    return [[(tok[n, r, :ln[n, r]].tolist(), float(sc[n, r])) for r in range(min(nbest, B)) if ln[n, r] >= 0] for n in range(N)]
