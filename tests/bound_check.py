"""The one bound every kernel family with a float64 oracle is held to (tests/lstm_check.py, tests/attention_check.py).
Plain module, no GPU, no pytest.

The bound of tensor X in a case is taken from a correct float32 implementation on that very data, never from the kernels:

    e32(X)   = max |X_float32-oracle - X_float64-oracle|
    floor(X) = 2^-23 * max |X_float64-oracle|
    max |X_result - X_float64-oracle|  <=  FACTOR * max(e32(X), floor(X)),     FACTOR = 4

(4: another summation order of the products and two 1-ulp hardware approximations per nonlinearity where libm is rounded
to half an ulp -- each worth a small factor, none an order of magnitude.)  No element is excluded, and a NaN or an inf
anywhere in a result is a failure whatever the data.

One exception, for the tensors named in `neg_inf` (the log-sum-exp of attention rows with no visible key): where the float64
oracle is -inf the result must be exactly -inf, and those positions leave the maxima of that tensor.
"""
import numpy as np

FACTOR = 4.0


def unit(want, model):
    """(max(e32, floor), e32, floor) of a tensor from its float64 and float32 oracles (finite everywhere)."""
    e32 = float(np.abs(model.astype(np.float64) - want).max()) if want.size else 0.0
    floor = 2.0 ** -23 * (float(np.abs(want).max()) if want.size else 0.0)
    return max(e32, floor), e32, floor


def compare(got, ref64, ref32, tensors, factor=FACTOR, factors=None, neg_inf=()):
    """Holds every tensor of `got` (name -> array) that `tensors` names to the bound above.  Returns (failures, ratios):
    failures is a list of (tensor name, message), empty for a result that passes; ratios[name] = error / max(e32, floor),
    inf for a tensor that is not finite everywhere.  factors: {name: factor} for tensors with a bound of their own."""
    failures, ratios = [], {}
    for name in tensors:
        if name not in got:
            continue
        x = np.asarray(got[name])
        want, model = ref64[name], ref32[name]
        if x.shape != want.shape:
            failures.append((name, "%s: shape %s, expected %s" % (name, x.shape, want.shape)))
            ratios[name] = float("inf")
            continue
        if name in neg_inf:
            hole = np.isneginf(want)
            if not np.array_equal(hole, np.isneginf(model)):
                failures.append((name, "%s: the float32 oracle is -inf at other places than the float64 oracle (%d against %d): "
                                 "the two oracles disagree, whatever the result" % (name, int(np.isneginf(model).sum()), int(hole.sum()))))
                ratios[name] = float("inf")
                continue
            wrong = hole & ~np.isneginf(x)
            if wrong.any():
                at = tuple(int(v) for v in np.argwhere(wrong)[0])
                failures.append((name, "%s: %d elements are not -inf where the float64 oracle is, first at %s"
                                 % (name, int(wrong.sum()), at)))
                ratios[name] = float("inf")
                continue
            x, want, model = (np.where(hole, 0.0, v) for v in (x, want, model))
        bad = ~np.isfinite(x)
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            failures.append((name, "%s: %d of %d elements not finite (unwritten or NaN / inf), first at %s"
                             % (name, int(bad.sum()), x.size, at)))
            ratios[name] = float("inf")
            continue
        u, e32, floor = unit(want, model)
        diff = np.abs(x.astype(np.float64) - want)
        err = float(diff.max()) if diff.size else 0.0
        ratios[name] = err / u if u > 0 else (0.0 if err == 0 else float("inf"))
        f = (factors or {}).get(name, factor)
        if not err <= f * u:
            at = tuple(int(v) for v in np.unravel_index(int(diff.argmax()), diff.shape))
            failures.append((name, "%s: error %.3g at %s (got %.9g, float64 %.9g) > %g * max(e32 %.3g, floor %.3g): ratio %.1f"
                             % (name, err, at, float(x[at]), float(want[at]), f, e32, floor, ratios[name])))
    return failures, ratios
