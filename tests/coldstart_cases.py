"""The cases of ops.rank_values shared by the host test (model against brute force, small sizes) and the GPU test (kernel against the
model, sizes placed at the kernel's edges): score rows of five families, value lists whose lengths meet 0, 1, the per-pass count,
one more and a ragged mix in ONE call, and values that hit every rule -- equal to catalogue scores, duplicated, +-0.0, above and
below every score, -inf / +inf / NaN -- with a skipped column per value that does, does not, or cannot (-1) beat it."""
import numpy as np

FAMILIES = ("normal", "equal", "few", "masked", "zeros")
B = 6


def scores(family, I, rng):
    if family == "normal":
        x = rng.standard_normal((B, I))
    elif family == "equal":
        x = np.full((B, I), 0.25)
    elif family == "few":
        x = rng.integers(0, 3, size=(B, I)) * 0.5 - 0.5
    elif family == "masked":
        x = rng.standard_normal((B, I))
        x[:, rng.permutation(I)[:(I + 2) // 3]] = -np.inf           # a third of the items (at least one), every row
        x[3] = -np.inf                                               # and one row that is entirely masked (row 2 lists no value)
    else:
        x = np.where(rng.integers(0, 2, size=(B, I)) == 1, -0.0, 0.0)
    return x.astype(np.float32)


def lengths(P, shift):
    """Six per-row value counts: 0, 1, P, P + 1 and two ragged ones, rotated by `shift`; the empty row never comes first or last."""
    lens = [1, P, 0, P + 1, 37, 2 * P + 3]
    k = shift % 3
    return lens[:2][::-1 if k == 1 else 1] + [0] + (lens[3:] if k != 2 else lens[3:][::-1])


def values(row, n, rng):
    """n values for one score row: a mix of every kind, the special ones first so that even n = 1 .. 8 meets several over the rows."""
    fin = row[np.isfinite(row)]
    top, low = (float(fin.max()), float(fin.min())) if fin.size else (1.0, -1.0)
    special = [top + 1.0, low - 1.0, 0.0, -0.0, -np.inf, np.nan, np.inf, top, low]
    rng.shuffle(special)
    out = np.empty(n, dtype=np.float32)
    for i in range(n):
        kind = i % 4 if i >= len(special) else -1
        if kind == -1:
            out[i] = special[i]
        elif kind == 0 and fin.size:
            out[i] = fin[rng.integers(0, fin.size)]                  # equal to a catalogue score
        elif kind == 1 and i:
            out[i] = out[rng.integers(0, i)]                         # a duplicate of an earlier value
        elif kind == 2:
            out[i] = rng.standard_normal()
        else:
            out[i] = rng.integers(-2, 3) * 0.5
    return out


def make(family, I, P, rng, shift, with_skip):
    """-> (scores [B x I] float32, ptr int64 [B + 1], vals float32, skip int32 or None)."""
    x = scores(family, I, rng)
    lens = lengths(P, shift)
    lists = [values(x[b], n, rng) for b, n in enumerate(lens)]
    ptr = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    vals = np.concatenate(lists).astype(np.float32)
    skip = None
    if with_skip:
        skip = rng.integers(-1, I, size=vals.size).astype(np.int32)
        skip[::5] = -1
    return x, ptr, vals, skip
