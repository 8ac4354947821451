"""The cases of ops.segment_row_sum shared by the host test (model against a plain loop) and the GPU test (kernel against the
model): tables of three magnitude families, list lengths below, at and beyond one chunk and beyond one round of the four waves in
ONE call, repeated ids, a strided table and a row offset."""
import numpy as np

FAMILIES = ("unit", "spread", "cancel")


def lengths(chunk):
    """Below, at and beyond one chunk; below, at and beyond one round of the four waves; an empty list between listed ones."""
    return [1, chunk - 1, 0, chunk, chunk + 1, 4 * chunk - 1, 4 * chunk, 4 * chunk + 1]


def table(family, n_rows, C, ld, rng):
    """float32 [n_rows x C] as a view of a [n_rows x ld] buffer whose padding columns hold NaN (reading one shows in the sum)."""
    if family == "spread":
        x = rng.choice([-1.0, 1.0], size=(n_rows, C)) * 10.0 ** rng.uniform(-15, 15, size=(n_rows, C))
    else:
        x = rng.standard_normal((n_rows, C))
    buf = np.full((n_rows, ld), np.nan, dtype=np.float32)
    buf[:, :C] = x
    return buf


def lists(family, lens, n_window, rng):
    """(ptr int64, rows int32, weights float32): every list draws ids from the window with repeats (a list longer than the window
    must repeat; short ones repeat their first id once more). 'cancel': entries come in pairs (i, w), (i, -w) placed apart."""
    rows, weights = [], []
    for n in lens:
        ids = rng.integers(0, n_window, size=n)
        if n >= 3:
            ids[n // 2] = ids[0]
        if family == "spread":
            w = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-15, 15, size=n)
        else:
            w = rng.standard_normal(n)
        if family == "cancel" and n >= 2:
            h = n // 2
            ids[h:2 * h] = ids[:h]
            w[h:2 * h] = -w[:h].astype(np.float32)
        rows.append(ids.astype(np.int32))
        weights.append(w.astype(np.float32))
    ptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr, np.concatenate(rows).astype(np.int32), np.concatenate(weights).astype(np.float32)


def make(family, C, chunk, rng, pad=0, row_offset=0, n_window=37):
    """-> (buffer float32 [n_rows x ld] (columns >= C are NaN), ptr, rows, weights)."""
    buf = table(family, row_offset + n_window, C, C + pad, rng)
    ptr, rows, weights = lists(family, lengths(chunk), n_window, rng)
    return buf, ptr, rows, weights
