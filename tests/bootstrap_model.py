"""A numpy model of the bootstrap contract (include/elimrec_hip.h, elimrec_bootstrap_means): Philox4x32-10 on uint64 arrays, the
drawn positions of a (seed, replicate, group) and the replicate means with float64 sums -- math.fsum with exact=True, for the tests
that claim a bound against the exactly rounded sum."""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
DOMAIN = 0x626F6F74          # counter word 3: "boot"


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11). counter: four arrays (or scalars) of 32-bit words, key: two 32-bit integers ->
    uint64 [..., 4] holding the four 32-bit output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(*counter))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                        # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1)


def positions(seed, r, g, n_g):
    """The n_g drawn positions of replicate r of group g, each in [0, n_g): int64 [n_g]."""
    if n_g == 0:
        return np.zeros(0, dtype=np.int64)
    calls = np.arange((n_g + 3) // 4, dtype=np.uint64)
    words = philox4x32((calls, r, g, DOMAIN), (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n_g]
    return ((words * np.uint64(n_g)) >> np.uint64(32)).astype(np.int64)


def means(rows, ptr, group_rows, R, seed, rows_b=None, exact=False):
    """float64 [R x G x C]: the replicate means of the contract. Values in float64 -- rows_b - rows with rows_b -- summed with
    np.sum (pairwise) or, exact=True, math.fsum (the exactly rounded sum); NaN for an empty group."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32
    val = rows.astype(np.float64)
    if rows_b is not None:
        assert np.asarray(rows_b).dtype == np.float32
        with np.errstate(invalid="ignore"):
            val = np.asarray(rows_b).astype(np.float64) - val
    ptr, group_rows = np.asarray(ptr, dtype=np.int64), np.asarray(group_rows, dtype=np.int64)
    G, C = ptr.size - 1, val.shape[1]
    out = np.full((R, G, C), np.nan)
    for g in range(G):
        listed = group_rows[ptr[g]:ptr[g + 1]]
        if not listed.size:
            continue
        for r in range(R):
            drawn = val[listed[positions(seed, r, g, listed.size)]]
            if exact:
                finite = np.isfinite(drawn).all(axis=0)
                with np.errstate(invalid="ignore"):
                    plain = drawn.sum(axis=0)
                out[r, g] = [math.fsum(drawn[:, c]) if finite[c] else plain[c] for c in range(C)]
            else:
                with np.errstate(invalid="ignore"):
                    out[r, g] = drawn.sum(axis=0)
            out[r, g] /= listed.size
    return out
