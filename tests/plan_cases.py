"""The key lists, batches and rows shared by test_plan_cpu.py and test_plan_gpu.py.

The GPU tests see the order of a member list only through segment_apply's float32 sums. test_plan_cpu.py licenses that: with rows(),
every segment of three or more members of every case below gives other bits when its list is reversed or rotated, no exemption.

Forms are selected by shape alone; FORM_* are what ops.segment_plan_form must answer (asserted per case on the GPU, and re-derived
from the planner's expressions in test_plan_cpu.py)."""
import collections
import functools

import numpy as np

FORM_WG, FORM_DEVICE, FORM_SORT = 0, 1, 2        # one workgroup, device-wide bitmap, radix sort

# segment_plan_impl takes the one-workgroup form for n <= PLAN_LDS_N = 8192 slots whose dynamic LDS,
#   (2 * ceil(key_space / 32) + 16 + 1024) * 4 + (3 * 8192 + 1) * 4 bytes,
# is at most 160 * 1024: 2 * words <= 40960 - 1040 - 24577 = 15343, words <= 7671, key_space <= 7671 * 32.
PLAN_LDS_N = 8192
WG_MAX_WORDS = (160 * 1024 // 4 - (16 + 1024) - (3 * PLAN_LDS_N + 1)) // 2
WG_MAX_KEY_SPACE = 32 * WG_MAX_WORDS             # 245 472
BIG_KEY_SPACE = 245504                           # one bitmap word beyond it (7672 words)
PAD_KEY = -(1 << 30)                             # what shard.py passes

Case = collections.namedtuple("Case", "keys split key_space form counts")


def expected_form(n, key_space):
    if 0 < key_space <= WG_MAX_KEY_SPACE and n <= PLAN_LDS_N:
        return FORM_WG
    if key_space > 0 and (key_space + 31) // 32 <= n:
        return FORM_DEVICE
    return FORM_SORT


def _scatter(counts, n, key_space, seed):
    """n keys below key_space: key k exactly counts[k] times, every remaining slot a key of its own (the smallest unused ones, so the
    named counts stay exact), the slots then scattered by a fixed permutation."""
    rng = np.random.default_rng(seed)
    named = sum(counts.values())
    assert named <= n and all(0 <= k < key_space for k in counts)
    free = np.setdiff1d(np.arange(key_space), np.fromiter(counts, dtype=np.int64))[:n - named]
    assert len(free) == n - named, "key space too small for the singles"
    keys = np.concatenate([np.repeat(np.fromiter(counts, dtype=np.int64), list(counts.values())), free])
    return keys[rng.permutation(n)].astype(np.int32)


def _case(keys, split, key_space, counts=None):
    keys = np.asarray(keys, dtype=np.int32)
    got = dict(zip(*np.unique(keys, return_counts=True)))
    for k, c in (counts or {}).items():
        assert got[k] == c, (k, c, got.get(k))
    return Case(keys, split, key_space, expected_form(len(keys), key_space), counts or {})


def _spread(sizes, key_space, first_last=True):
    """Distinct keys for member lists of the given sizes: the largest at key 0, the next at key_space - 1, the rest spread in between."""
    sizes = sorted(sizes, reverse=True)
    inner = np.linspace(37, key_space - 40, num=max(len(sizes) - 2, 1)).astype(np.int64)
    keys = [0, key_space - 1] + [int(k) for k in inner]
    assert len(set(keys[:len(sizes)])) == len(sizes)
    return dict(zip(keys, sizes))


WG_TIERS = (1, 2, 3, 8, 9, 64, 65, 512, 513)                     # insertion sort | one wave's rank sort | the workgroup's
DEVICE_TIERS = (1, 8, 9, 63, 64, 65, 128, 129, 4096, 4097, 8192, 8193)   # registers | a wave | bitonic (128 .. 8192 padded) | global


@functools.lru_cache(maxsize=None)
def segment_cases():
    """name -> Case. Keys 0 and key_space - 1 are in every list with a known key space."""
    c = {}
    # ---- one workgroup
    c["wg_tiers"] = _case(_scatter(_spread(WG_TIERS, 5000), 2501, 5000, 1), 77, 5000, _spread(WG_TIERS, 5000))
    # 8192 slots of one key: the workgroup's rank sort over all of LDS; the largest n of this form
    c["wg_8192_one_key"] = _case(np.full(8192, 4711), 4711, 8200, {4711: 8192})
    # 910 keys of 9 members: as many long lists as 8192 slots allow (16 waves walk 57 rounds of them). all_serial, the branch for more
    # than 1023 long lists, cannot be reached in this form: 1024 lists of at least PLAN_LONG + 1 = 9 members are 9216 slots > 8192.
    k910 = np.concatenate([[0, 8199], np.arange(100, 100 + 8 * 908, 8)])
    c["wg_910x9"] = _case(_scatter({int(k): 9 for k in k910}, 8190, 8200, 2), 4096, 8200, {int(k): 9 for k in k910})
    c["wg_n1"] = _case([0], 0, 1)
    for ks in (1, 31, 32, 33):
        rng = np.random.default_rng(ks)
        keys = np.concatenate([[0, ks - 1, ks - 1, 0, 0], rng.integers(0, ks, 36)])
        c["wg_ks%d" % ks] = _case(keys, ks // 2, ks)
    # the largest key space of this form (the LDS bound above), keys at both ends of the bitmap
    rng = np.random.default_rng(3)
    keys = np.concatenate([[0, WG_MAX_KEY_SPACE - 1], rng.integers(0, WG_MAX_KEY_SPACE, 775)])
    keys[2 + rng.permutation(775)[:40]] = WG_MAX_KEY_SPACE - 1
    c["wg_max_key_space"] = _case(keys, 100000, WG_MAX_KEY_SPACE)
    # ---- device-wide bitmap
    c["dev_8193_one_key"] = _case(np.full(8193, 4711), 4712, 8200, {4711: 8193})        # one slot beyond wg_8192_one_key: the top tier
    c["dev_tiers"] = _case(_scatter(_spread(DEVICE_TIERS, 30000), 27001, 30000, 4), 15000, 30000, _spread(DEVICE_TIERS, 30000))
    two = {0: 9000, 19999: 8193, 64: 8192, 7777: 300, 9: 9, 12345: 3}
    c["dev_two_beyond_lds"] = _case(_scatter(two, 26001, 20000, 5), 64, 20000, two)
    rng = np.random.default_rng(6)                                                       # fewer than 8192 slots, bitmap beyond LDS
    keys = np.concatenate([[0, BIG_KEY_SPACE - 1], rng.integers(0, BIG_KEY_SPACE, 7678)])
    keys[2 + rng.permutation(7678)[:70]] = BIG_KEY_SPACE - 1
    c["dev_7680_big_key_space"] = _case(keys, 122752, BIG_KEY_SPACE)
    for ks in (31, 32, 33):
        rng = np.random.default_rng(100 + ks)
        c["dev_ks%d" % ks] = _case(np.concatenate([[0, ks - 1], rng.integers(0, ks, 8198)]), 16, ks)
    # ---- radix sort: a known key space with too few slots for its bitmap, and the device-wide lists with the key space withheld
    rng = np.random.default_rng(7)
    keys = np.concatenate([[0, BIG_KEY_SPACE - 1], rng.integers(0, BIG_KEY_SPACE, 298)])
    keys[2 + rng.permutation(298)[:12]] = 99999
    c["sort_300_big_key_space"] = _case(keys, 99999, BIG_KEY_SPACE)
    c["sort_n1"] = _case([BIG_KEY_SPACE - 1], BIG_KEY_SPACE - 1, BIG_KEY_SPACE)
    for name in ("dev_8193_one_key", "dev_tiers", "dev_two_beyond_lds"):
        c[name.replace("dev_", "sort_")] = _case(c[name].keys, c[name].split, 0)
    for name, case in c.items():
        assert case.form == {"wg": FORM_WG, "dev": FORM_DEVICE, "sort": FORM_SORT}[name.split("_")[0]], name
    return c


def split_keys(case):
    """split_key at 0, at a word boundary, mid-word, at an absent key, at key_space and above it (and below 0)."""
    ks = case.key_space if case.key_space else int(case.keys.max()) + 1
    present = set(case.keys.tolist())
    absent = next(k for k in range(ks // 2, ks + 2) if k not in present)
    return sorted({-5, 0, 32 * (ks // 64), 32 * (ks // 64) + 13, absent, int(case.keys.max()), ks - 1, ks, ks + 1, ks + 1000})


LD = 24         # columns of rows(): six float4 per row. One column tells a reordered list of three apart about every other time
                # (with 8 columns 7 of the 1576 lists of the cases summed to the same bits reversed); 24 leave none, which
                # test_plan_cpu.py asserts


@functools.lru_cache(maxsize=None)
def rows(n, ld=LD, seed=11):
    """float32 [n, ld]: normal values times 2**randint(-12, 12), so that float32 sums depend on their order."""
    rng = np.random.default_rng([seed, n, ld])
    r = (rng.standard_normal((n, ld)) * np.exp2(rng.integers(-12, 13, (n, ld)))).astype(np.float32)
    r.setflags(write=False)
    return r


SCALE = 0.37109375      # an exact float32 that is no power of two


# ---------------------------------------------------------------------------------------------------- batches
Batch = collections.namedtuple("Batch", "users pos neg U I form")


@functools.lru_cache(maxsize=None)
def batches():
    """name -> valid Batch (int64 ids). 3B = 300 and 8193 slots at U + I = 500 reach the one-workgroup and the device-wide form;
    U + I = BIG_KEY_SPACE with 300 slots reaches the sorted front end (no table of that size exists: only ids are read)."""
    out = {}
    for name, (U, I, B) in {"wg_B100": (200, 300, 100), "wg_B1": (200, 300, 1), "dev_B2731": (200, 300, 2731),
                            "sort_B100": (100000, BIG_KEY_SPACE - 100000, 100), "sort_B1": (100000, BIG_KEY_SPACE - 100000, 1)}.items():
        rng = np.random.default_rng(B + U)
        u, p, q = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
        u[0], p[0], q[0] = 0, 0, I - 1                                   # keys 0, U and U + I - 1
        if B > 1:
            u[-1], p[-1] = U - 1, I - 1
        out[name] = Batch(u.astype(np.int64), p.astype(np.int64), q.astype(np.int64), U, I, expected_form(3 * B, U + I))
    return out


BAD_VALUES = {"minus_one": lambda lim: -1, "limit": lambda lim: lim, "two_to_40": lambda lim: (1 << 40) + 5}


def bad_batches(name):
    """[(label, Batch, expected err bits)]: one bad user, one bad positive, one bad negative, each alone and all three together, with
    -1, exactly the limit, and 2^40 + 5 (which narrows to the valid id 5: the comparison must come first)."""
    good = batches()[name]
    B = len(good.users)
    out = []
    for vname, f in BAD_VALUES.items():
        for which in ((0,), (1,), (2,), (0, 1, 2)):
            cols = [good.users.copy(), good.pos.copy(), good.neg.copy()]
            for j in which:
                cols[j][(7 * j + 3) % B] = f(good.U if j == 0 else good.I)
            out.append(("%s-%s" % (vname, "".join("upn"[j] for j in which)), good._replace(users=cols[0], pos=cols[1], neg=cols[2]),
                        sum(1 << j for j in which)))
    return out


# ---------------------------------------------------------------------------------------------------- what the sums are taken over
WIDE_LD = 260       # more than one pass of segment_sum_kernel's 64 lanes over the float4 columns
WIDE_CASES = ("wg_tiers", "dev_ks33")


@functools.lru_cache(maxsize=None)
def sum_cases():
    """[(name, keys, ld)]: every key list whose member order the GPU tests observe through segment_apply, with the row width used."""
    import plan_model as pm
    out = [(name, case.keys, LD) for name, case in segment_cases().items()]
    out += [(name, segment_cases()[name].keys, WIDE_LD) for name in WIDE_CASES]
    out += [("batch_" + name, pm.batch_keys(b.users, b.pos, b.neg, b.U, b.I)[0], LD) for name, b in batches().items()]
    return out
