"""The named cases of the neighbour-vote tests, shared by tests/test_vote_cpu.py (conditions on the inputs) and
tests/test_vote_gpu.py (the kernel against tests/vote_model.py). A case: neighbour lists idx int32 / val fp32 [n x Kn], one history
per segment, one list of further left-out ids per segment (or None), and the segments a call names."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name idx val hist excl users")

SLOTS, CAP, GROUPS = 2048, 1024, 512         # csrc/vote.hip's VOTE_SLOTS, VOTE_SLOTS / 2, VOTE_GROUPS (the CPU tests check them)
POSITIONS, SLOTS_PER_STEP = 16, 32           # history positions in flight, slots of each per capacity check (16 lanes x VOTE_STEP)
KS = (1, 64, 256)


def _random_lists(rng, n, Kn):
    idx = rng.integers(0, n, size=(n, Kn)).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, size=(n, Kn)).astype(np.float32)
    return idx, val


def basics():
    """n = 70, Kn = 3. Histories of length 0, 1 and about 10, a repeated history id, history ids outside the table; list entries
    that are -1, past n and -inf; an item voted for and left out, a user whose every candidate is left out."""
    rng = np.random.default_rng(11)
    n, Kn = 70, 3
    idx, val = _random_lists(rng, n, Kn)
    idx[3] = [-1, 5, 70]
    idx[4] = [2 ** 31 - 1, 6, 6]                                             # a repeated id within a list votes twice
    val[5] = [-np.inf, 0.5, np.inf]
    val[6, 1] = np.nan
    idx[7], val[7] = [-1, -1, -1], [-np.inf] * 3                             # a filler row
    hist = [[], [3], [4], [5, 6, 7], list(rng.integers(0, n, size=10)), [8, 8, 9, 8], [70, -1, 12, 2 ** 31 - 1, -2 ** 31, 13],
            list(rng.integers(0, n, size=11)), [20, 21], [20, 21], [7], [300]]
    excl = [[] for _ in hist]
    excl[1] = [5]                                                            # voted for (by item 3's list) and left out
    excl[8] = [int(i) for i in np.concatenate([idx[20], idx[21]])]           # every candidate left out
    excl[9] = [int(idx[20, 0]), -4, 70, int(idx[20, 0])]                     # ids outside the table, a repeat
    excl[4] = list(range(0, 70, 2))
    return Case("basics", idx, val, hist, excl, list(range(len(hist))))


def fixed_point():
    """Values 2^-25 (rounds to 0: listed with cnt 1 and score 0), 3 * 2^-25 (a tie, to the even 2), 1/3, negatives; two votes that
    cancel to exactly 0 (cnt 2); sums 2^34 + 2 (id 41) and 2^34 + 1 (id 40) round to one fp32 score and are ordered by id."""
    n, Kn = 70, 3
    idx = np.full((n, Kn), -1, dtype=np.int32)
    val = np.full((n, Kn), -np.inf, dtype=np.float32)
    idx[0], val[0] = [30, 31, 32], [2.0 ** -25, 3 * 2.0 ** -25, 1.0 / 3.0]
    idx[1], val[1] = [33, 34, 35], [-0.25, -1.0 / 3.0, 0.75]
    idx[2], val[2] = [35, 36, 32], [-0.75, -2.0 ** -25, 1.0 / 3.0]
    idx[3], val[3] = [40, 41, 37], [1024.0, 1024.0, 5 * 2.0 ** -25]
    idx[4], val[4] = [40, 41, 38], [2.0 ** -24, 2.0 ** -23, -3 * 2.0 ** -25]
    hist = [[0, 1, 2, 3, 4], [0], [1, 2], [3, 4], [4, 3, 2, 1, 0]]
    return Case("fixed_point", idx, val, hist, None, list(range(len(hist))))


def hash_chain():
    """n a little over 2 x SLOTS; the voted ids 5, 5 + SLOTS, 5 + 2 SLOTS share a home slot, 6 and 6 + SLOTS the next, and the
    left-out ids 6 and 5 + SLOTS sit in the same probe chain; ids at the table's end wrap around."""
    n, Kn = 2 * SLOTS + 70, 3
    rng = np.random.default_rng(5)
    idx, val = _random_lists(rng, n, Kn)
    idx[0] = [5, 5 + SLOTS, 5 + 2 * SLOTS]
    idx[1] = [6, 6 + SLOTS, 5]
    idx[2] = [SLOTS - 1, 2 * SLOTS - 1, 7]
    idx[3] = [0, SLOTS, 2 * SLOTS]
    hist = [[0, 1], [0, 1, 2, 3], [2, 3, 2]]
    excl = [[6, 5 + SLOTS], [2 * SLOTS - 1, 6], []]
    return Case("hash_chain", idx, val, hist, excl, [0, 1, 2])


def at_the_cap():
    """Kn = 3 and a history of 256 entries: V = 256 x 3 + 256 = CAP without a further left-out id (the LDS form) and CAP + 1 with
    one (the dense form); a short user between them."""
    rng = np.random.default_rng(3)
    n, Kn = 70, 3
    idx, val = _random_lists(rng, n, Kn)
    long = [int(i) for i in rng.integers(0, 40, size=CAP // (Kn + 1))]
    hist = [long, [1, 2], long, long[::-1]]
    excl = [[], [], [69], [69]]
    return Case("at_the_cap", idx, val, hist, excl, [0, 1, 2, 3])


def dense_rows():
    """Seven users with short histories over shared lists: with lds=False and a grid of 2 workgroups each workgroup serves three
    or four of them on one workspace row, so an entry one user leaves dirty is met by the next."""
    rng = np.random.default_rng(9)
    n, Kn = 70, 3
    idx, val = _random_lists(rng, n, Kn)
    idx[:, 0] = 50                                                           # every list votes for item 50
    hist = [list(rng.integers(0, 30, size=m)) for m in (4, 9, 1, 6, 0, 12, 3)]
    excl = [[50] if u % 3 == 0 else [] for u in range(len(hist))]            # ... and some users leave it out
    return Case("dense_rows", idx, val, hist, excl, list(range(len(hist))))


CUT_N, CUT_KN, CUT_H = 1664, 128, 12


def _cut(name, value_of_slot):
    """A history of 12 items whose lists of 128 hold 1536 distinct ids: more than the selection list's CAP. The 12 positions are in
    flight together and a step covers 32 slots of each, so candidates arrive by slot."""
    idx = np.full((CUT_N, CUT_KN), -1, dtype=np.int32)
    val = np.full((CUT_N, CUT_KN), -np.inf, dtype=np.float32)
    for j in range(CUT_H):
        idx[j] = 64 + j * CUT_KN + np.arange(CUT_KN)
        val[j] = [value_of_slot(s, j) for s in range(CUT_KN)]
    return Case(name, idx, val, [list(range(CUT_H)), [0, 1]], None, [0, 1])


def cut_rising():
    return _cut("cut_rising", lambda s, j: 0.001 * (s + 1) + 0.0001 * j)


def cut_falling():
    return _cut("cut_falling", lambda s, j: 1.0 - 0.001 * s - 0.0001 * j)


def cut_flat():
    return _cut("cut_flat", lambda s, j: 0.5)


BUILDERS = collections.OrderedDict((f.__name__, f) for f in (basics, fixed_point, hash_chain, at_the_cap, dense_rows, cut_rising,
                                                             cut_falling, cut_flat))
_BUILT = {}


def case(name):
    if name not in _BUILT:
        _BUILT[name] = BUILDERS[name]()
    return _BUILT[name]
