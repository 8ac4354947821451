"""The graphs of the dense-form device tests of the co-interaction neighbours (tests/test_cooccur_dense_gpu.py), shared with the
host test that shows they do what they claim (tests/test_cooccur_cpu.py). Each builder returns a Case: the other side's lists
(user -> items, IN THE ORDER GIVEN -- the dense form's running list depends on the arrival order), n_query and the query rows.
Every size comes from ops.COOCCUR_SLOTS and ops.COOCCUR_GROUPS."""
import collections

import numpy as np

import cooccur_model as cm

# csrc/cooccur.hip: COOCCUR_CAP = COOCCUR_SLOTS / 2, CO_THREADS and CO_STEP have no accessor. A quarter wave (16 of a wave's 64 lanes)
# shares one user, so CO_THREADS / 16 users are in flight and a user gives 16 * CO_STEP entries to a step.
CO_THREADS, CO_STEP, QUARTER = 256, 4, 16
USERS_PER_PASS, ENTRIES_PER_STEP = CO_THREADS // QUARTER, QUARTER * CO_STEP
SORT_SIZES = (63, 64, 65, 128, 129, 1024, 1025)

Case = collections.namedtuple("Case", "users n_query rows")


def slots():
    from elimrec_amd import ops
    return int(ops.COOCCUR_SLOTS)


def groups():
    from elimrec_amd import ops
    return int(ops.COOCCUR_GROUPS)


def cap():
    return slots() // 2


def cut_limit():
    """The list is sorted and cut once it is longer than this (COOCCUR_CAP - CO_THREADS * CO_STEP)."""
    return cap() - CO_THREADS * CO_STEP


def csrs(case):
    """(q_ptr, q_nbr, o_ptr, o_nbr) of a case."""
    o_ptr, o_nbr = cm.csr_of(case.users)
    return cm.transpose_csr(o_ptr, o_nbr, case.n_query) + (o_ptr, o_nbr)


def walk_of_rows(case):
    q_ptr, q_nbr, _, _ = csrs(case)
    return cm.walk(q_ptr, q_nbr, len(case.users))[np.asarray(case.rows, dtype=np.int64)]


def many_rows():
    """2 G + 76 items, each held by 4 hub users that hold all of them (every W >= 4 n > SLOTS / 2: every row is dense whatever
    `lds` says, and its n - 1 candidates cross the cut limit once), each hub in an order of its own, and 300 users of degree 3 so
    that counts, degrees and lists differ from row to row. Queried: every item in a shuffled order, five of them twice."""
    rng = np.random.default_rng(21)
    n = 2 * groups() + 76
    users = [rng.permutation(n).tolist() for _ in range(4)]
    users += [rng.choice(n, size=3, replace=False).tolist() for _ in range(300)]
    rows = rng.permutation(n).tolist()
    for at in (3, 400, 2 * groups() + 1, 77, n):
        rows.insert(at, rows[(at * 7 + 11) % n])
    return Case(users, n, rows)


def _hubs(rng, n_dense, pool):
    """Items 0 .. n_dense - 1 with 5 users each; a user holds its item and ceil(SLOTS / 10) + 40 + 9 d others drawn from the pool
    [n_dense, n_dense + pool), so W(d) is past SLOTS / 2 and most pool items have one or two such users (the LDS form)."""
    users = []
    for d in range(n_dense):
        deg = -(-slots() // 10) + 40 + 9 * d
        for _ in range(5):
            held = (n_dense + rng.choice(pool, size=deg - 1, replace=False)).tolist()
            held.insert(int(rng.integers(0, deg)), d)
            users.append(held)
    users += [(n_dense + rng.choice(pool, size=3, replace=False)).tolist() for _ in range(200)]
    return users


def _cheap_rows(users, n_query, n_dense, count, rng):
    """`count` rows of the LDS form with at least one neighbour, in a shuffled order."""
    o_ptr, o_nbr = cm.csr_of(users)
    q_ptr, q_nbr = cm.transpose_csr(o_ptr, o_nbr, n_query)
    walk = cm.walk(q_ptr, q_nbr, len(users))
    cheap = np.flatnonzero((walk > 1) & (walk <= cap()))
    cheap = cheap[cheap >= n_dense]
    return rng.permutation(cheap)[:count].tolist()


def interleaved():
    """Dense rows at positions 0, 3 and 6 of 8, LDS rows between them: with lds=True the dense form runs G = 3 workgroups, the three
    dense positions are congruent mod 3, so workgroup 0 serves all three on one counter row, and workgroups 1 and 2, whose
    positions are all LDS rows, serve none. The dense rows' candidate sets overlap (random draws from one pool)."""
    rng = np.random.default_rng(22)
    pool = 3 * cap()
    users = _hubs(rng, 3, pool)
    n = 3 + pool + 2                                         # the last two items have no user
    lds = _cheap_rows(users, n, 3, 5, rng)
    rows = [0, lds[0], lds[1], 1, lds[2], lds[3], 2, lds[4]]
    return Case(users, n, rows)


def second_pass():
    """Q = CO_THREADS + 44 rows with one dense row at position CO_THREADS + 14: with lds=True G = 1, and the one workgroup meets
    its row in the second pass of its `base` loop, after skipping CO_THREADS LDS rows in the first. The rest are LDS rows, twelve
    of them items nobody holds (fillers)."""
    rng = np.random.default_rng(23)
    pool = 3 * cap()
    users = _hubs(rng, 1, pool)
    n = 1 + pool + 12
    Q, at = CO_THREADS + 44, CO_THREADS + 14
    rows = _cheap_rows(users, n, 1, Q - 13, rng) + list(range(1 + pool, n))
    rows = rng.permutation(rows).tolist()
    rows.insert(at, 0)
    return Case(users, n, rows)


def _blocks(extra, ids, n_blocks=5):
    """Query item 0 with n_blocks x USERS_PER_PASS users in segment order; user k holds ENTRIES_PER_STEP fresh items and then item 0
    (so one step of pass 2 meets a whole block's USERS_PER_PASS x ENTRIES_PER_STEP candidates, and the step after it only item 0):
    every c = 1. ids: the fresh items' ids in arrival order (block, user, place). extra[t]: how many further users, outside item
    0's segment, hold all of block t's items -- deg(j) = 1 + extra[t]."""
    per = USERS_PER_PASS * ENTRIES_PER_STEP
    assert len(ids) == n_blocks * per and len(extra) == n_blocks
    users = []
    for k in range(n_blocks * USERS_PER_PASS):
        users.append(list(ids[k * ENTRIES_PER_STEP:(k + 1) * ENTRIES_PER_STEP]) + [0])
    for level in range(max(extra)):
        users.append([j for t in range(n_blocks) if extra[t] > level for j in ids[t * per:(t + 1) * per]])
    return Case(users, 1 + len(ids), [0])


def block_of(case, n_blocks=5):
    """item id -> the block of `_blocks` that holds it (item 0: -1)"""
    per = USERS_PER_PASS * ENTRIES_PER_STEP
    where = np.full(case.n_query, -1, dtype=np.int64)
    for k in range(n_blocks * USERS_PER_PASS):
        where[case.users[k][:-1]] = k * ENTRIES_PER_STEP // per
    return where


def _shuffled_ids(seed, n_blocks=5):
    return (1 + np.random.default_rng(seed).permutation(n_blocks * USERS_PER_PASS * ENTRIES_PER_STEP)).tolist()


def rising(n_blocks=5):
    """deg(j) falls from n_blocks to 1 along the blocks: under cosine and jaccard every block outranks all blocks before it, so
    every candidate enters and every cut raises the threshold. Ids are shuffled: within a block the id decides."""
    return _blocks([n_blocks - 1 - t for t in range(n_blocks)], _shuffled_ids(24, n_blocks), n_blocks)


def falling(n_blocks=5):
    """deg(j) rises from 1 to n_blocks: after the first cut (at the end of block 1, the threshold being 0 until then) no candidate may
    enter."""
    return _blocks(list(range(n_blocks)), _shuffled_ids(25, n_blocks), n_blocks)


def flat_desc(n_blocks=5):
    """No further users: under "count" every score is 1. Ids descend along the arrival order, so every later candidate outranks
    every kept one by ~id in the key's low word alone."""
    n = n_blocks * USERS_PER_PASS * ENTRIES_PER_STEP
    return _blocks([0] * n_blocks, list(range(n, 0, -1)), n_blocks)


def flat_asc(n_blocks=5):
    """As flat_desc with ascending ids: after the first cut none may enter."""
    n = n_blocks * USERS_PER_PASS * ENTRIES_PER_STEP
    return _blocks([0] * n_blocks, list(range(1, n + 1)), n_blocks)


WRAP_HOMES = (-4, -3, -2, -1, 0, 1)                          # home slots, relative to the table's end


def wrap():
    """A catalogue of 8 x SLOTS items. Item 100's first user holds it and the 48 items id = slot + SLOTS k, k < 8, whose home slots
    are the table's last four and its first two: 32 keys start in the last four slots, so probing runs past the end and on over
    slots 0, 1 and their own keys. A second user holds item 100 and every third of them: counts 1 and 2, W = 49 + 17."""
    S = slots()
    many = [(h % S) + S * k for h in WRAP_HOMES for k in range(8)]
    many = np.random.default_rng(26).permutation(many).tolist()
    return Case([[100] + many, many[::3] + [100]], 8 * S, [100])


def full_list():
    """One user holds item 7 and COOCCUR_CAP - 1 other items of a catalogue of 3 x SLOTS: W = COOCCUR_CAP, the largest the LDS
    form takes, and the list's largest size. 400 users of degree 3 outside item 7's segment vary deg(j)."""
    rng = np.random.default_rng(27)
    n = 3 * slots()
    others = (8 + rng.choice(n - 8, size=cap() - 1, replace=False)).tolist()
    held = others[:900] + [7] + others[900:]
    users = [held] + [rng.choice(others, size=3, replace=False).tolist() for _ in range(400)]
    return Case(users, n, [7])


def sort_sizes():
    """Items 0 .. 6 with exactly SORT_SIZES candidates each -- one below, at and one past the network's smallest size, the next
    power of two and one past it, half the list and one past it (a network over the whole list). Item r's first user holds it and
    its n fresh items, a second user it and every third of them (counts 1 and 2); 300 users of degree 3 over the fresh items vary
    deg(j). W(r) = n + 1 + ceil(n / 3) + 1 <= COOCCUR_CAP."""
    rng = np.random.default_rng(28)
    total = sum(SORT_SIZES)
    ids = (len(SORT_SIZES) + rng.permutation(total)).tolist()
    users, at = [], 0
    for r, n in enumerate(SORT_SIZES):
        fresh = ids[at:at + n]
        at += n
        users += [fresh[:n // 2] + [r] + fresh[n // 2:], [r] + fresh[::3]]
    users += [rng.choice(ids, size=3, replace=False).tolist() for _ in range(300)]
    return Case(users, len(SORT_SIZES) + total, [5, 0, 6, 1, 2, 3, 4])


BUILDERS = dict(many_rows=many_rows, interleaved=interleaved, second_pass=second_pass, rising=rising, falling=falling,
                flat_desc=flat_desc, flat_asc=flat_asc, wrap=wrap, full_list=full_list, sort_sizes=sort_sizes)
_BUILT = {}


def case(name):
    """The case, built once per process."""
    if name not in _BUILT:
        _BUILT[name] = BUILDERS[name]()
    return _BUILT[name]
