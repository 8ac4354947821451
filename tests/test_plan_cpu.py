"""tests/plan_model.py against hand-written cases and plain Python loops, and the condition that gives test_plan_gpu.py its power: on
the rows of plan_cases.rows(), every member list of three or more slots of every GPU case sums to other float32 bits when it is
reversed or rotated. No GPU, no project imports."""
import numpy as np
import pytest

import plan_cases as pc
import plan_model as pm


def test_plan_by_hand():
    #       slot  0  1  2  3  4  5  6
    keys = [5, 2, 5, 40, 2, 5, 0]
    p = pm.plan(keys, 5, 41, pad_key=-100)
    assert p.active.tolist() == [0, 2, 5, 40] and p.active.dtype == np.int32
    assert p.seg_info.tolist() == [4, 2, 0, 2, 2, 4, 0, 4] and p.seg_info.dtype == np.int32
    assert p.slot_seg.tolist() == [2, 1, 2, 3, 1, 2, 0]
    assert p.members.tolist() == [6, 1, 4, 0, 2, 5, 3] and p.seg_start.tolist() == [0, 1, 3, 6, 7]
    assert p.bitmap.tolist() == [0b100101, 1 << 8] and p.bitmap.dtype == np.uint32
    assert p.active_rows.tolist() == [0, 2, 5, 40, -96, -95, -94]
    assert pm.plan(keys, 5, 41).active_rows is None and pm.plan(keys, 5, 0).bitmap is None


@pytest.mark.parametrize("split,n_lo", [(-3, 0), (0, 0), (1, 1), (2, 1), (3, 2), (5, 2), (6, 3), (32, 3), (40, 3), (41, 4), (64, 4),
                                        (1000, 4)])
def test_n_lo_rules(split, n_lo):
    """split_key <= 0 gives 0, >= key_space gives n_act, an absent key counts the keys below it -- with and without a key space
    (the radix-sort form: finalize_segments_kernel's two rules, restated here as a loop over the sorted keys)."""
    keys = np.array([5, 2, 5, 40, 2, 5, 0])
    for key_space in (41, 64, 0):
        info = pm.plan(keys, split, key_space).seg_info.tolist()
        assert info == [4, n_lo, 0, n_lo, n_lo, 4, 0, 4], (key_space, info)
    ks = np.sort(keys)
    segid = np.cumsum(np.concatenate([[1], ks[1:] != ks[:-1]]))
    got = None
    for i in range(len(ks)):
        if i == 0 and ks[0] >= split:
            got = 0
        if ks[i] < split and (i == len(ks) - 1 or ks[i + 1] >= split):
            got = segid[i]
    assert got == n_lo


def test_batch_keys_by_hand():
    U, I = 10, 20
    keys, err = pm.batch_keys([3, 9], [0, 19], [7, 7], U, I)
    assert keys.tolist() == [3, 10, 17, 9, 29, 17] and keys.dtype == np.int32 and err == 0
    keys, err = pm.batch_keys([10, 9], [0, 19], [7, 7], U, I)         # exactly the limit
    assert keys.tolist() == [0, 10, 17, 9, 29, 17] and err == 1
    for bad in (-1, 2 ** 40, 2 ** 40 + 5, 2 ** 63 - 1, -2 ** 63):
        k, e = pm.batch_keys([bad, 9], [0, 19], [7, 7], U, I)
        assert k.tolist() == [0, 10, 17, 9, 29, 17] and e == 1, bad
        k, e = pm.batch_keys([3, 9], [0, bad], [7, 7], U, I)
        assert k.tolist() == [3, 10, 17, 9, 10, 17] and e == 2, bad
        k, e = pm.batch_keys([3, 9], [0, 19], [bad, 7], U, I)
        assert k.tolist() == [3, 10, 10, 9, 29, 17] and e == 4, bad
    k, e = pm.batch_keys([3, 9], [20, 19], [7, 20], U, I)              # exactly the limit
    assert k.tolist() == [3, 10, 17, 9, 29, 10] and e == 6
    k, e = pm.batch_keys([-1, 10], [20, -5], [2 ** 40, 7], U, I)
    assert k.tolist() == [0, 10, 10, 0, 10, 17] and e == 7


def test_segment_sums_by_hand_and_against_a_loop():
    big, one = np.float32(2 ** 24), np.float32(1)
    rows = np.array([[big, 1], [one, 2], [one, 3], [-big, 4]], dtype=np.float32)
    s = pm.segment_sums_f32(rows, [0, 1, 2, 3, 1, 2, 0, 3], [0, 4, 8])
    assert s.dtype == np.float32 and s.tolist() == [[0.0, 10.0], [2.0, 10.0]]          # 2^24 + 1 rounds back to 2^24 twice
    assert pm.segment_sums_f32(rows, [1, 2, 0, 3], [0, 4], scale=0.5).tolist() == [[1.0, 5.0]]
    assert pm.segment_sums_f32(rows, [2], [0, 0, 1, 1]).tolist() == [[0, 0], [1, 3], [0, 0]]
    case = pc.segment_cases()["wg_tiers"]
    p = pm.plan(case.keys, case.split, case.key_space)
    r = pc.rows(len(case.keys))
    for scale in (None, pc.SCALE):
        got = pm.segment_sums_f32(r, p.members, p.seg_start, scale)
        for s in range(len(p.active)):
            acc = np.zeros(r.shape[1], dtype=np.float32)
            for m in p.members[p.seg_start[s]:p.seg_start[s + 1]]:
                acc = acc + r[m]
            want = acc * np.float32(1.0 if scale is None else scale)
            assert want.dtype == np.float32 and got[s].tobytes() == want.tobytes(), (scale, s)


@pytest.mark.parametrize("name", ["wg_tiers", "wg_ks1", "wg_ks31", "wg_ks32", "wg_ks33", "dev_ks33", "sort_300_big_key_space"])
def test_bitmap_padding_and_lists_against_a_loop(name):
    case = pc.segment_cases()[name]
    keys, n = case.keys.tolist(), len(case.keys)
    p = pm.plan(case.keys, case.split, case.key_space, pad_key=pc.PAD_KEY)
    words = [0] * ((case.key_space + 31) // 32)
    for k in keys:
        words[k // 32] |= 1 << (k % 32)
    assert p.bitmap.tolist() == words and len(words) * 32 >= case.key_space > (len(words) - 1) * 32
    assert all(w >> (case.key_space - 32 * i) == 0 for i, w in enumerate(words) if case.key_space - 32 * i < 32), "bits beyond key_space"
    uniq = sorted(set(keys))
    tail = [pc.PAD_KEY + r for r in range(len(uniq), n)]
    assert p.active_rows.tolist() == uniq + tail and all(t < 0 for t in tail) and len(set(tail)) == len(tail)
    lists = [[j for j in range(n) if keys[j] == k] for k in uniq]
    assert p.members.tolist() == [j for l in lists for j in l]
    assert p.seg_start.tolist() == [0] + np.cumsum([len(l) for l in lists]).tolist()
    assert [uniq[s] for s in p.slot_seg.tolist()] == keys
    assert p.seg_info[1] == sum(k < case.split for k in uniq)


def test_cases_hold_what_they_name():
    c = pc.segment_cases()
    assert pc.WG_MAX_KEY_SPACE == 245472 and pc.BIG_KEY_SPACE == pc.WG_MAX_KEY_SPACE + 32
    lens = lambda name: set(np.unique(c[name].keys, return_counts=True)[1].tolist())
    assert set(pc.WG_TIERS) <= lens("wg_tiers") and len(c["wg_tiers"].keys) <= 8192
    assert set(pc.DEVICE_TIERS) <= lens("dev_tiers") and 9000 <= len(c["dev_tiers"].keys) <= 30000
    assert lens("wg_910x9") == {9} and len(np.unique(c["wg_910x9"].keys)) == 910
    assert lens("wg_8192_one_key") == {8192} and lens("dev_8193_one_key") == {8193}
    assert sum(l > 8192 for l in np.unique(c["dev_two_beyond_lds"].keys, return_counts=True)[1]) == 2
    for name, case in c.items():
        if case.key_space:
            assert case.keys.min() == 0 or len(case.keys) == 1 or "one_key" in name, name
            assert case.keys.max() == case.key_space - 1 or "one_key" in name or name == "wg_n1", name
    assert [(len(c[k].keys), c[k].key_space, c[k].form) for k in ("wg_8192_one_key", "dev_8193_one_key", "dev_7680_big_key_space",
                                                                  "sort_300_big_key_space")] == \
        [(8192, 8200, 0), (8193, 8200, 1), (7680, 245504, 1), (300, 245504, 2)]
    assert pc.expected_form(8192, pc.WG_MAX_KEY_SPACE) == 0 and pc.expected_form(8192, pc.WG_MAX_KEY_SPACE + 1) == 1
    b = pc.batches()
    assert [b[k].form for k in ("wg_B100", "wg_B1", "dev_B2731", "sort_B100", "sort_B1")] == [0, 0, 1, 2, 2]
    for name in b:
        bad = pc.bad_batches(name)
        assert len(bad) == 12 and sorted(set(e for _, _, e in bad)) == [1, 2, 4, 7]
        for label, batch, bits in bad:
            assert pm.batch_keys(batch.users, batch.pos, batch.neg, batch.U, batch.I)[1] == bits, (name, label)


def _reordered(p, how):
    """The member lists of plan p with every list of three or more slots reversed / its first two entries moved to the end."""
    members = p.members.copy()
    for s in np.nonzero(np.diff(p.seg_start) >= 3)[0]:
        b, e = p.seg_start[s], p.seg_start[s + 1]
        members[b:e] = p.members[b:e][::-1] if how == "reversed" else np.concatenate([p.members[b + 2:e], p.members[b:b + 2]])
    return members


@pytest.mark.parametrize("name,keys,ld", pc.sum_cases(), ids=["%s-%d" % (c[0], c[2]) for c in pc.sum_cases()])
def test_member_order_shows_in_the_sums(name, keys, ld):
    """Zero exemptions: every list of >= 3 members of every GPU case gives at least one other bit, scaled or not, when it is summed in
    reversed order or with its first two members last. So a GPU sum equal to the model's bits vouches for the ascending order."""
    p = pm.plan(keys, 0, 0)
    r = pc.rows(len(keys), ld)
    long = np.diff(p.seg_start) >= 3
    for scale in (None, pc.SCALE):
        want = pm.segment_sums_f32(r, p.members, p.seg_start, scale)
        for how in ("reversed", "rotated"):
            other = pm.segment_sums_f32(r, _reordered(p, how), p.seg_start, scale)
            same = (want.view(np.uint32) == other.view(np.uint32)).all(axis=1)
            assert not (same & long).any(), (name, how, scale, np.nonzero(same & long)[0][:10], int(long.sum()))
            assert (same | long).all()                                  # lists of one or two members: the order cannot matter
