"""CPU: the numpy restatement of the capturable inference front (tests/frustum_detect_plan_ref.py) pinned to hand-worked cases and
to the very expressions the existing path uses -- the skip rule of InputBuilder.build_device, np.cumsum and soff[::S] of
frustum.frustum_candidates.  The seeded tables keep every box off the rule's knife edges (heights and widths a whole pixel or more
from their thresholds); the knife-edge cases have a margin of exactly 0 by construction."""
import numpy as np

import frustum_detect_plan_ref as R


def _table(D=12, S=3, F=4, seed=0):
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 900, (D, S))
    cnt[[1, 6]] = 0                                                         # no row
    x0, y0 = rs.uniform(0, 500, D), rs.uniform(0, 200, D)
    w, h = rs.uniform(20, 200, D), rs.uniform(20, 100, D)
    h[3], w[8] = 3.0, 0.25                                                  # too low, too narrow
    box = np.stack([x0, y0, x0 + w, y0 + h], 1)
    return cnt, box, rs.randint(0, F, D).astype(np.int32)


def _host_rule(cnt, box, hthr=5, pthr=1):
    """InputBuilder.build_device's lines, and frustum_candidates' prefix sum over the kept boxes' counts."""
    counts = cnt.sum(1)
    skip = (box[:, 3] - box[:, 1] < hthr) | (box[:, 2] - box[:, 0] < 1) | (counts < pthr)
    return np.nonzero(~skip & (counts > 0))[0]


def test_plan_by_hand():
    cnt = np.asarray([[3, 0], [0, 0], [2, 5], [4, 4]])
    box = np.asarray([[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 4.0]], dtype=np.float64)
    frame = np.asarray([0, 1, 1, 0])
    slot_box, n, seg_off, off, counts, st = R.plan(cnt, box, frame, 4, 5, 1, 3, 100, 2)
    assert slot_box.tolist() == [0, 2, 4] and n == 2 and st == 0            # box 1: no row; box 3: 4 px high; one empty slot
    assert seg_off.tolist() == [0, 3, 3, 3, 3, 5, 10, 10, 10] and off.tolist() == [0, 3, 100, 10] and counts.tolist() == [3, 7, 0]
    assert slot_box.dtype == np.int32 and seg_off.dtype == off.dtype == counts.dtype == np.int64
    # one slot: the second survivor is dropped and said
    slot_box, n, seg_off, off, counts, st = R.plan(cnt, box, frame, 4, 5, 1, 1, 100, 2)
    assert slot_box.tolist() == [0] and st == R.ST_MANY and seg_off.tolist() == [0, 3, 3, 3, 3, 3, 3, 3, 3] and off.tolist() == [0, 3]
    # the capacity cuts inside box 2's second segment
    slot_box, n, seg_off, off, counts, st = R.plan(cnt, box, frame, 4, 5, 1, 2, 6, 2)
    assert st == R.ST_TRUNC and seg_off.tolist() == [0, 3, 3, 3, 3, 5, 6, 6, 6] and counts.tolist() == [3, 3] and off.tolist() == [0, 3, 6]
    assert R.plan(cnt, box, frame, 4, 5, 1, 2, 10, 2)[5] == 0               # exactly met
    # n_boxes: 2 live boxes; beyond the table; negative
    assert R.plan(cnt, box, frame, 2, 5, 1, 3, 100, 2)[:2][0].tolist() == [0, 4, 4]
    assert R.plan(cnt, box, frame, 5, 5, 1, 3, 100, 2)[5] == R.ST_RANGE and R.plan(cnt, box, frame, 5, 5, 1, 3, 100, 2)[1] == 2
    got = R.plan(cnt, box, frame, -1, 5, 1, 3, 100, 2)
    assert got[1] == 0 and got[5] == R.ST_RANGE and got[0].tolist() == [4, 4, 4] and got[3].tolist() == [100, 100, 100, 0]
    # a frame out of range: ignored and said, but only below n_boxes
    bad = frame.copy()
    bad[2] = 2
    assert R.plan(cnt, box, bad, 4, 5, 1, 3, 100, 2)[0].tolist() == [0, 4, 4] and R.plan(cnt, box, bad, 4, 5, 1, 3, 100, 2)[5] == R.ST_RANGE
    assert R.plan(cnt, box, bad, 2, 5, 1, 3, 100, 2)[5] == 0
    bad[2] = -1
    assert R.plan(cnt, box, bad, 4, 5, 1, 3, 100, 2)[5] == R.ST_RANGE


def test_plan_knife_edges():
    one = lambda h, w, c, hthr=5, pthr=1: R.plan([[c]], [[0.0, 0.0, w, h]], [0], 1, hthr, pthr, 1, 100, 1)[1]
    assert one(5.0, 8.0, 3) == 1 and one(np.nextafter(5.0, 0.0), 8.0, 3) == 0          # h - 0 is h: exactly the threshold; one ulp under
    assert one(8.0, 1.0, 3) == 1 and one(8.0, 0.5, 3) == 0                              # width exactly 1
    assert one(8.0, 8.0, 7, pthr=7) == 1 and one(8.0, 8.0, 6, pthr=7) == 0              # count == lidar_point_threshold
    assert one(8.0, 8.0, 0, pthr=0) == 0                                                # threshold 0 keeps no empty box


def test_plan_equals_the_existing_paths_expressions():
    for seed in range(6):
        cnt, box, frame = _table(seed=seed)
        D, S = cnt.shape
        for hthr, pthr in ((5, 1), (3, 12), (50, 1), (5, 10 ** 6)):
            kept = _host_rule(cnt, box, hthr, pthr)
            slot_box, n, seg_off, off, counts, st = R.plan(cnt, box, frame, D, hthr, pthr, D, 1 << 40, 4)
            assert st == 0 and n == len(kept) and slot_box[:n].tolist() == kept.tolist() and (slot_box[n:] == D).all()
            # frustum_candidates on the kept boxes alone: its cumsum, its soff[::S]
            seg_counts = cnt[kept]
            soff = np.concatenate([[0], np.cumsum(seg_counts.reshape(-1))]).astype(np.int64)
            assert np.array_equal(off[:n], soff[::S][:n]) and off[D] == soff[-1] and np.array_equal(counts[:n], seg_counts.sum(1))
            assert np.array_equal(seg_off[kept * S], soff[::S][:n]) and seg_off[-1] == soff[-1]
            if pthr == 1 and hthr == 5:
                assert 3 not in kept and 8 not in kept and 1 not in kept and n == D - 4
            B1 = max(1, n - 2)
            slot_box, n2, _, off2, counts2, st = R.plan(cnt, box, frame, D, hthr, pthr, B1, 1 << 40, 4)
            assert slot_box[:n2].tolist() == kept[:B1].tolist() and bool(st & R.ST_MANY) == (len(kept) > B1)
            assert np.array_equal(counts2[:n2], cnt[kept[:B1]].sum(1))


def test_fov_plan_and_gathers_by_hand():
    seg_off, fov_off = R.fov_plan([[3, 1], [0, 0], [2, 5]], 1000)
    assert seg_off.tolist() == [0, 3, 4, 4, 4, 6, 11] and fov_off.tolist() == [0, 4, 4, 11] and fov_off.dtype == np.int64
    cnt = np.random.RandomState(1).randint(0, 4096, (5, 3))
    seg_off, fov_off = R.fov_plan(cnt, int(cnt.sum()))
    soff = np.concatenate([[0], np.cumsum(cnt.reshape(-1))]).astype(np.int64)            # frustum_candidates' lines
    assert np.array_equal(seg_off, soff) and np.array_equal(fov_off, soff[::3])
    D, C = 3, 3
    box2d = np.arange(16, dtype=np.float64).reshape(4, 4)
    g = R.gathers([2, 0, 3], box2d, [0.1, 0.2, 0.3, 0.0], [1, 0, 1, 0], [2, 1, 0, 0], [0, 0, 1, 9], [0.5, 0.6, 0.7, 0.0],
                  np.arange(24).reshape(2, 12), C)
    assert g["fangle"].tolist() == [0.3, 0.1, 0.0] and g["box2d"][0].tolist() == [8, 9, 10, 11] and g["slot_frame"].tolist() == [1, 1, 0]
    assert g["P"][:, 0].tolist() == [12, 12, 0] and g["slot_class"].tolist() == [0, 2, 0] and g["slot_group"].tolist() == [1, 0, 9]
    assert g["one_hot"].tolist() == [[1, 0, 0], [0, 0, 1], [1, 0, 0]] and g["rgb_prob"].shape == (3, 1) and g["rgb_prob"].dtype == np.float32
