"""CPU: the numpy restatement of capturable SUN-RGBD inference (tests/sunrgbd_detect_plan_ref.py) pinned to hand-worked tables, to
the very expressions the existing path uses -- frustum.subsampled_counts and the kept rule of SunrgbdInputBuilder.build_device,
np.cumsum and soff[::S] of frustum.sunrgbd_candidates, the keep-list loop of SunrgbdDetector.detect_frames -- and to the reference's
recorded run of tests/golden/frustum_sunrgbd.npz (det_kept, det_index_off, det_sub_box)."""
import functools
import os

import numpy as np

import frustum_sunrgbd_ref as ref
import sunrgbd_detect_plan_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frustum_sunrgbd.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def test_plan_by_hand():
    # thresholds 2 rows, cap 6: box 0 holds 3 rows, box 1 one row (dropped), box 2 seven rows (subsampled), box 3 eight
    cnt = np.asarray([[3, 0], [1, 0], [2, 5], [4, 4]])
    frame, cls = np.asarray([0, 1, 1, 0]), np.asarray([2, 0, 1, 2])
    p = R.plan(cnt, frame, cls, 4, 2, 6, 4, 100, 2, 3)
    assert p["slot_box"].tolist() == [0, 2, 3, 4] and p["n_kept"] == 3 and p["status"] == 0
    assert p["seg_off"].tolist() == [0, 3, 3, 3, 3, 5, 10, 14, 18] and p["off"].tolist() == [0, 3, 10, 100, 18]
    assert p["counts"].tolist() == [3, 7, 8, 0] and p["cnt32"].tolist() == [3, 7, 8, 0]
    assert p["sub_off"].tolist() == [0, 0, 6, 12, 12] and p["sub_start"].tolist() == [0, 0, 6, 0] and p["sub_len"].tolist() == [0, 6, 6, 0]
    assert p["slot_group"].tolist() == [2, 4, 2, 6]                         # frame * 3 + class; the spare group F * C = 6
    assert p["slot_box"].dtype == np.int32 and p["cnt32"].dtype == p["sub_len"].dtype == p["slot_group"].dtype == np.int32
    assert all(p[k].dtype == np.int64 for k in ("seg_off", "off", "counts", "sub_off", "sub_start"))
    # two slots: the third survivor is dropped, holds no rows, and is said
    p = R.plan(cnt, frame, cls, 4, 2, 6, 2, 100, 2, 3)
    assert p["slot_box"].tolist() == [0, 2] and p["status"] == R.ST_MANY and p["seg_off"].tolist() == [0, 3, 3, 3, 3, 5, 10, 10, 10]
    assert p["sub_off"].tolist() == [0, 0, 6]
    # the capacity cuts inside box 2's second segment: its STORED rows (6) no longer exceed the cap -- no subsample
    p = R.plan(cnt, frame, cls, 4, 2, 6, 3, 9, 2, 3)
    assert p["status"] == R.ST_TRUNC and p["seg_off"].tolist() == [0, 3, 3, 3, 3, 5, 9, 9, 9] and p["counts"].tolist() == [3, 6, 0]
    assert p["n_kept"] == 3 and p["off"].tolist() == [0, 3, 9, 9] and not p["sub_len"].any() and p["sub_off"].tolist() == [0] * 4
    assert R.plan(cnt, frame, cls, 4, 2, 6, 3, 18, 2, 3)["status"] == 0     # exactly met
    # n_boxes: 2 live boxes; beyond the table; negative
    assert R.plan(cnt, frame, cls, 2, 2, 6, 3, 100, 2, 3)["slot_box"].tolist() == [0, 4, 4]
    p = R.plan(cnt, frame, cls, 5, 2, 6, 3, 100, 2, 3)
    assert p["status"] == R.ST_RANGE and p["n_kept"] == 3
    p = R.plan(cnt, frame, cls, -1, 2, 6, 3, 100, 2, 3)
    assert p["n_kept"] == 0 and p["status"] == R.ST_RANGE and p["slot_box"].tolist() == [4] * 3 and p["off"].tolist() == [100] * 3 + [0]
    assert p["slot_group"].tolist() == [6] * 3 and not p["seg_off"].any()
    # a frame or a class out of range: ignored and said, but only below n_boxes
    for col, vals in ((frame, (2, -1)), (cls, (3, -1))):
        for v in vals:
            bad = col.copy()
            bad[2] = v
            a = (bad, cls) if col is frame else (frame, bad)
            p = R.plan(cnt, a[0], a[1], 4, 2, 6, 3, 100, 2, 3)
            assert p["slot_box"].tolist() == [0, 3, 4] and p["status"] == R.ST_RANGE
            assert R.plan(cnt, a[0], a[1], 2, 2, 6, 3, 100, 2, 3)["status"] == 0


def test_plan_knife_edges():
    one = lambda c, thr, cap=64: R.plan([[c]], [0], [0], 1, thr, cap, 1, 1000, 1, 1)
    assert one(4, 5)["n_kept"] == 0 and one(5, 5)["n_kept"] == 1            # point_threshold - 1, point_threshold
    assert one(0, 0)["n_kept"] == 0 and one(1, 0)["n_kept"] == 1 and one(1, -3)["n_kept"] == 1     # max(1, threshold)
    assert one(64, 5)["sub_len"].tolist() == [0] and one(65, 5)["sub_len"].tolist() == [64]        # cap, cap + 1
    assert one(65, 5)["sub_off"].tolist() == [0, 64] and one(65, 5)["counts"].tolist() == [65]
    assert one(3, 5, 2)["n_kept"] == 0                                     # min(count, cap) = 2 < 5: a cap below the bar keeps nothing


def test_plan_equals_the_host_paths_expressions():
    from frustum_convnet_amd import frustum
    rs = np.random.RandomState(2)
    for D, S, cap, thr in ((12, 3, 64, 5), (40, 1, 20, 1), (9, 2, 5, 7)):
        cnt = rs.randint(0, 60, (D, S)) * (rs.uniform(size=(D, 1)) < 0.8)
        frame, cls = rs.randint(0, 3, D), rs.randint(0, 10, D)
        counts = cnt.sum(1)
        sub = [np.arange(cap) if n > cap else None for n in counts]         # what draw_frustum_subsample gives, as to length
        rows = frustum.subsampled_counts(counts, sub)
        kept = np.nonzero(rows >= max(1, int(thr)))[0]                      # SunrgbdInputBuilder.build_device
        p = R.plan(cnt, frame, cls, D, thr, cap, D, 1 << 40, 3, 10)
        n = p["n_kept"]
        assert n == len(kept) and p["slot_box"][:n].tolist() == kept.tolist() and (p["slot_box"][n:] == D).all() and p["status"] == 0
        assert np.array_equal(np.minimum(p["counts"][:n], cap), rows[kept])
        assert [i for i in range(n) if p["sub_len"][i]] == [i for i, d in enumerate(kept) if sub[d] is not None]
        only = np.where(np.isin(np.arange(D), kept)[:, None], cnt, 0)       # sunrgbd_candidates' prefix sum, over the kept boxes
        soff = np.concatenate([[0], np.cumsum(only.reshape(-1))])
        assert np.array_equal(p["seg_off"], soff) and np.array_equal(p["off"][:n], soff[::S][kept]) and p["off"][D] == soff[-1]
        assert np.array_equal(p["slot_group"][:n], (frame * 10 + cls)[kept])


def test_plan_on_the_references_recorded_run():
    """The reference's extract_frustum_data_from_rgb_detection run: 7 boxes, 6 kept, 2 subsampled."""
    g = _golden()
    mine = ref.select(g["points"], g["off"], g["K"], g["Rtilt"], g["det_boxes"], g["det_frame"])
    seg, S = 4096, int(-(-np.diff(g["off"]).max() // 4096))
    cnt = np.asarray([[int(((ix // seg) == s).sum()) for s in range(S)] for ix in mine["index"]])
    D, cap = len(g["det_boxes"]), int(g["meta_cap"])
    p = R.plan(cnt, g["det_frame"], np.arange(D) % 10, D, 5, cap, D, 1 << 40, len(g["off"]) - 1, 10)
    n = p["n_kept"]
    assert (D, n) == (7, 6) and p["slot_box"][:n].tolist() == g["det_kept"].tolist() and p["status"] == 0
    assert np.array_equal(np.minimum(p["counts"][:n], cap), np.diff(g["det_index_off"]))
    assert p["slot_box"][:n][p["sub_len"][:n] > 0].tolist() == g["det_sub_box"].tolist() and len(g["det_sub_box"]) == 2
    assert p["sub_off"].tolist()[:n + 1] == np.concatenate([[0], np.cumsum(p["sub_len"][:n])]).tolist()
    six = R.plan(cnt, g["det_frame"], np.arange(D) % 10, D, 5, cap, 6, int(p["off"][D]), len(g["off"]) - 1, 10)
    assert six["status"] == 0 and six["slot_box"].tolist() == g["det_kept"].tolist()


def test_det_rows_by_hand_and_against_the_host_loop():
    dets = np.arange(40, dtype=np.float32).reshape(5, 8)
    keep = np.asarray([[3, 1, -1], [0, -1, -1], [2, 4, 5], [1, 1, 1]])
    det_off, rows, scores, n, st = R.det_rows(keep, [2, 0, 3, -1], dets)
    assert det_off.tolist() == [0, 2, 2, 5, 5] and n == 5 and st == R.ST_OVER
    assert rows.tolist() == [3, 1, 2, 4, 5] + [-1] * 7
    assert scores[:4].tolist() == [31.0, 15.0, 23.0, 39.0] and np.isnan(scores[4:]).all()          # row 5 = num_dets: NaN
    assert R.corners(dets, rows).tolist() == [False] * 4 + [True] * 8
    assert det_off.dtype == rows.dtype == np.int32 and scores.dtype == np.float32
    det_off, rows, scores, n, st = R.det_rows(keep, [9, 3, 1, 0], dets)    # cnt beyond top_k is clamped
    assert det_off.tolist() == [0, 3, 6, 7, 7] and st == 0 and rows[:7].tolist() == [3, 1, -1, 0, -1, -1, 2]
    assert np.isnan(scores[[2, 4, 5]]).all() and not np.isnan(scores[[0, 1, 3, 6]]).any()
    rs = np.random.RandomState(0)
    keep, cnt = rs.randint(0, 50, (7, 6)), rs.randint(0, 7, 7)
    dets = rs.uniform(size=(50, 8)).astype(np.float32)
    det_off, rows, scores, n, st = R.det_rows(keep, cnt, dets)
    want = np.concatenate([keep[g, :cnt[g]] for g in range(7)])             # SunrgbdDetector.detect_frames
    assert np.array_equal(rows[:n], want) and np.array_equal(det_off, np.concatenate([[0], np.cumsum(cnt)]))
    assert np.array_equal(scores[:n], dets[want, 7]) and (rows[n:] == -1).all() and st == 0
