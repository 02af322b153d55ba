"""CPU: the fp64 referee of the refinement stage's training link (tests/refine_label_ref.py) against the reference's own
random_shift_rotate_box3d, compute_box_3d_obj_array, extract_pc_in_box3d and utils/box_util.box3d_iou, recorded in
tests/golden/refine_label.npz by tests/golden/make_golden_refine_label.py as extract_frustum_det_data chains them.  No product
symbol is used here.  The fixture's finite rows keep meta_margin_pred from every face plane of every jittered enlarged box of
their frame and meta_margin_label from every matched label box; beyond those margins the reference's hull tests and the referee's
closed boxes must agree on EVERY row."""
import functools
import os

import numpy as np

import cascade_ref
import refine_label_ref as rr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_label.npz")
NO_POSITIVE, NO_POINT, TIE, BELOW, NO_LABEL = 5, 6, 2, 1, 3     # the special candidates (make_golden_refine_label.py)


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN))
    nmax = int(np.diff(g["off"]).max())
    for k in ("ref_mask", "ref_label"):
        g[k] = np.unpackbits(g[k], axis=1, count=nmax).astype(bool)
    return g


@functools.lru_cache(maxsize=None)
def referee():
    g = golden()
    return rr.select_labeled(g["points"], g["off"], g["dets"], g["cand_row"], g["cand_frame"], g["ref_gt_idx"], g["gt_box3d"],
                             g["jitter"], float(g["meta_ratio"]), float(g["meta_shift"]))


def test_fixture_is_what_the_issue_describes():
    g = golden()
    assert g["dets"].dtype == np.float32 and g["points"].dtype == np.float32 and g["points"].shape[1] == 4
    n = np.diff(g["off"])
    assert 600 <= n[0] <= 800 and n[1] == 0 and 2 * 4096 < n[2] < 3 * 4096
    assert g["jitter"].shape == (8, 3, 7) and (g["jitter"] >= 0).all() and (g["jitter"] < 1).all()
    assert float(g["meta_margin_pred"]) == 1e-6 and float(g["meta_margin_label"]) == 1e-6 and float(g["meta_iou_margin"]) == 1e-3
    assert (~np.isfinite(g["points"][:, :3])).any(1).sum() == 6
    assert os.path.getsize(GOLDEN) < 200 * 1024


def test_match_equals_the_references_iou_and_keeps_its_margins():
    g = golden()
    thresh, margin = float(g["meta_thresh"]), float(g["meta_iou_margin"])
    idx, best, every = rr.match(g["dets"], g["cand_row"], g["cand_frame"], g["gt_box3d"], g["gt_off"], thresh)
    assert np.array_equal(idx, g["ref_gt_idx"])
    assert idx.tolist() == [0, -1, 2, -1, 4, 5, 6, 4]
    for d, ious in enumerate(every):
        want = g["ref_iou"][d, :len(ious)]
        assert np.isnan(g["ref_iou"][d, len(ious):]).all()
        assert np.abs(ious - want).max(initial=0.0) <= 1e-9, d
        if len(ious):
            top = np.sort(want)[::-1]
            assert abs(top[0] - thresh) >= margin, d                # no decision depends on float32 rounding ...
            if len(top) > 1 and d != TIE:
                assert top[0] - top[1] >= margin, d                 # ... nor on the order of near-equal overlaps
    assert g["ref_iou"][TIE, 2] == g["ref_iou"][TIE, 3]             # the exact tie: the lower row wins
    assert len(every[NO_LABEL]) == 0 and 0 < best[BELOW] < thresh


def test_jitter_chain_is_bit_identical_to_the_reference():
    g = golden()
    prev_differs = 0
    for d in np.nonzero(g["ref_gt_idx"] >= 0)[0]:
        chain = rr.enlarged_chain(g["dets"][g["cand_row"][d]], g["jitter"][d], float(g["meta_ratio"]), float(g["meta_shift"]))
        assert np.array_equal(chain, g["ref_box"][d]), d
        assert (np.abs(chain[:, 6]) <= np.pi).all()
        # the copies chain: copy 1 is NOT the un-jittered box perturbed by draw 1
        alone = rr.enlarged_chain(g["dets"][g["cand_row"][d]], g["jitter"][d][1:2], float(g["meta_ratio"]), float(g["meta_shift"]))
        prev_differs += int(not np.array_equal(alone[0], chain[1]))
    assert prev_differs == 6
    # both branches of the floored modulo occur (ry = 3.1 wraps past +pi, ry = -3.1 past -pi)
    ry4, ry7 = g["dets"][g["cand_row"][4], 6], g["dets"][g["cand_row"][7], 6]
    assert ry4 > 3.0 and ry7 < -3.0 and g["ref_box"][4, :, 6].min() < -3.0 and g["ref_box"][7, :, 6].max() > 3.0


def test_corners_match_at_the_cascade_bar():
    g, mine = golden(), referee()
    for d in np.nonzero(g["ref_gt_idx"] >= 0)[0]:
        j = g["ref_gt_idx"][d]
        for a in range(3):
            u = d * 3 + a
            assert cascade_ref.within(mine["pred_box3d"][u], g["ref_pred_corners"][u], extent=g["ref_box"][d, a, 3:6].max()), u
            assert cascade_ref.within(mine["box3d"][u], g["ref_gt_corners"][j], extent=g["gt_box3d"][j, 3:6].max()), u
            assert np.array_equal(mine["pred_size"][u], g["ref_box"][d, a, 3:6]) and mine["pred_angle"][u] == g["ref_box"][d, a, 6]
            assert mine["heading"][u] == g["gt_box3d"][j, 6] and np.array_equal(mine["size"][u], g["gt_box3d"][j, 3:6])


def test_selected_rows_and_positives_equal_the_hull_tests_on_every_row():
    g, mine = golden(), referee()
    close_p = close_l = 0
    for d in range(8):
        f = g["cand_frame"][d]
        n = int(g["off"][f + 1] - g["off"][f])
        fr = g["points"][int(g["off"][f]):int(g["off"][f + 1]), :3]
        fin = np.isfinite(fr).all(1)
        for a in range(3):
            u = d * 3 + a
            assert np.array_equal(np.nonzero(g["ref_mask"][u, :n])[0], mine["index"][u]), u
            assert np.array_equal(g["ref_label"][u, :n][mine["index"][u]], mine["positive"][u]), u
            assert not g["ref_mask"][u, n:].any() and not (g["ref_label"][u] & ~g["ref_mask"][u]).any()
            if g["ref_gt_idx"][d] >= 0 and fin.any():
                dp = rr.face_distance(fr[fin], g["ref_box"][d, a])
                dl = rr.face_distance(fr[fin], rr.centre_form(g["gt_box3d"][g["ref_gt_idx"][d]]))
                assert dp.min() >= float(g["meta_margin_pred"]) and dl.min() >= float(g["meta_margin_label"]), u
                close_p += int((dp < 1e-4).sum())
                close_l += int((dl < 1e-4).sum())
    assert close_p >= 50 and close_l >= 50            # the margins are tested: rows within 0.1 mm of a face exist in numbers
    assert np.array_equal(mine["pos"] == 0, g["ref_reject"])
    cnt, pos = mine["counts"].reshape(8, 3), mine["pos"].reshape(8, 3)
    assert (cnt[NO_POSITIVE] > 20).all() and (pos[NO_POSITIVE] == 0).all() and (cnt[NO_POINT] == 0).all()
    assert (cnt[[BELOW, NO_LABEL]] == 0).all() and (pos[[0, 2, 4, 7]] > 10).all()
    assert all(len(set((mine["index"][4 * 3 + a] // 4096).tolist())) == 3 for a in range(3))
    # a non-finite row in the middle of a label box is never selected
    bad = np.nonzero(~np.isfinite(g["points"][:, :3]).all(1))[0]
    for i in bad:
        f = int(np.searchsorted(g["off"], i, side="right") - 1)
        assert not g["ref_mask"][:, i - int(g["off"][f])][np.repeat(g["cand_frame"] == f, 3)].any()
