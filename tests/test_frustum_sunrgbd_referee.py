"""CPU: the SUN-RGBD frustum extraction's referee (tests/frustum_sunrgbd_ref.py), frustum.perturb_boxes2d_sunrgbd and
frustum.draw_frustum_subsample pinned to the reference's recorded run (tests/golden/frustum_sunrgbd.npz, written by
tests/golden/make_golden_frustum_sunrgbd.py from the reference's own extract_frustum_data and
extract_frustum_data_from_rgb_detection): selected row indices, labels and counts exact; frustum angle and corners within 1e-12
(the bar tests/test_gpu_frustum_label.py holds); the two host draws bit for bit under the fixture's seed when called alone, the
generator's next draw equal."""
import functools
import os

import numpy as np
import pytest

import frustum_sunrgbd_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frustum_sunrgbd.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def _referee(which):
    g = _golden()
    if which == "train":
        return ref.select(g["points"], g["off"], g["K"], g["Rtilt"], g["train_boxes"], g["train_box_frame"],
                          np.repeat(g["gt_box3d"], int(g["meta_augment"]), 0))
    return ref.select(g["points"], g["off"], g["K"], g["Rtilt"], g["det_boxes"], g["det_frame"])


def test_training_records_are_the_referees_selection():
    g, mine = _golden(), _referee("train")
    sub = ref.fixture_sub(g, "train")
    cap = int(g["meta_cap"])
    assert [d for d in range(len(sub)) if sub[d] is not None] == np.nonzero(mine["counts"] > cap)[0].tolist()
    kept, pos = ref.training_kept(mine["pos"], mine["seg"], sub)
    assert np.array_equal(kept, g["train_kept"])
    recs = ref.fixture_records(g, "train")
    assert len(recs) == len(kept)
    for k, (d, index, label) in enumerate(recs):
        full = mine["index"][d]
        pick = slice(None) if sub[d] is None else sub[d]
        assert np.array_equal(index, full[pick]), d                        # indices, in record order
        assert np.array_equal(label, mine["seg"][d][pick]), d              # labels
        assert len(index) == min(mine["counts"][d], cap) and label.sum() == pos[d]
        assert np.array_equal(g["train_box2d"][k], g["train_boxes"][d].astype(np.float32))
    aerr = np.abs(g["train_angle"] - mine["frustum_angle"][kept])
    cerr = np.abs(g["train_box3d"] - mine["corners"][kept])
    print("angle worst abs err %.3e, corners worst abs err %.3e" % (aerr.max(), cerr.max()))
    assert (aerr <= 1e-12).all() and (cerr <= 1e-12).all()
    rep = np.repeat(g["gt_box3d"], int(g["meta_augment"]), 0)
    assert np.array_equal(g["train_heading"], rep[kept, 6]) and np.array_equal(g["train_size"], 2.0 * rep[kept, 3:6])
    # the cases the fixture holds
    few, big, subfew = g["meta_few"], g["meta_big"], g["meta_subfew"]
    assert (mine["pos"][few] < 5).all() and (mine["pos"][few] > 0).all() and not set(few) & set(kept)
    assert (mine["counts"][big] > cap).all() and set(big) <= set(kept)
    assert (mine["pos"][subfew] >= 5).all() and np.array_equal(pos[subfew] < 5, g["meta_subfew_dropped"]) and g["meta_subfew_dropped"].any()
    assert not set(subfew[g["meta_subfew_dropped"]]) & set(kept)
    assert min(e.min() for e in mine["edge"] if len(e)) >= float(g["meta_margin_px"])
    assert min(e.min() for e in mine["face"] if len(e)) >= float(g["meta_margin"])
    assert any((d < 0).any() for d in mine["depth"])                       # rows behind the camera are selected


def test_detection_records_are_the_referees_selection():
    g, mine = _golden(), _referee("det")
    sub = ref.fixture_sub(g, "det")
    cap = int(g["meta_cap"])
    rows = np.minimum(mine["counts"], cap)
    assert np.array_equal(np.nonzero(rows >= 5)[0], g["det_kept"]) and 0 < mine["counts"][int(g["meta_det_tiny"])] < 5
    for k, (d, index, _) in enumerate(ref.fixture_records(g, "det")):
        full = mine["index"][d]
        assert np.array_equal(index, full if sub[d] is None else full[sub[d]]), d
        assert np.array_equal(g["det_box2d"][k], g["det_boxes"][d])         # unrounded (prepare_data.py:357)
    assert (np.abs(g["det_angle"] - mine["frustum_angle"][g["det_kept"]]) <= 1e-12).all()


def test_rows_are_a_swap_and_a_negation_of_the_input():
    g = _golden()
    rows = ref.to_upright_camera(g["points"][:500])
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(bits(rows[:, 0]), bits(g["points"][:500, 0])) and np.array_equal(bits(rows[:, 2]), bits(g["points"][:500, 1]))
    assert np.array_equal(bits(rows[:, 1]) ^ np.uint32(0x80000000), bits(g["points"][:500, 2]))
    assert np.array_equal(bits(rows[:, 3:]), bits(g["points"][:500, 3:]))


def test_perturb_boxes2d_sunrgbd_equals_the_reference_alone():
    from frustum_convnet_amd import frustum
    g = _golden()
    boxes = np.repeat(g["gt_box2d"], int(g["meta_augment"]), 0)
    np.random.seed(int(g["meta_seed"]))
    got = frustum.perturb_boxes2d_sunrgbd(boxes)
    assert got.dtype == np.float64 and np.array_equal(got, g["alone_boxes"])
    assert np.random.random() == float(g["alone_next"])
    rng = np.random.RandomState(int(g["meta_seed"]))
    assert np.array_equal(frustum.perturb_boxes2d_sunrgbd(boxes, rng=rng), g["alone_boxes"]) and rng.random() == float(g["alone_next"])
    # in the reference's interleaved run the boxes are these up to the first subsample draw, and others behind it
    n = int(g["meta_big"][0]) + 1
    assert np.array_equal(g["train_boxes"][:n], got[:n]) and not np.array_equal(g["train_boxes"], got)


def test_draw_frustum_subsample_equals_the_reference_alone():
    """extract_frustum_data_from_rgb_detection draws nothing but its subsamples, detection after detection."""
    from frustum_convnet_amd import frustum
    g, mine = _golden(), _referee("det")
    np.random.seed(int(g["meta_seed"]))
    got = frustum.draw_frustum_subsample(mine["counts"], cap=int(g["meta_cap"]))
    want = ref.fixture_sub(g, "det")
    assert len(got) == len(want) and sum(x is not None for x in want) == 2
    for a, b in zip(got, want):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    assert np.random.random() == float(g["det_next"])
    assert frustum.draw_frustum_subsample([5, 2048, 0]) == [None, None, None]
    assert np.array_equal(frustum.subsampled_counts(mine["counts"], got), np.minimum(mine["counts"], int(g["meta_cap"])))


def test_host_made_subsamples_are_range_checked():
    from frustum_convnet_amd import frustum
    ok = frustum._check_sub("t", [None, np.array([0, 4, 2])], [3, 5])
    assert ok[0] is None and ok[1].dtype == np.int32
    for sub, counts in (([np.array([0, 5])], [5]), ([np.array([-1])], [5]), ([np.array([0.5])], [5]), ([np.zeros((2, 2), np.int64)], [5]),
                        ([np.zeros(0, np.int64)], [5]), ([None], [5, 6])):
        with pytest.raises(ValueError):
            frustum._check_sub("t", sub, counts)
