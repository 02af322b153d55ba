"""No GPU: the generators of tests/inputs_cases.py on their own.  Every case is generated, its knife-edge condition holds (each
margin exactly 0 where the case says so, else > 1e-9, no case left out), the label rows it spells out are the oracle's; plus the
host logic next to the batch-builder kernels: the SUN-RGBD resampling rule and RefineInputBuilder's refusal of a sample without
a window."""
import numpy as np
import pytest

import inputs_cases as ic


@pytest.mark.parametrize("name", list(ic.CASES))
def test_case_generates_off_the_knife_edge(name):
    case = ic.built(name)
    face_min, gap_min, nface, ntie = ic.check_margins(case)
    ic.check_rows(case)
    print("%s: smallest face margin %.3e, smallest fallback gap %.3e, %d exact faces, %d exact ties" %
          (name, face_min, gap_min, nface, ntie))
    want = case["want"]
    B = len(case["rec"]["raw_counts"])
    assert B <= 6 and case["npoints"] <= 2048 and want["point_cloud"].shape == (B, 3, case["npoints"])
    assert max(want["center_ref%d" % (s + 1)].shape[-1] for s in range(len(case["strides"]))) <= 600
    assert set(np.unique(want["cls_label"])) <= {-1, 0, 1} and ((want["cls_label"] == 1).sum(1) >= 1).all()
    assert len(ic.records(case)) == B and len(case["labels"]) == B


def test_spelled_out_rows():
    """The rows the cases are named after, once more in plain sight."""
    fb = ic.built("fallback_last_padded-off")["want"]
    assert fb["cls_label"][1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and fb["cls_label"][2].tolist() == [1] * 8
    assert fb["lens"].tolist() == [[16, 8, 4, 2], [9, 5, 3, 2], [1, 1, 1, 1]]
    on = ic.built("fallback_last_padded-on")["want"]
    assert on["cls_label"][1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and on["cls_label"][2].tolist() == [1] * 8
    for b, n in enumerate((8, 5, 1)):
        alone = ic.built("fallback_last_padded-alone%d" % b)["want"]
        assert alone["cls_label"].shape == (1, n) and alone["lens"][0].tolist() == fb["lens"][b].tolist()
        assert alone["cls_label"][0].tolist() == fb["cls_label"][b, :n].tolist()
    tie = ic.built("exact_tie")["want"]["cls_label"]
    assert [np.nonzero(r)[0].tolist() for r in tie] == [[1], [7], [13]] and tie.shape == (3, 16)
    l2 = ic.built("kitti_long_l2")["want"]["cls_label"]
    assert [np.nonzero(r)[0].tolist() for r in l2] == [[0], [39], [263], [279]] and (l2 >= 0).all() and l2.shape == (4, 280)
    face = ic.built("kitti_face_inclusive")["want"]["cls_label"][0]
    assert face[17:24].tolist() == [0, -1, 1, 1, 1, -1, 0] and np.count_nonzero(face) == 5
    lw = ic.built("long_windows")["want"]
    assert lw["cls_label"].shape == (2, 300) and int(np.argmax(lw["cls_label"][0])) >= 256


def test_forced_coin_of_exactly_one_half_does_not_flip():
    """flip on: the sample with coin 0.5 keeps its x, the one with 0.5000001 is mirrored (against the same batch with flip off)."""
    for shift in (False, True):
        off, on = (ic.built("flip_shift_matrix-f%ds%d" % (f, shift))["want"] for f in (0, 1))
        assert np.array_equal(on["point_cloud"][0], off["point_cloud"][0]) and np.array_equal(on["point_cloud"][2], off["point_cloud"][2])
        assert np.array_equal(on["point_cloud"][1, 0], -off["point_cloud"][1, 0]) and on["box3d_center"][1, 0] == -off["box3d_center"][1, 0]
    for tiny in ("rec", "tiny"):
        off, on = (ic.built("sunrgbd-f%ds1-%s-n257" % (f, tiny))["want"] for f in (0, 1))
        flipped = [not np.array_equal(on["point_cloud"][b, 0], off["point_cloud"][b, 0]) for b in range(6)]
        assert flipped == [c > 0.5 for c in ic.SUN_COIN] == [False, True, False, True, False, True]


@pytest.mark.parametrize("N", [1, 2, 257])
def test_sunrgbd_choice_rule(N):
    """draw_sunrgbd replaces only when a record has fewer points than N: for n >= N the drawn indices are distinct, for n < N
    they are N indices into the n points (a multiset)."""
    from frustum_convnet_amd.inputs import draw_sunrgbd
    counts = [n for n in (N - 1, N, N + 1) if n > 0]
    choice, coin, normal, hshift = draw_sunrgbd(counts, N, True, True, np.random.RandomState(5 + N))
    assert choice.shape == (len(counts), N) and choice.dtype == np.int32
    assert coin.shape == normal.shape == hshift.shape == (len(counts),)
    for n, row in zip(counts, choice):
        assert row.min() >= 0 and row.max() < n
        if n >= N:
            assert len(set(row.tolist())) == N, (n, N)
        else:
            assert len(row) == N > len(set(row.tolist())), (n, N)          # N draws from fewer than N points: repeats
    if N > 1:
        assert sorted(choice[counts.index(N)].tolist()) == list(range(N))  # n == N without replacement: a permutation
    # switched-off augmentations draw nothing and hand back the neutral values
    _, coin0, normal0, hshift0 = draw_sunrgbd(counts, N, False, False, np.random.RandomState(1))
    assert not coin0.any() and not normal0.any() and (hshift0 == 0.5).all()


def _refine_builder():
    from frustum_convnet_amd.config import reset_cfg
    from frustum_convnet_amd.inputs import RefineInputBuilder
    reset_cfg()
    return RefineInputBuilder(64, strides=ic.REFINE_STRIDES)


def test_lpad_refuses_a_sample_without_a_window():
    b = _refine_builder()
    assert b._lpad([1.6, 0.9, 0.05]) == [16, 8, 4, 2] and b._lpad(np.array([60.0])) == [600, 300, 150, 75]
    with pytest.raises(ValueError, match=r"sample 1\b.*-0\.3"):
        b._lpad([1.6, -0.3, 0.0])
    with pytest.raises(ValueError, match=r"sample 0\b.*0\.0"):
        b._lpad([0.0, 1.6])
    with pytest.raises(ValueError, match=r"sample 2\b.*nan"):
        b._lpad(np.array([1.6, 0.9, float("nan")]))
