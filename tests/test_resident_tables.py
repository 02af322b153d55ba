"""The shared host side of the capturable sources (frustum_convnet_amd/resident.py), exercised directly: the refusals of the label
table, the detection table and the held-tensor check, the K / Rtilt parser and the spare corners -- on the CPU, no kernel runs -- and,
marked gpu (tests/test_emu_resident_tables.py runs them under the emulation too), what set_boxes leaves in the tables of the two
inference sources."""
import types

import numpy as np
import pytest
import torch

from frustum_convnet_amd import resident

CLASSES = ["Car", "Pedestrian", "Cyclist"]
BUILDER = types.SimpleNamespace(device=torch.device("cuda"), classes=CLASSES)
GT2D = np.asarray([[100.0, 50.0, 300.0, 200.0], [400.0, 80.0, 500.0, 180.0], [10.0, 20.0, 60.0, 90.0]])
GT3D = np.arange(21, dtype=np.float64).reshape(3, 7)
WH = np.asarray([[1242.0, 375.0], [1224.0, 370.0]])


def _labels(gt2d=GT2D, gt3d=GT3D, frame=(0, 1, 0), names=("Car", "Cyclist", "Car"), F=2):
    return resident.LabelTable("who", gt2d, gt3d, np.asarray(frame), names, F)


def test_label_table_refusals():
    with pytest.raises(ValueError, match=r"^who: 3 box_frame, 2 gt_box2d, 3 gt_box3d, 3 types$"):
        _labels(gt2d=GT2D[:2])
    with pytest.raises(ValueError, match=r"^who: 3 box_frame, 3 gt_box2d, 3 gt_box3d, 2 types$"):
        _labels(names=("Car", "Car"))
    for frame in ((0.0, 1.0, 0.0), (0, 2, 0), (0, -1, 0)):
        with pytest.raises(ValueError, match=r"^who: box_frame must hold integers in \[0, 2\)$"):
            _labels(frame=frame)
    with pytest.raises(ValueError, match=r"^who: box_frame must hold integers in \[0, 2\)$"):
        _labels(GT2D[:0], GT3D[:0], np.zeros(0, dtype=np.int64), ())
    flat = GT2D.copy()
    flat[1, 3] = flat[1, 1]
    with pytest.raises(ValueError, match=r"^who: label box 1 is degenerate: \(.*400\.0.*80\.0.*500\.0.*80\.0.*\)$"):
        _labels(gt2d=flat).load(BUILDER, "cpu", 2, False, None, 0.1, WH)
    far = GT2D.copy()
    far[2] = [5000.0, 20.0, 5050.0, 90.0]
    with pytest.raises(ValueError, match=r"^who: label box 2 cannot be perturbed into the 1242 x 375 image: "):
        _labels(gt2d=far).load(BUILDER, "cpu", 2, True, None, 0.1, WH)
    with pytest.raises(ValueError, match=r"^who: select_box2d goes with perturb=False$"):
        _labels().load(BUILDER, "cpu", 2, True, GT2D, 0.1, WH)
    with pytest.raises(ValueError, match=r"^who: select_box2d goes with perturb=False$"):
        _labels().load(BUILDER, "cpu", 2, True, GT2D)                       # (without a clip as well: SUN-RGBD)
    with pytest.raises(ValueError, match=r"^who: 2 select_box2d for 3 labels$"):
        _labels().load(BUILDER, "cpu", 2, False, GT2D[:2])
    with pytest.raises(ValueError, match=r"^who: type 'Tram' is not one of \('Car', 'Pedestrian', 'Cyclist'\)$"):
        _labels(names=("Car", "Tram", "Car")).load(BUILDER, "cpu", 2, False, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _labels().load(types.SimpleNamespace(device=torch.device("cpu"), classes=CLASSES), "cpu", 2, False, None)
    _labels(gt2d=flat).load(BUILDER, "cpu", 2, False, None)                 # no clip, no retry: nothing of the boxes to refuse
    _labels(gt2d=far).load(BUILDER, "cpu", 2, False, None, 0.1, WH)         # not perturbed: only the degenerate box is refused


def test_label_table_holds_and_gathers_the_labels():
    lab = _labels().load(BUILDER, "cpu", 2, False, GT2D + 1.0)
    assert lab.G == 3 and lab.boxes is lab.sel2d and lab.pick_idx.tolist() == [[0, 1]] and lab.g_count.tolist() == [3]
    assert lab.g_class.tolist() == [[0], [2], [0]] and lab.g_class.dtype == torch.int64 and lab.g_frame.dtype == torch.int32
    assert torch.equal(lab.g_heading, torch.from_numpy(GT3D[:, 6])) and torch.equal(lab.eye, torch.eye(3))
    lab.pick_idx.copy_(torch.tensor([[2, 1]], dtype=torch.int32))
    lab._gather_labels()
    assert np.array_equal(lab.gt2d.numpy(), GT2D[[2, 1]]) and np.array_equal(lab.sel2d.numpy(), GT2D[[2, 1]] + 1.0)
    assert np.array_equal(lab.gt3d.numpy(), GT3D[[2, 1]]) and lab.bframe.tolist() == [0, 1]
    assert _labels().load(BUILDER, "cpu", 2, True, None).boxes is not lab.sel2d
    holder = types.SimpleNamespace()
    resident.adopt(holder, lab)
    assert sorted(vars(holder)) == sorted(resident.LabelTable.NAMES) and holder.gt2d is lab.gt2d


BOXES = np.asarray([[10.0, 20.0, 110.0, 220.0], [30.0, 40.0, 130.0, 240.0], [50.0, 60.0, 150.0, 260.0]])
GOOD = (BOXES, [0, 1, 1], ["Car", "Cyclist", "Pedestrian"], [0.9, 0.5, 0.25])


def _table(spare_group=4):
    return resident.DetectTable("cpu", 5, 2, CLASSES, spare_group)


def test_detect_table_refusals_and_rows():
    tab = _table()
    six = (np.tile(BOXES, (2, 1)), [0] * 6, ["Car"] * 6, [0.5] * 6)
    with pytest.raises(ValueError, match=r"^s: 6 boxes \(at most 5\), 6 frames, 6 types, 6 scores, 6 groups$"):
        tab.set_boxes("s", *six)
    with pytest.raises(ValueError, match=r"^s: 6 boxes \(at most 5\), 6 frames, 6 types, 6 scores$"):
        _table(None).set_boxes("s", *six)
    with pytest.raises(ValueError, match=r"^s: 3 boxes \(at most 5\), 3 frames, 3 types, 3 scores, 2 groups$"):
        tab.set_boxes("s", *GOOD, [0, 1])
    bad = BOXES.copy()
    bad[1, 2] = np.inf
    with pytest.raises(ValueError, match=r"^s: boxes and scores must be finite$"):
        tab.set_boxes("s", bad, *GOOD[1:])
    with pytest.raises(ValueError, match=r"^s: boxes and scores must be finite$"):
        tab.set_boxes("s", *GOOD[:3], [0.9, np.nan, 0.1])
    with pytest.raises(ValueError, match=r"^s: frames must be integers in \[0, 2\) and groups integers in \[0, 4\)$"):
        tab.set_boxes("s", BOXES, [0, 2, 1], *GOOD[2:])
    with pytest.raises(ValueError, match=r"^s: frames must be integers in \[0, 2\)$"):
        _table(None).set_boxes("s", BOXES, [0, 2, 1], *GOOD[2:])
    with pytest.raises(ValueError, match=r"^s: frames must be integers in \[0, 2\)$"):
        _table(None).set_boxes("s", BOXES, [0.0, 1.0, 1.0], *GOOD[2:])
    with pytest.raises(ValueError, match=r"^s: type 'Tram' is not one of \('Car', 'Pedestrian', 'Cyclist'\)$"):
        tab.set_boxes("s", BOXES, [0, 1, 1], ["Car", "Tram", "Car"], GOOD[3])
    with pytest.raises(ValueError, match=r"groups integers in \[0, 4\)$"):
        tab.set_boxes("s", *GOOD, [0, 4, 1])                                # a group == spare_group
    with pytest.raises(ValueError, match=r"groups integers in \[0, 2\)$"):
        _table(2).set_boxes("s", *GOOD)                                    # every box its own group needs n <= spare_group
    assert tab.n_boxes.tolist() == [0] and not tab.boxes2d[:5].any()        # a refused fill writes nothing
    tab.set_boxes("s", *GOOD, [3, 0, 3])
    assert tab.n_boxes.tolist() == [3] and np.array_equal(tab.boxes2d[:3].numpy(), BOXES) and tab.box_frame[:3].tolist() == [0, 1, 1]
    assert tab.box_class[:3].tolist() == [0, 2, 1] and tab.box_group[:3].tolist() == [3, 0, 3] and np.array_equal(tab.box_prob[:3].numpy(), np.float32([0.9, 0.5, 0.25]))
    tab.set_boxes("s", np.zeros((0, 4)), [], [], [])                        # n = 0: no live row; the rows stay as they are
    assert tab.n_boxes.tolist() == [0] and np.array_equal(tab.boxes2d[:3].numpy(), BOXES)
    # the spare row D: a unit box, frame 0, class 0, the spare group, probability 0
    assert tab.boxes2d[5].tolist() == [0.0, 0.0, 1.0, 1.0] and tab.box_frame[5] == 0 and tab.box_class[5] == 0 and tab.box_group[5] == 4
    assert tab.box_prob[5] == 0 and not hasattr(_table(None), "box_group") and "box_group" in tab.NAMES


def test_held_tensor_check(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))          # (a CPU tensor standing in for a device tensor)
    good = torch.zeros((4, 8))
    resident.held("who", good)
    resident.held("who", good, "dets", "(R, 8)", lambda t: t.shape[1] == 8)
    text = r"^who: frame_points must be a contiguous \(n >= 1, >= 3\) float32 device tensor \(it is held, not copied\)$"
    for t in (torch.zeros((4, 16))[:, ::2], good.double(), good[:0], good.clone().requires_grad_(), good[None], good.numpy()):
        with pytest.raises(ValueError, match=text):
            resident.held("who", t)
    with pytest.raises(ValueError, match=r"^who: dets must be a contiguous \(R, 8\) float32 device tensor \(it is held, not copied\)$"):
        resident.held("who", torch.zeros((4, 7)), "dets", "(R, 8)", lambda t: t.shape[1] == 8)
    monkeypatch.undo()
    with pytest.raises(ValueError, match=text):
        resident.held("who", good)                                          # not on the device


def test_intrinsics_parser():
    K = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    k9, r9 = resident.intrinsics("who", K, torch.from_numpy(K.astype(np.float64)).reshape(2, 9) + 1.0, 2, "cpu")
    assert k9.dtype == r9.dtype == torch.float64 and k9.shape == r9.shape == (2, 9) and k9.is_contiguous()
    assert np.array_equal(k9.numpy(), K.reshape(2, 9).astype(np.float64)) and np.array_equal(r9.numpy(), K.reshape(2, 9) + 1.0)
    with pytest.raises(ValueError, match=r"^who: K must hold 3 x 9 numbers, got \(2, 3, 3\)$"):
        resident.intrinsics("who", K, K, 3, "cpu")
    with pytest.raises(ValueError, match=r"^who: Rtilt must hold 2 x 9 numbers, got \(2, 8\)$"):
        resident.intrinsics("who", K, np.zeros((2, 8)), 2, "cpu")


def test_spare_corners_and_small_helpers():
    want = [0.5, 0.5, 0.5, 0.5, 0.5, -0.5, -0.5, 0.5, -0.5, -0.5, 0.5, 0.5, 0.5, -0.5, 0.5, 0.5, -0.5, -0.5, -0.5, -0.5, -0.5, -0.5, -0.5, 0.5]
    got = resident.spare_corners("cpu")
    assert got.dtype == torch.float64 and got.shape == (24,) and got.tolist() == want
    assert resident.class_index("who", CLASSES, []) == [] and resident.class_index("who", CLASSES, ["Cyclist", "Car"]) == [2, 0]
    with pytest.raises(ValueError, match=r"^who: need 1 <= B1 <= D <= 2048, got B1 = 4, D = 3$"):
        resident.check_slots("who", 4, 3, 2048, b="B1")
    with pytest.raises(ValueError, match=r"^who: need 1 <= B <= D <= G and D <= 2048, got B = 2, D = 5, G = 4$"):
        resident.check_slots("who", 2, 5, 2048, 4)
    with pytest.raises(ValueError, match=r"^who: D \* S = 5 \* 3 segments exceed the plan's 14$"):
        resident.check_segments("who", 5, 3, 14)
    with pytest.raises(ValueError, match=r"^who: capacity must be >= 1 row, got 0$"):
        resident.check_capacity("who", 0)
    resident.check_slots("who", 3, 3, 3)
    resident.check_segments("who", 5, 3, 15)
    pts, seg_off, off, counts, slot, n_kept, status = resident.batch_skeleton("cpu", 3, 5, 2, 7, 4, 5)
    assert pts.shape == (8, 4) and pts.dtype == torch.float32 and seg_off.shape == (11,) and off.shape == (4,) and counts.shape == (3,)
    assert seg_off.dtype == off.dtype == counts.dtype == torch.int64 and slot.tolist() == [5, 5, 5] and slot.dtype == torch.int32
    assert n_kept.tolist() == [0] and status.tolist() == [0] and n_kept.dtype == status.dtype == torch.int32


# ------------------------------------------------------------------------------------------------ the two inference sources' tables
def _kitti():
    import test_gpu_frustum_detect as m
    from test_gpu_frustum import _input_builder
    g = m._golden()
    src = m._source(_input_builder(32), 3, D=5, boxes=False)
    fill = lambda n, s=src: s.set_boxes(g["boxes"][:n], g["box_frame"][:n], m.TYPES9[:n], np.linspace(0.2, 0.95, 9)[:n], list(range(n)))
    given = lambda n: (g["boxes"][:n], g["box_frame"][:n], [CLASSES.index(t) for t in m.TYPES9[:n]], np.linspace(0.2, 0.95, 9)[:n])
    return src, fill, given, lambda: _kitti()[:2]


def _sunrgbd():
    import test_gpu_sunrgbd_detect_source as m
    g = m._golden()
    src = m._source(3, D=5, boxes=False)
    names = m._types(g)
    fill = lambda n, s=src: s.set_boxes(g["det_boxes"][:n], g["det_frame"][:n], names[:n], g["det_prob"][:n])
    given = lambda n: (g["det_boxes"][:n], g["det_frame"][:n], [src.builder.classes.index(t) for t in names[:n]], g["det_prob"][:n])
    return src, fill, given, lambda: _sunrgbd()[:2]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["kitti", "sunrgbd"])
def test_set_boxes_fills_the_table_and_the_plan_ignores_stale_rows(which):
    src, fill, given, fresh = (_kitti if which == "kitti" else _sunrgbd)()
    D = src.D
    rows = lambda n: (src.boxes2d[:n].cpu().numpy(), src.box_frame[:n].cpu().numpy(), src.box_class[:n].cpu().numpy(), src.box_prob[:n].cpu().numpy())
    fill(5)
    for got, want in zip(rows(5), given(5)):
        assert np.array_equal(got, np.asarray(want).astype(got.dtype))
    assert src.n_boxes.tolist() == [5] and src.boxes2d[D].tolist() == [0.0, 0.0, 1.0, 1.0] and src.box_frame[D] == 0 and src.box_class[D] == 0
    assert src.box_prob[D] == 0 and src.table.boxes2d is src.boxes2d and src.table.n_boxes is src.n_boxes
    if which == "kitti":
        assert src.box_group.tolist() == [0, 1, 2, 3, 4, src.spare_group]
    fill(2)                                                                 # fewer boxes: rows 2..4 stay behind n_boxes, stale
    for got, want in zip(rows(5), given(5)):
        assert np.array_equal(got, np.asarray(want).astype(got.dtype))
    assert src.n_boxes.tolist() == [2]
    other, fill_other = fresh()                                             # the same seed, the two boxes alone
    fill_other(2, other)
    a, b = src.step(), other.step()
    torch.cuda.synchronize()
    assert int(src.n_kept.cpu()[0]) == int(other.n_kept.cpu()[0]) <= 2 and torch.equal(src.slot_box.cpu(), other.slot_box.cpu())
    assert (src.slot_box.cpu()[int(src.n_kept.cpu()[0]):] == D).all()
    for k in ("point_cloud", "rot_angle", "rgb_prob", "one_hot"):
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
