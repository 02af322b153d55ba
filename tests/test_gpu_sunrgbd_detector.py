"""-m gpu: evaluate.SunrgbdDetector -- detect_frames + evaluate on the synthetic depth frames of tests/golden/frustum_sunrgbd.npz with
the five-scale model (B = 3 surviving boxes) -- against the same steps called one by one, and the no-survivor return.
tests/test_emu_det_eval.py runs the same functions on the host emulation of the kernels."""
import numpy as np
import pytest
import torch

import frustum_sunrgbd_ref as fref
import sunrgbd_detect_ref as ref
from test_gpu_frustum_sunrgbd import _builder, _dev, _golden

pytestmark = pytest.mark.gpu
PICK = np.asarray([0, 1, 3, 4])                       # boxes of the fixture: 3 selects fewer than 5 points and is dropped
TYPES = ["bed", "bed", "desk", "toilet"]              # two boxes of one (frame, class): one NMS group of two frustums
DRAW_ROWS = [0, 1, 3]                                 # their rows in the fixture's recorded draws (det_kept = 0 1 2 4 5 6)


def _setup():
    from frustum_convnet_amd.config import cfg
    from frustum_convnet_amd import det_base_sunrgbd, synth
    g = _golden()
    b = _builder(g, False, False)                      # (resets cfg)
    cfg.DATA.HEIGHT_HALF = tuple(float(x) for x in g["meta_strides"])
    cfg.DATA.STRIDE = cfg.DATA.HEIGHT_HALF
    cfg.DATA.DATASET_NAME = "SUNRGBD"
    cfg.DATA.MAX_DEPTH = float(g["meta_max_depth"])
    m = det_base_sunrgbd.PointNetDet(3, num_vec=10, num_classes=2)
    synth.fill_state_dict(m.state_dict(), seed=7)
    with torch.no_grad():                              # size residuals near 0: every decoded box has the size of its cluster
        m.reg_out.weight[3 + 2 * 12 + 10:] *= 0.05
        m.reg_out.bias[3 + 2 * 12 + 10:] *= 0.05
    m = m.cuda().eval()
    dev = {k: _dev(g[k]) for k in ("points", "off", "K", "Rtilt")}
    sub = fref.fixture_sub(g, "det")
    args = dict(boxes=g["det_boxes"][PICK], bframe=g["det_frame"][PICK], prob=g["det_prob"][PICK], sub=[sub[d] for d in PICK],
                draws=(g["det_draw_choice"][DRAW_ROWS],))
    return g, b, m, dev, args


def test_detect_frames_and_evaluate_equal_the_steps_one_by_one():
    from frustum_convnet_amd import detect, evaluate, frustum
    from frustum_convnet_amd.config import reset_cfg
    try:
        g, b, m, dev, a = _setup()
        det = evaluate.SunrgbdDetector(m, b)
        res = det.detect_frames(dev["points"], dev["off"], dev["K"], dev["Rtilt"], a["boxes"], a["bframe"], TYPES, a["prob"], "nms", 0.1,
                                draws=a["draws"], sub=a["sub"])
        # ---- one by one
        sel = frustum.sunrgbd_candidates(dev["points"], dev["off"], dev["K"], dev["Rtilt"], a["boxes"], a["bframe"], sub=a["sub"])
        batch = b.build_device(sel, dev["K"], dev["Rtilt"], TYPES, a["prob"], draws=a["draws"])
        kept = batch.pop("kept")
        assert kept.tolist() == [0, 1, 3] and np.array_equal(res["kept"], kept)
        ug = torch.tensor([0, 0, 1], dtype=torch.int32)               # (frame 0, bed) x 2, (frame 1, toilet)
        dets, valid, keep, cnt = m.detect(batch, unit_group=ug, num_groups=2, method="nms", thresh=0.1, rule="sunrgbd")
        for k, v in (("dets", dets), ("valid", valid), ("keep", keep), ("cnt", cnt)):
            assert torch.equal(res[k], v), k
        cnt_h, keep_h = cnt.cpu().numpy(), keep.cpu().numpy()
        rows = np.concatenate([keep_h[q, :cnt_h[q]] for q in range(2)]).astype(np.int64)
        print("kept rows per group", cnt_h.tolist(), "of", int(valid.sum()), "valid")
        assert (cnt_h >= 1).all() and np.array_equal(res["rows"], rows) and res["rows"].dtype == np.int64
        assert res["det_off"].tolist() == [0, int(cnt_h[0]), int(cnt_h.sum())]
        classes = b.classes
        assert res["group_frame"].tolist() == [0, 1] and res["group_class"].tolist() == [classes.index("bed"), classes.index("toilet")]
        cor = detect.box3d_corners(dets, rows)
        assert torch.equal(res["corners"], cor) and torch.equal(res["scores"], dets[:, 7][torch.from_numpy(rows).cuda()])
        d_h = dets.cpu().numpy()[rows]
        assert np.abs(cor.cpu().numpy() - ref.corners(d_h)).max() < 1e-5
        L2 = batch["center_ref2"].shape[2]
        assert set((rows // L2).tolist()) <= {0, 1, 2} and (valid.cpu().numpy()[rows] != 0).all()
        # ---- evaluate: label boxes = shrunk copies of the best detection of each group, one far box, one label-only group, and a
        # box of a class without any detection; detections of no labelled class do not exist here
        cor_h = cor.cpu().numpy()
        shrink = lambda c: (c.mean(0, keepdims=True) + 0.9 * (c - c.mean(0, keepdims=True))).astype(np.float32)
        gt = np.stack([shrink(cor_h[0]), cor_h[0] + np.float32(40.0), shrink(cor_h[cnt_h[0]]), shrink(cor_h[0]), shrink(cor_h[0])])
        gt_frame, gt_class = [0, 0, 1, 1, 0], [classes.index("bed")] * 2 + [classes.index("toilet")] + [classes.index("bed"), classes.index("sofa")]
        ev = det.evaluate(res, gt, gt_frame, gt_class)
        cls_ids = sorted({classes.index(x) for x in ("bed", "toilet", "sofa")})
        assert ev["classes"].tolist() == cls_ids and np.array_equal(ev["det_index"], np.arange(len(rows)))
        remap = {c: i for i, c in enumerate(cls_ids)}
        # groups: the detector's two, then the label-only ones ordered by (frame, class)
        extra = sorted([(1, classes.index("bed")), (0, classes.index("sofa"))])
        gcls = [remap[classes.index("bed")], remap[classes.index("toilet")]] + [remap[c] for _, c in extra]
        order = [0, 1, 2] + ([3, 4] if extra[0] == (1, classes.index("bed")) else [4, 3])
        goff = [0, 2, 3, 4, 5]
        doff = [0, int(cnt_h[0]), int(cnt_h.sum()), int(cnt_h.sum()), int(cnt_h.sum())]
        one = evaluate.match_detections_ap(cor, res["scores"], doff, _dev(gt[order]), goff, gcls, 3)
        for k in one:
            assert torch.equal(ev[k], one[k]), k
        want = ref.evaluate(cor_h, res["scores"].cpu().numpy(), doff, gt[order], goff, gcls, 3)
        got = {k: v.cpu().numpy() for k, v in one.items()}
        print("tp", got["tp"].tolist(), "ap", got["ap"].tolist(), "npos", got["npos"].tolist())
        fin = np.isfinite(want["ovmax"])
        assert np.abs(got["ovmax"][fin] - want["ovmax"][fin]).max() < 5e-5 and np.array_equal(got["npos"], want["npos"])
        assert got["npos"].tolist() == [3, 1, 1] and got["ap"][remap[classes.index("sofa")]] == 0.0
        assert got["tp"][0] == 1 and abs(got["ovmax"][0] - 0.729) < 1e-3 and got["tp"][cnt_h[0]] == 1       # the shrunk copies: 0.9 ** 3
        assert np.array_equal(got["rank"], want["rank"])
    finally:
        reset_cfg()


def test_no_box_survives():
    from frustum_convnet_amd import evaluate
    from frustum_convnet_amd.config import reset_cfg
    try:
        g, b, m, dev, a = _setup()
        det = evaluate.SunrgbdDetector(m, b)
        away = np.asarray([[5000.0, 5000.0, 5100.0, 5100.0]] * 2)
        res = det.detect_frames(dev["points"], dev["off"], dev["K"], dev["Rtilt"], away, np.zeros(2, np.int32), ["bed", "sofa"],
                                [0.5, 0.5], "nms", 0.1)
        assert len(res["kept"]) == 0 and res["kept"].dtype == np.int64 and len(res["rows"]) == 0 and res["det_off"].tolist() == [0]
        assert all(res[k] is None for k in ("dets", "valid", "keep", "cnt", "corners", "scores"))
        assert len(res["group_frame"]) == 0 and len(res["group_class"]) == 0
        gt = ref.corners(np.asarray([[0.0, 0.0, 3.0, 1.0, 1.0, 1.0, 0.3]])).astype(np.float32)
        ev = det.evaluate(res, gt, [0], [1])                          # nothing detected: AP 0 over the labelled classes
        assert ev["ap"].cpu().numpy().tolist() == [0.0] and ev["npos"].cpu().numpy().tolist() == [1] and ev["tp"].numel() == 0
        assert ev["classes"].tolist() == [1]
        with pytest.raises(ValueError):
            det.evaluate(res, gt[:0], [], [])
    finally:
        reset_cfg()
