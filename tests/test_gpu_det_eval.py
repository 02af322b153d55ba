"""-m gpu: matching and AP on the device (fcn_det_match, fcn_det_ap, evaluate.match_detections_ap; csrc/det_eval.h) against the
reference's recorded eval_det_cls run (tests/golden/sunrgbd_detect.npz) and against its fp64 numpy restatement
(tests/sunrgbd_detect_ref.py) on a scene that holds, by construction, the group and class sizes the kernels' loops turn on.
tests/test_emu_det_eval.py runs the same functions on the host emulation of the kernels."""
import functools

import numpy as np
import pytest
import torch

import sunrgbd_detect_ref as ref
from test_sunrgbd_detect_referee import golden

pytestmark = pytest.mark.gpu
BADARG = 10001                     # FCN_E_BADARG
THRESH, MARGIN = 0.25, 1e-3        # the margins of the golden fixture: the fp32 IoU (bar 5e-5) leaves the flags no room
KEYS = ("tp", "ovmax", "jmax", "rank", "rec", "prec", "ap", "npos")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _p(t):
    return None if t is None else t.data_ptr()


def _box(rng, centre=None):
    c = rng.uniform([-1.0, -0.3, -1.0], [1.0, 0.6, 1.0]) if centre is None else np.asarray(centre, dtype=np.float64)
    return np.concatenate([c, np.array([1.0, 0.8, 0.9]) * rng.uniform(0.7, 1.4, 3), [rng.uniform(-np.pi, np.pi)]])


def _jitter(rng, box, amount):
    b = box.copy()
    b[:3] += rng.normal(0, amount, 3)
    b[3:6] *= rng.uniform(1 - amount, 1 + amount, 3)
    b[6] += rng.normal(0, amount)
    return b


def _acceptable(v):
    if len(v) == 0:
        return True
    s = np.sort(v)[::-1]
    if abs(s[0] - THRESH) <= MARGIN:
        return False
    return not (s[0] > THRESH and len(s) > 1 and s[0] - s[1] <= MARGIN)


def _group(rng, n_labels, n_dets):
    """Label boxes on a 2.5 m grid (+ 3 m in front of the camera), detections jittered about one of them or anywhere over the
    grid; a detection too close to a decision (the fixture's margins) is redrawn.  -> label corners, detection corners (float32)."""
    side = max(1, int(np.ceil(np.sqrt(n_labels))))
    spots = [(2.5 * (k % side), 0.0, 3.0 + 2.5 * (k // side)) for k in range(n_labels)]
    labels = [_box(rng, np.asarray(s) + rng.uniform(-0.4, 0.4, 3) * [1, 0.3, 1]) for s in spots]
    gc = ref.corners(np.stack(labels)).astype(np.float32) if labels else np.zeros((0, 8, 3), dtype=np.float32)
    dc = np.zeros((n_dets, 8, 3), dtype=np.float32)
    for d in range(n_dets):
        for _ in range(200):
            if labels and rng.uniform() < 0.7:
                row = _jitter(rng, labels[rng.integers(len(labels))], rng.choice([0.05, 0.15, 0.4]))
            else:
                row = _box(rng, (rng.uniform(-1, 2.5 * side), rng.uniform(-0.3, 0.3), rng.uniform(2.0, 3.0 + 2.5 * side)))
            c = ref.corners(row[None])[0].astype(np.float32)
            if _acceptable(ref.iou3d(c, gc)):
                break
        else:
            raise RuntimeError("re-draw did not terminate")
        dc[d] = c
    return gc, dc


@functools.lru_cache(maxsize=None)
def _scene():
    """Classes 0 / 1 / 2 of 1 / 257 / 5000 detections (the AP kernel's scan chunks of 256: one, two with a single element in the
    second, twenty), class 3 with label boxes and no detection, class 4 with one group of 300 detections x 40 label boxes (more
    than the matcher's 256 threads) and the constructed cases.  Returns the inputs, the restatement's answer and the groups
    of the cases."""
    rng = np.random.default_rng(77)
    plan = [(0, 2, 1), (1, 3, 200), (1, 0, 57)] + [(2, 3, 200)] * 25 + [(3, 5, 0), (4, 40, 300), (4, 2, 0)]
    gts, dets, gcls = [], [], []
    for c, m, n in plan:
        gc, dc = _group(rng, m, n)
        gts.append(gc); dets.append(dc); gcls.append(c)
    f32 = lambda rows: ref.corners(np.stack(rows)).astype(np.float32)
    # two detections on one label box; and: best label taken while a second one qualifies (still a false positive)
    one = _box(rng, (0.0, 0.1, 3.0))
    gts.append(f32([one])); dets.append(f32([_jitter(rng, one, 0.05), _jitter(rng, one, 0.05)])); gcls.append(4)
    a, b = np.array([0.0, 0.0, 3.0, 1.0, 1.0, 1.0, 0.0]), np.array([0.6, 0.0, 3.0, 1.0, 1.0, 1.0, 0.0])
    between = np.array([0.25, 0.0, 3.0, 1.0, 1.0, 1.0, 0.0])
    gts.append(f32([a, b])); dets.append(f32([_jitter(rng, a, 0.01), _jitter(rng, between, 0.005)])); gcls.append(4)
    G = len(gcls)
    det_off = np.concatenate([[0], np.cumsum([len(x) for x in dets])]).astype(np.int64)
    gt_off = np.concatenate([[0], np.cumsum([len(x) for x in gts])]).astype(np.int64)
    det_c, gt_c = np.concatenate(dets), np.concatenate(gts)
    nd = len(det_c)
    scores = rng.permutation(nd).astype(np.float32) / np.float32(nd) + np.float32(0.1)          # distinct, exact in float32
    lo, hi = sorted(scores[det_off[G - 1]:det_off[G]].tolist())
    scores[det_off[G - 1]], scores[det_off[G - 1] + 1] = hi, lo                                  # the detection ON a scores higher
    assert len(np.unique(scores)) == nd
    want = ref.evaluate(det_c, scores, det_off, gt_c, gt_off, gcls, 5, THRESH)
    return {"det_c": det_c, "scores": scores, "det_off": det_off, "gt_c": gt_c, "gt_off": gt_off, "gcls": np.asarray(gcls), "C": 5,
            "want": want, "G": G}


def _run(det_c, scores, det_off, gt_c, gt_off, gcls, C, thresh=THRESH):
    from frustum_convnet_amd import evaluate
    out = evaluate.match_detections_ap(_dev(det_c), _dev(scores), det_off, _dev(gt_c), gt_off, gcls, C, thresh)
    torch.cuda.synchronize()
    assert sorted(out) == sorted(KEYS) and all(out[k].is_cuda for k in out)
    assert out["tp"].dtype == torch.int32 and out["rec"].dtype == torch.float64 and out["ovmax"].dtype == torch.float32
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, want, what):
    assert np.array_equal(got["tp"], want["tp"]) and np.array_equal(got["jmax"], want["jmax"]), what
    assert np.array_equal(got["rank"], want["rank"]) and np.array_equal(got["npos"], want["npos"]), what
    fin = np.isfinite(want["ovmax"])
    assert np.array_equal(np.isneginf(got["ovmax"]), ~fin), what
    err = np.abs(got["ovmax"][fin] - want["ovmax"][fin]).max() if fin.any() else 0.0
    cur = max(np.abs(got[k] - want[k]).max() if len(want[k]) else 0.0 for k in ("rec", "prec"))
    ape = np.abs(got["ap"] - want["ap"]).max()
    print("%s: %d detections, tp %d; ovmax worst %.3e, rec / prec worst %.3e, ap worst %.3e, ap %s" %
          (what, len(want["tp"]), int(want["tp"].sum()), err, cur, ape, np.round(got["ap"], 6).tolist()))
    assert err < 5e-5, what                # the project's IoU bar against the same python
    assert cur < 1e-12, what               # one fp64 division of integer counts
    assert ape < 1e-9, what                # integer counts: only the order of the fp64 summation differs


def test_matcher_and_ap_reproduce_the_references_recorded_run():
    g = golden()
    got = _run(g["ev_det_corners"], g["ev_scores"], g["ev_det_off"], g["ev_gt_corners"], g["ev_gt_off"], g["ev_group_class"],
               int(g["ev_num_classes"]), float(g["ev_thresh"]))
    fix = {k: g["ev_" + k] for k in KEYS}
    _compare(got, fix, "fixture")
    want = ref.evaluate(g["ev_det_corners"], g["ev_scores"], g["ev_det_off"], g["ev_gt_corners"], g["ev_gt_off"], g["ev_group_class"],
                        int(g["ev_num_classes"]), float(g["ev_thresh"]))
    _compare(got, want, "restatement")


def test_group_and_class_sizes_by_construction():
    sc = _scene()
    want, doff, goff, G = sc["want"], sc["det_off"], sc["gt_off"], sc["G"]
    got = _run(sc["det_c"], sc["scores"], doff, sc["gt_c"], goff, sc["gcls"], sc["C"])
    _compare(got, want, "scene")
    per_class = np.bincount(np.repeat(sc["gcls"], np.diff(doff)), minlength=5)
    assert per_class.tolist()[:4] == [1, 257, 5000, 0] and got["ap"][3] == 0.0 and (got["ap"][[1, 2, 4]] > 0).all()
    assert got["npos"].tolist() == np.bincount(sc["gcls"], weights=np.diff(goff), minlength=5).astype(int).tolist()
    tp, ov, jm = got["tp"], got["ovmax"], got["jmax"]
    g = 2                                                        # detections and no label box: all false positives
    assert goff[g + 1] == goff[g] and doff[g + 1] - doff[g] == 57 and not tp[doff[g]:doff[g + 1]].any()
    assert np.isneginf(ov[doff[g]:doff[g + 1]]).all() and (jm[doff[g]:doff[g + 1]] == -1).all()
    g = G - 3                                                    # label boxes and no detection: counted in npos only
    assert doff[g + 1] == doff[g] and goff[g + 1] - goff[g] == 2
    g = G - 4                                                    # 300 detections x 40 label boxes
    assert doff[g + 1] - doff[g] == 300 and goff[g + 1] - goff[g] == 40 and 0 < tp[doff[g]:doff[g + 1]].sum() <= 40
    assert jm[doff[g]:doff[g + 1]].max() > 30
    g = G - 2                                                    # two detections on one label box: the second is a false positive
    assert sorted(tp[doff[g]:doff[g + 1]].tolist()) == [0, 1] and (ov[doff[g]:doff[g + 1]] > THRESH).all()
    g = G - 1                                                    # best label taken, a second one qualifies: still a false positive
    assert tp[doff[g]:doff[g + 1]].tolist() == [1, 0] and jm[doff[g] + 1] == 0 and ov[doff[g] + 1] > THRESH
    assert ref.iou3d(sc["det_c"][doff[g] + 1], sc["gt_c"][goff[g]:goff[g + 1]])[1] > THRESH + MARGIN
    # the curve of the 5000-detection class crosses twenty scan chunks: cumulative counts end at the class's totals
    base, n = per_class[:2].sum(), 5000
    cls2 = np.repeat(sc["gcls"], np.diff(doff)) == 2
    assert abs(got["rec"][base + n - 1] * got["npos"][2] - tp[cls2].sum()) < 1e-9
    assert abs(got["prec"][base + n - 1] * n - tp[cls2].sum()) < 1e-9
    assert sorted(got["rank"][cls2].tolist()) == list(range(n))


def test_equal_scores_rank_the_lower_index_first():
    """The documented tie rule (the reference's np.argsort is unstable here): restatement only."""
    g = golden()
    box = g["ev_gt_corners"][:1]
    nested = (box.mean(1, keepdims=True) + 0.9 * (box - box.mean(1, keepdims=True))).astype(np.float32)
    far = (box + np.float32(50.0)).astype(np.float32)
    det_c = np.concatenate([far, nested, nested, far])
    scores = np.asarray([0.7, 0.7, 0.7, 0.9], dtype=np.float32)
    args = (det_c, scores, [0, 4], box, [0, 1], [0], 1)
    want = ref.evaluate(*args)
    got = _run(*args)
    _compare(got, want, "ties")
    assert got["rank"].tolist() == [1, 2, 3, 0] and got["tp"].tolist() == [0, 1, 0, 0]


def _raw_buffers(nd, C, guard=3):
    i32, dev = dict(dtype=torch.int32, device="cuda"), "cuda"
    return {"tp": torch.full((nd + guard,), -7, **i32), "ovmax": torch.full((nd + guard,), -7.0, dtype=torch.float32, device=dev),
            "jmax": torch.full((nd + guard,), -7, **i32), "rank": torch.full((nd + guard,), -7, **i32),
            "rec": torch.full((nd + guard,), -7.0, dtype=torch.float64, device=dev),
            "prec": torch.full((nd + guard,), -7.0, dtype=torch.float64, device=dev),
            "ap": torch.full((C + guard,), -7.0, dtype=torch.float64, device=dev)}


def test_raw_entries_poisoned_outputs_and_refusals():
    from frustum_convnet_amd import _native, evaluate
    g = golden()
    nd, ng, G, C = len(g["ev_scores"]), len(g["ev_gt_corners"]), len(g["ev_group_class"]), int(g["ev_num_classes"])
    L, s = _native.lib(), _native.current_stream()
    t = {"doff": _dev(g["ev_det_off"].astype(np.int32)), "goff": _dev(g["ev_gt_off"].astype(np.int32)), "dc": _dev(g["ev_det_corners"]),
         "sc": _dev(g["ev_scores"]), "gc": _dev(g["ev_gt_corners"]), "npos": _dev(g["ev_npos"].astype(np.int32)),
         "cls": _dev(np.repeat(g["ev_group_class"], np.diff(g["ev_det_off"])).astype(np.int32))}
    o = _raw_buffers(nd, C)
    match = lambda o: [_p(t["doff"]), _p(t["goff"]), G, _p(t["dc"]), _p(t["sc"]), nd, _p(t["gc"]), ng, THRESH, _p(o["tp"]),
                       _p(o["ovmax"]), _p(o["jmax"]), s]
    ap = lambda o: [_p(o["tp"]), _p(t["sc"]), _p(t["cls"]), nd, _p(t["npos"]), C, _p(o["rank"]), _p(o["rec"]), _p(o["prec"]),
                    _p(o["ap"]), s]
    # every refusal first: nothing is written by any of them
    for i in (0, 1, 3, 4, 6, 9, 10, 11):
        bad = match(o); bad[i] = None
        assert L.fcn_det_match(*bad) == BADARG, i
    for i, v in ((2, -1), (5, -1), (7, -1), (8, float("nan"))):
        bad = match(o); bad[i] = v
        assert L.fcn_det_match(*bad) == BADARG, (i, v)
    for i in (0, 1, 2, 4, 6, 7, 8, 9):
        bad = ap(o); bad[i] = None
        assert L.fcn_det_ap(*bad) == BADARG, i
    for i, v in ((3, -1), (5, -1)):
        bad = ap(o); bad[i] = v
        assert L.fcn_det_ap(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in o.values())
    # accepted: the results are the fixture's, every element written, the entries behind them untouched
    assert L.fcn_det_match(*match(o)) == 0 and L.fcn_det_ap(*ap(o)) == 0
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in o.items()}
    assert all((h[k][nd:] == -7).all() for k in o if k != "ap") and (h["ap"][C:] == -7).all()
    got = {k: (h[k][:C] if k == "ap" else h[k][:nd]) for k in o}
    got["npos"] = g["ev_npos"]
    _compare(got, {k: g["ev_" + k] for k in KEYS}, "raw entries")
    # empty problems touch nothing: no group, no detection, no class
    o2 = _raw_buffers(nd, C)
    e = match(o2); e[2] = 0
    assert L.fcn_det_match(*e) == 0
    e = match(o2); e[5] = 0
    assert L.fcn_det_match(*e) == 0
    e = ap(o2); e[5] = 0
    assert L.fcn_det_ap(*e) == 0
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in o2.values())
    e = ap(o2); e[3] = 0                                           # no detection at all: every class has AP 0
    assert L.fcn_det_ap(*e) == 0
    torch.cuda.synchronize()
    assert (o2["ap"].cpu().numpy()[:C] == 0).all() and (o2["ap"].cpu().numpy()[C:] == -7).all() and (o2["rec"].cpu().numpy() == -7).all()
    # offsets that run past the buffers are clamped to them: the matcher reads and writes inside nd / ng
    o3 = _raw_buffers(nd, C)
    far = g["ev_det_off"].astype(np.int32).copy(); far[-1] = nd + 1000
    gfar = g["ev_gt_off"].astype(np.int32).copy(); gfar[-1] = ng + 1000
    fd, fg = _dev(far), _dev(gfar)
    e = match(o3); e[0], e[1] = _p(fd), _p(fg)
    assert L.fcn_det_match(*e) == 0
    torch.cuda.synchronize()
    assert all((o3[k].cpu().numpy()[nd:] == -7).all() for k in ("tp", "ovmax", "jmax"))
    assert np.array_equal(o3["tp"].cpu().numpy()[:nd], g["ev_tp"])
    # the host side refuses what it can see: offsets, classes, a class without a label box
    good = (_dev(g["ev_det_corners"]), _dev(g["ev_scores"]), g["ev_det_off"], _dev(g["ev_gt_corners"]), g["ev_gt_off"], g["ev_group_class"], C)
    swapped = g["ev_det_off"].copy(); swapped[1] = nd                 # descends behind its second entry
    for k, v in ((2, swapped), (2, g["ev_det_off"] + 1), (2, g["ev_det_off"][:-1]), (4, g["ev_gt_off"][::-1].copy()),
                 (4, np.concatenate([g["ev_gt_off"][:-1], [ng + 1]])), (5, g["ev_group_class"] + 1), (5, -g["ev_group_class"] - 1),
                 (6, C + 1), (1, g["ev_scores"][:-1])):
        bad = list(good); bad[k] = v
        with pytest.raises(ValueError):
            evaluate.match_detections_ap(*bad)
    only3 = g["ev_group_class"] == 3                                # drop class 3's label boxes: npos[3] == 0
    keep = np.repeat(~only3, np.diff(g["ev_gt_off"]))
    goff = np.concatenate([[0], np.cumsum(np.where(only3, 0, np.diff(g["ev_gt_off"])))])
    with pytest.raises(ValueError, match="npos"):
        evaluate.match_detections_ap(good[0], good[1], g["ev_det_off"], _dev(g["ev_gt_corners"][keep]), goff, g["ev_group_class"], C)
