"""-m gpu: the KITTI evaluation on the device (fcn_kitti_*, evaluate.kitti_label_rows / kitti_eval / kitti_results;
csrc/kitti_eval.h) against the fp64 restatement of the reference's evaluator (tests/kitti_eval_ref.py, made trustworthy by
tests/test_kitti_eval_referee.py) on seeded scenes that hold, by construction, the sizes the kernels' loops turn on
(tests/kitti_eval_scenes.py: the knife-edge condition keeps every decision off the fp32 overlaps' error), and against the
reference's own compute_alpha (tests/golden/kitti_eval.npz).  tests/test_emu_kitti_eval.py runs the kernel-level cases on the
host emulation of the kernels."""
import numpy as np
import pytest
import torch

import kitti_eval_ref as ref
import kitti_eval_scenes as scenes

pytestmark = pytest.mark.gpu
BADARG = 10001                     # FCN_E_BADARG
KEYS = ("precision", "aos", "ap", "aos_ap", "thresholds", "num_thresholds", "n_gt", "tp", "fp", "fn", "overlaps", "pair_off", "flags")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _p(t):
    return None if t is None else t.data_ptr()


def _run(sc, classes=(0, 1, 2)):
    from frustum_convnet_amd import evaluate
    out = evaluate.kitti_eval(_dev(sc["det"]), _dev(sc["det_class"]), sc["det_off"], _dev(sc["gt"]), _dev(sc["gt_type"]), sc["gt_off"],
                              classes)
    torch.cuda.synchronize()
    assert sorted(out) == sorted(KEYS) and all(out[k].is_cuda for k in out if k != "pair_off")
    assert out["precision"].dtype == torch.float64 and tuple(out["precision"].shape) == (3, 3, 3, 41)
    assert tuple(out["aos"].shape) == (3, 3, 41) and tuple(out["ap"].shape) == (3, 3, 3) and tuple(out["aos_ap"].shape) == (3, 3)
    assert tuple(out["thresholds"].shape) == (27, 41) and out["tp"].dtype == torch.int32 and tuple(out["fn"].shape) == (27, 41)
    return {k: (v if k == "pair_off" else v.cpu().numpy()) for k, v in out.items()}


def _close(got, want, tol):
    """Largest difference where both are finite; NaN must sit in the same places."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


def _compare(got, want, what):
    ove = float(np.abs(got["overlaps"] - want["overlaps"]).max()) if len(want["overlaps"]) else 0.0
    pe, ape = _close(got["precision"], want["precision"], 0), _close(got["ap"], want["ap"], 0)
    ae, aape = _close(got["aos"], want["aos"], 0), _close(got["aos_ap"], want["aos_ap"], 0)
    print("%s: %d pairs, overlaps worst %.3e; thresholds per list %s; precision worst %.3e, ap %.3e, aos %.3e, aos_ap %.3e; ap %s" %
          (what, len(want["overlaps"]), ove, want["num_thresholds"].tolist(), pe, ape, ae, aape, np.round(got["ap"], 4).tolist()))
    assert ove < 5e-5, what                                       # the project's bar for the fp32 clip against the fp64 python
    for k in ("n_gt", "num_thresholds", "tp", "fp", "fn"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got["thresholds"], want["thresholds"]), what          # float32 scores, promoted: exact
    assert pe < 1e-12 and ape < 1e-12, what                       # one fp64 division of integer counts; eleven of them summed in order
    assert ae < 1e-9 and aape < 1e-9, what                        # at most 1e4 fp64 terms, each a few ulp (cos of another libm)


@pytest.mark.parametrize("name", scenes.NAMES)
def test_scene_matches_the_referee(name):
    sc, want = scenes.scene(name)
    got = _run(sc)
    _compare(got, want, name)
    again = _run(sc)                                              # two runs: the same bits, the orientation sums included
    for k in KEYS:
        assert np.array_equal(got[k], again[k], equal_nan=k not in ("pair_off",)), (name, k)
    nd, ng = np.diff(sc["det_off"]), np.diff(sc["gt_off"])
    car = [(0 * 3 + 0) * 3 + d for d in range(3)] + [(1 * 3 + 0) * 3 + d for d in range(3)] + [(2 * 3 + 0) * 3 + d for d in range(3)]
    if name == "mixed":
        assert nd[0] == 0 and ng[1] == 0 and (sc["gt_type"][sc["gt_off"][2]:sc["gt_off"][3]] == ref.DONTCARE).all()
        assert nd[3] == 65 and (nd[4], ng[4]) == (130, 70)
        assert len(np.unique(sc["det"][:, 12])) < len(sc["det"]) // 2          # equal scores are common
        assert (got["num_thresholds"] > 0).sum() >= 20 and np.isfinite(got["ap"]).all() and (got["ap"] > 0).any()
        assert (got["fp"] > 0).any() and (got["fn"] > 0).any() and np.isfinite(got["aos_ap"]).all()
    if name == "single":
        assert len(nd) == 1
    if name == "no_cyclist":
        assert (sc["gt_type"] == ref.CYCLIST).any() and not (sc["det_class"] == 2).any()
        assert np.isnan(got["ap"][:, 2]).all() and np.isnan(got["precision"][:, 2]).all() and np.isnan(got["aos"][2]).all()
        assert np.isfinite(got["ap"][:, :2]).all() and (got["n_gt"].reshape(3, 3, 3)[:, 2] > 0).any()
    if name == "alpha10":
        assert (sc["det"][:, 0] == -10).sum() == 1 and np.isnan(got["aos"]).all() and np.isnan(got["aos_ap"]).all()
        assert np.isfinite(got["ap"]).all()
    if name.startswith("tp"):
        n = int(name[2:])
        assert all(len(want["tp_scores"][k]) == n for k in car) and (got["n_gt"][car] == n).all()
        assert (got["num_thresholds"][car] == min(n, 41)).all()
        # every detection is right, so the precision is 1 at every threshold there is: AP = 100 / 11 per sample point 0, 4, .. below T
        assert np.abs(got["ap"][:, 0] - 100.0 / 11 * len(range(0, min(n, 41), 4))).max() < 1e-9


def test_overlaps_at_60_m_depth():
    rng = np.random.default_rng(31)
    gt = [scenes.label(rng, ref.CAR, depth=60.0 + k, x=20.0 - 5 * k) for k in range(6)] + [scenes.label(rng, ref.DONTCARE, depth=61.0, x=0.0)]
    det = [scenes.detection(rng, g, j, 1.0) for g in gt for j in (0.01, 0.05, 0.2)]
    sc = scenes.pack([(np.asarray(det), np.zeros(len(det), np.int32), np.asarray(gt), np.asarray([0] * 6 + [5], np.int32))])
    want = ref.frame_overlaps(sc["det"].astype(np.float64), sc["gt"].astype(np.float64), sc["gt_type"]).reshape(-1, 3)
    got = _run(sc)["overlaps"]
    err = np.abs(got - want).max(0)
    print("60 m: %d pairs, %d with a ground overlap; worst image %.3e ground %.3e 3-D %.3e" % (len(want), (want[:, 1] > 0).sum(), *err))
    assert (want[:, 1] > 0.5).sum() >= 6 and (want[:, 2] > 0).sum() >= 6 and err.max() < 5e-5


def test_label_rows_match_the_golden_file_and_the_restatement():
    from frustum_convnet_amd import evaluate
    g = np.load(ref.GOLDEN)
    m = len(g["alpha"])
    rng = np.random.default_rng(5)
    # the reference's compute_alpha on (x, z, ry) triples (z = 0, x = 0 and both among them), and on its own label rows
    lab = g["label"]                                                            # h, w, l, tx, ty, tz, ry
    dets = np.concatenate([np.stack([g["xz"][:, 0], np.ones(m), g["xz"][:, 1], np.full(m, 3.9), np.full(m, 1.6), np.full(m, 1.5), g["ry"],
                                     np.linspace(0, 1, m)], 1),
                           np.concatenate([lab[:, 3:6], lab[:, [2, 1, 0]], lab[:, 6:7], np.ones((m, 1))], 1)]).astype(np.float32)
    dets[5, 3], dets[6, 4], dets[7, 5], dets[8, 5] = 0.009, 0.0, -1.0, 0.011      # l, w, h too small: dropped; h = 0.011 stays
    boxes = rng.uniform(0, 1000, (9, 4)).astype(np.float32)
    rows = rng.permutation(2 * m).astype(np.int64)
    row_box = rng.integers(0, 9, 2 * m)
    table, ok = evaluate.kitti_label_rows(_dev(dets), _dev(rows), _dev(boxes), row_box)
    torch.cuda.synchronize()
    assert table.is_cuda and ok.is_cuda and table.dtype == torch.float32 and ok.dtype == torch.int32 and tuple(table.shape) == (2 * m, 13)
    table, ok = table.cpu().numpy(), ok.cpu().numpy()
    want, wok = ref.label_rows(dets, rows, boxes, row_box)
    gold = np.concatenate([g["alpha"], g["label_alpha"]])[rows]
    e_gold, e_ref, e_copy = np.abs(table[:, 0] - gold).max(), np.abs(table[:, 0] - want[:, 0]).max(), np.abs(table[:, 1:] - want[:, 1:]).max()
    print("label rows: alpha worst %.3e against the reference's recorded values, %.3e against the restatement; copied columns %.3e" %
          (e_gold, e_ref, e_copy))
    assert e_gold < 1e-6 and e_ref < 1e-6 and e_copy < 1e-6
    assert np.array_equal(ok != 0, wok) and (~wok).sum() == 3 and wok[np.nonzero(rows == 8)[0][0]]
    # rows = None: every row in order; an index outside dets / boxes2d: a NaN row with ok = 0, nothing dereferenced
    t2, ok2 = evaluate.kitti_label_rows(_dev(dets), None, _dev(boxes), np.zeros(2 * m, np.int64))
    assert np.abs(t2.cpu().numpy()[:, 0] - np.concatenate([g["alpha"], g["label_alpha"]])).max() < 1e-6
    t3, ok3 = evaluate.kitti_label_rows(_dev(dets), [0, -1, 2 * m, 1], _dev(boxes), [0, 0, 0, 9])
    t3, ok3 = t3.cpu().numpy(), ok3.cpu().numpy()
    assert ok3.tolist() == [1, 0, 0, 0] and np.isnan(t3[1:]).all() and np.isfinite(t3[0]).all()
    with pytest.raises(ValueError):
        evaluate.kitti_label_rows(_dev(dets), rows, _dev(boxes), row_box[:-1])


def _raw(sc, guard=3):
    """Device inputs of the raw entries and poisoned outputs with `guard` extra elements behind each."""
    nd, ng, F = len(sc["det"]), len(sc["gt"]), len(sc["det_off"]) - 1
    poff = np.concatenate([[0], np.cumsum(np.diff(sc["det_off"]) * np.diff(sc["gt_off"]))])
    t = {"doff": _dev(sc["det_off"].astype(np.int32)), "goff": _dev(sc["gt_off"].astype(np.int32)), "poff": _dev(poff.astype(np.int32)),
         "det": _dev(sc["det"]), "cls": _dev(sc["det_class"]), "gt": _dev(sc["gt"]), "typ": _dev(sc["gt_type"])}
    full = lambda n, dt: torch.full((n + guard,), -7, dtype=dt, device="cuda")
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    o = {"ov": full(int(poff[-1]) * 3, f32), "flags": full(10, i32), "assigned": full(27 * nd * 2, i32), "tp_score": full(27 * ng, f32),
         "tp_count": full(27, i32), "n_gt": full(27, i32), "sorted": full(27 * ng, f32), "thr": full(27 * 41, f64), "nthr": full(27, i32),
         "counts": full(3 * 27 * 41, i32), "sim": full(F * 9 * 41, f64), "prec": full(27 * 41, f64), "aos": full(9 * 41, f64),
         "ap": full(27, f64), "aos_ap": full(9, f64)}
    return t, o, (nd, ng, F, int(poff[-1]))


def _calls(t, o, dims, s):
    nd, ng, F, npairs = dims
    scene = lambda: [_p(t["doff"]), _p(t["goff"]), _p(t["poff"]), F, _p(t["det"]), _p(t["cls"]), nd, _p(t["gt"]), _p(t["typ"]), ng, _p(o["ov"]), npairs]
    return {"fcn_kitti_overlaps": lambda: scene() + [_p(o["flags"]), s],
            "fcn_kitti_pass_a": lambda: scene() + [7, _p(o["assigned"]), _p(o["tp_score"]), _p(o["tp_count"]), _p(o["n_gt"]), s],
            "fcn_kitti_thresholds": lambda: [_p(o["tp_score"]), _p(o["tp_count"]), _p(o["n_gt"]), ng, _p(o["sorted"]), _p(o["thr"]), _p(o["nthr"]), s],
            "fcn_kitti_pass_b": lambda: scene() + [7, _p(o["thr"]), _p(o["nthr"]), _p(o["assigned"]), _p(o["counts"]), _p(o["sim"]), s],
            "fcn_kitti_curves": lambda: [_p(o["counts"]), _p(o["nthr"]), _p(o["sim"]), F, _p(o["flags"]), 7, _p(o["prec"]), _p(o["aos"]),
                                         _p(o["ap"]), _p(o["aos_ap"]), s]}


ORDER = ("fcn_kitti_overlaps", "fcn_kitti_pass_a", "fcn_kitti_thresholds", "fcn_kitti_pass_b", "fcn_kitti_curves")
# argument positions whose NULL is refused / whose negative count is refused (the scene's first twelve arguments are shared)
NULLS = {"fcn_kitti_overlaps": (0, 1, 2, 4, 5, 7, 8, 10, 12), "fcn_kitti_pass_a": (0, 1, 2, 4, 5, 7, 8, 10, 13, 14, 15, 16),
         "fcn_kitti_thresholds": (0, 1, 2, 4, 5, 6), "fcn_kitti_pass_b": (0, 1, 2, 4, 5, 7, 8, 10, 13, 14, 15, 16, 17),
         "fcn_kitti_curves": (0, 1, 2, 4, 6, 7, 8, 9)}
NEGS = {"fcn_kitti_overlaps": (3, 6, 9, 11), "fcn_kitti_pass_a": (3, 6, 9, 11), "fcn_kitti_thresholds": (3,), "fcn_kitti_pass_b": (3, 6, 9, 11),
        "fcn_kitti_curves": (3,)}


def test_raw_entries_poisoned_outputs_and_refusals():
    from frustum_convnet_amd import _native, evaluate
    sc, want = scenes.scene("single")
    L, s = _native.lib(), _native.current_stream()
    t, o, dims = _raw(sc)
    nd, ng, F, npairs = dims
    calls = _calls(t, o, dims, s)
    # every refusal first: nothing is written by any of them
    for name in ORDER:
        for i in NULLS[name]:
            bad = calls[name](); bad[i] = None
            assert getattr(L, name)(*bad) == BADARG, (name, i)
        for i in NEGS[name]:
            bad = calls[name](); bad[i] = -1
            assert getattr(L, name)(*bad) == BADARG, (name, i)
    lr = lambda: [_p(t["det"]), 1, None, 1, _p(t["gt"]), 1, _p(t["cls"]), _p(o["ov"]), _p(o["flags"]), s]       # (any device pointers)
    for i in (0, 4, 6, 7, 8):
        bad = lr(); bad[i] = None
        assert L.fcn_kitti_label_rows(*bad) == BADARG, i
    for i, v in ((1, -1), (3, -1), (5, -1), (3, 2)):                          # (3, 2): rows = NULL asks for more rows than dets has
        bad = lr(); bad[i] = v
        assert L.fcn_kitti_label_rows(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in o.values())
    # accepted, in order: the referee's results, every element written, the guards behind them untouched
    for name in ORDER:
        assert getattr(L, name)(*calls[name]()) == 0, name
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in o.items()}
    assert all((h[k][-3:] == -7).all() for k in h)
    got = {"overlaps": h["ov"][:-3].reshape(-1, 3), "precision": h["prec"][:-3].reshape(3, 3, 3, 41), "aos": h["aos"][:-3].reshape(3, 3, 41),
           "ap": h["ap"][:-3].reshape(3, 3, 3), "aos_ap": h["aos_ap"][:-3].reshape(3, 3), "thresholds": h["thr"][:-3].reshape(27, 41),
           "num_thresholds": h["nthr"][:-3], "n_gt": h["n_gt"][:-3], "tp": h["counts"][:-3].reshape(3, 27, 41)[0],
           "fp": h["counts"][:-3].reshape(3, 27, 41)[1], "fn": h["counts"][:-3].reshape(3, 27, 41)[2]}
    _compare(got, want, "raw entries")
    assert (h["assigned"][:-3] != -7).all() and (h["flags"][:10] != -7).all()
    # empty problems: no frame touches nothing but the counters the entries zero themselves
    t2, o2, _ = _raw(sc)
    c2 = _calls(t2, o2, (nd, ng, 0, npairs), s)
    for name in ("fcn_kitti_overlaps", "fcn_kitti_pass_a", "fcn_kitti_pass_b"):
        assert getattr(L, name)(*c2[name]()) == 0, name
    torch.cuda.synchronize()
    h2 = {k: v.cpu().numpy() for k, v in o2.items()}
    assert all((h2[k] == -7).all() for k in ("ov", "assigned", "tp_score", "sim"))
    assert (h2["flags"][:10] == 0).all() and (h2["tp_count"][:27] == 0).all() and (h2["counts"][:-3] == 0).all()
    assert all((h2[k][-3:] == -7).all() for k in h2)
    # offsets that run past the buffers are clamped to them: nothing is read or written outside nd / ng / npairs
    t3, o3, _ = _raw(sc)
    far = lambda a, n: _dev(np.concatenate([a[:-1], [n + 1000]]).astype(np.int32))
    t3["doff"], t3["goff"] = far(sc["det_off"], nd), far(sc["gt_off"], ng)
    c3 = _calls(t3, o3, dims, s)
    for name in ORDER:
        assert getattr(L, name)(*c3[name]()) == 0, name
    t3["poff"] = _dev(np.asarray([npairs + 1000, npairs + 2000], np.int32))      # pairs that do not fit: the frame counts as empty
    for name in ORDER:
        assert getattr(L, name)(*_calls(t3, o3, dims, s)[name]()) == 0, name
    torch.cuda.synchronize()
    assert all((v.cpu().numpy()[-3:] == -7).all() for v in o3.values())
    assert (o3["n_gt"].cpu().numpy()[:27] == 0).all() and (o3["counts"].cpu().numpy()[:-3] == 0).all()
    # the host side refuses what it can see
    good = [_dev(sc["det"]), _dev(sc["det_class"]), sc["det_off"], _dev(sc["gt"]), _dev(sc["gt_type"]), sc["gt_off"]]
    for k, v in ((2, sc["det_off"] + 1), (2, sc["det_off"][::-1].copy()), (2, np.asarray([0, nd - 1])), (5, np.asarray([0, ng + 1])),
                 (5, np.asarray([0, 1, ng])), (1, sc["det_class"][:-1]), (4, sc["gt_type"][:-1]), (0, _dev(sc["det"][:, :12])),
                 (3, _dev(sc["gt"][:, :13]))):
        bad = list(good); bad[k] = v
        with pytest.raises(ValueError):
            evaluate.kitti_eval(*bad)
    for classes in ((), (3,), (-1, 0)):
        with pytest.raises(ValueError):
            evaluate.kitti_eval(*good, classes=classes)


def test_cpu_tensors_raise():
    """No CPU fallback in any of the three functions."""
    from frustum_convnet_amd import evaluate
    sc, _ = scenes.scene("single")
    cpu = lambda k: torch.from_numpy(sc[k])
    with pytest.raises(RuntimeError):
        evaluate.kitti_eval(cpu("det"), cpu("det_class"), sc["det_off"], cpu("gt"), cpu("gt_type"), sc["gt_off"])
    with pytest.raises(RuntimeError):
        evaluate.kitti_label_rows(torch.zeros((4, 8)), None, torch.zeros((1, 4)), [0, 0, 0, 0])
    keep, cnt = torch.zeros((1, 2), dtype=torch.int32), torch.ones((1,), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        evaluate.kitti_results((torch.zeros((4, 8)), None, keep, cnt), torch.zeros((1, 4)), [0], ["Car"])


def test_classes_argument_leaves_the_others_out():
    sc, want = scenes.scene("single")
    got = _run(sc, classes=(1,))
    assert np.isnan(got["ap"][:, [0, 2]]).all() and np.isnan(got["aos"][[0, 2]]).all()
    assert _close(got["ap"][:, 1], want["ap"][:, 1], 0) < 1e-12 and _close(got["aos_ap"][1], want["aos_ap"][1], 0) < 1e-9
    k = np.arange(27).reshape(3, 3, 3)
    assert (got["num_thresholds"][k[:, [0, 2]]] == 0).all() and np.array_equal(got["tp"][k[:, 1]], want["tp"][k[:, 1]])


def _fake_detect_frames():
    """A hand-built dict of the shape TwoStageDetector.detect_frames returns: 5 boxes of which boxes 4, 0, 3 survive ('kept'), 2
    rows per first-stage frustum, second-stage units refining first-stage rows 1, 4, 5 (frustums 0, 2, 2 = boxes 4, 3, 3), 3 rows
    per second-stage unit, two NMS groups keeping rows (7, 2) and (4,)."""
    rng = np.random.default_rng(9)
    dets2 = np.concatenate([rng.normal(0, 5, (9, 3)) + [0, 1, 20], rng.uniform(0.5, 4, (9, 3)), rng.uniform(-3, 3, (9, 1)), rng.uniform(0, 2, (9, 1))], 1)
    keep = np.asarray([[7, 2, -1], [4, -1, -1]], dtype=np.int32)
    res = {"dets": _dev(dets2.astype(np.float32)), "valid": None, "keep": _dev(keep), "cnt": _dev(np.asarray([2, 1], np.int32)),
           "stage1_row": np.asarray([1, 4, 5]), "stage1": (torch.zeros((6, 8), device="cuda"), None, None, None), "kept": np.asarray([4, 0, 3])}
    boxes = rng.uniform(0, 900, (5, 4)).astype(np.float32)
    return res, dets2.astype(np.float32), boxes, [1, 0, 0, 0, 2], ["Car", "Car", "Car", "Pedestrian", "cyclist"]


def test_kitti_results_on_a_hand_built_detect_frames_dict():
    from frustum_convnet_amd import evaluate
    res, dets2, boxes, frame, types = _fake_detect_frames()
    out = evaluate.kitti_results(res, _dev(boxes), frame, types, num_frames=4)
    torch.cuda.synchronize()
    # rows 7, 2 -> units 2, 0 -> boxes 3, 4 -> frames 0, 2; row 4 -> unit 1 -> box 3 -> frame 0.  By frame (stable): 7, 4, 2
    assert out["rows"].tolist() == [7, 4, 2] and out["row_box"].tolist() == [3, 3, 4] and out["det_off"].tolist() == [0, 2, 2, 3, 3]
    assert out["det_class"].cpu().tolist() == [1, 1, 2] and out["ok"].cpu().tolist() == [1, 1, 1]
    want, _ = ref.label_rows(dets2, [7, 4, 2], boxes, [3, 3, 4])
    assert np.abs(out["det_table"].cpu().numpy() - want).max() < 1e-6
    # the tuple of a single-stage PointNetDet.detect over all boxes in order: 5 units of ... rows do not divide -> refused; 9 = 3 x 3
    with pytest.raises(ValueError):
        evaluate.kitti_results((res["dets"], None, res["keep"], res["cnt"]), _dev(boxes), frame, types)
    one = evaluate.kitti_results((res["dets"], None, res["keep"], res["cnt"]), _dev(boxes[:3]), frame[:3], ["Car", "Van", "Pedestrian"])
    # rows 7, 2, 4 -> boxes 2, 0, 1 -> frames 0, 1, 0: by frame 7, 4, 2; a Van is no evaluated class
    assert one["rows"].tolist() == [7, 4, 2] and one["row_box"].tolist() == [2, 1, 0] and one["det_off"].tolist() == [0, 2, 3]
    assert one["det_class"].cpu().tolist() == [1, -1, 0]
    # nothing survived
    none = evaluate.kitti_results({"dets": None, "valid": None, "keep": None, "cnt": None, "stage1_row": np.zeros(0, np.int64), "stage1": None,
                                   "kept": np.zeros(0, np.int64)}, _dev(boxes), frame, types)
    assert tuple(none["det_table"].shape) == (0, 13) and none["det_off"].tolist() == [0, 0, 0, 0]


def test_two_stage_model_end_to_end_equals_the_referee_on_the_same_kept_rows():
    """A tiny car first stage and refine second stage (N = 512, hash-initialised) through TwoStageDetector.detect_frames ->
    kitti_results -> kitti_eval; the referee is fed the kept rows the device table holds.  Labels: a copy of every second kept
    detection (overlap 1 in the three metrics) and one label far from everything."""
    from helpers import load_golden
    from test_gpu_model import _model
    from test_gpu_frustum import _golden
    from frustum_convnet_amd import cascade, evaluate, inputs
    g = _golden()
    g1, g2 = load_golden("car_b4_n512"), load_golden("refine_b4_n512")
    m1 = _model(g1).eval()
    ib = inputs.InputBuilder(int(g1["meta_npoint"]))
    m2 = _model(g2).eval()
    rb = inputs.RefineInputBuilder(int(g2["meta_npoint"]))
    rng = np.random.RandomState(9)
    lengths = (6000, 5000)
    xyz = [np.stack([rng.uniform(3, 45, n), rng.uniform(-12, 12, n), rng.uniform(-2.0, 0.5, n), rng.uniform(0, 1, n)], 1) for n in lengths]
    fpts = _dev(np.concatenate(xyz, 0).astype(np.float32))
    foff = _dev(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
    cal = {k: _dev(g[k]) for k in ("P", "V2C", "R0")}
    boxes = np.asarray([[300.0, 150.0, 520.0, 300.0], [700.0, 160.0, 900.0, 280.0], [500.0, 120.0, 760.0, 330.0], [100.0, 150.0, 330.0, 290.0]])
    bframe, types = np.asarray([0, 0, 1, 1], dtype=np.int32), ["Car", "Pedestrian", "Car", "Cyclist"]
    np.random.seed(11)
    two = cascade.TwoStageDetector(m1, m2, rb, input_builder=ib)
    res = two.detect_frames(fpts, foff, cal, g["img_wh"], boxes, bframe, types, np.asarray([0.9, 0.8, 0.6, 0.5]),
                            unit_group=np.arange(4, dtype=np.int32), num_groups=4, method="nms", thresh=0.1, top_k=6)
    assert res["dets"] is not None and int(res["cnt"].clamp(min=0).sum()) > 0
    out = evaluate.kitti_results(res, _dev(boxes.astype(np.float32)), bframe, types, num_frames=2)
    torch.cuda.synchronize()
    det, cls, doff = out["det_table"].cpu().numpy(), out["det_class"].cpu().numpy(), out["det_off"]
    n = len(det)
    assert n == int(res["cnt"].clamp(min=0).sum()) and doff[-1] == n and (out["ok"].cpu().numpy() == 1).all()
    want_rows, _ = ref.label_rows(res["dets"].cpu().numpy(), out["rows"], boxes, out["row_box"])
    assert np.abs(det - want_rows).max() < 1e-5 * max(1.0, np.abs(want_rows).max())
    gt, gtt, goff = [], [], [0]
    for f in range(2):
        for j in range(doff[f], doff[f + 1], 2):
            d = det[j].astype(np.float64)
            gt.append([0.0, 0.0, d[0] + 0.25, d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]])
            gtt.append(int(cls[j]) if cls[j] >= 0 else ref.OTHER)
        gt.append([0.0, 0.0, 0.0, 5.0, 5.0, 105.0, 95.0, 1.5, 1.6, 3.9, -40.0, 1.6, 70.0, 0.3])
        gtt.append(ref.CAR)
        goff.append(len(gt))
    sc = {"det": det, "det_class": cls, "det_off": doff, "gt": np.asarray(gt, np.float32), "gt_type": np.asarray(gtt, np.int32),
          "gt_off": np.asarray(goff, np.int64)}
    for f in range(2):
        ov = ref.frame_overlaps(det[doff[f]:doff[f + 1]].astype(np.float64), sc["gt"][goff[f]:goff[f + 1]].astype(np.float64), sc["gt_type"][goff[f]:goff[f + 1]])
        assert scenes.knife_edge_ok(ov) and scenes.heights_ok(det, 2, 4), "the model's detections leave the comparison no margin"
    want = ref.evaluate(det, cls, doff, sc["gt"], sc["gt_type"], sc["gt_off"])
    got = _run(sc)
    _compare(got, want, "end to end")
    print("end to end: %d kept detections of classes %s" % (n, cls.tolist()))
    assert got["tp"].max() >= 1 and (got["n_gt"] >= 1).any()
