"""TEST INFRASTRUCTURE ONLY: the seeded scenes of the KITTI evaluation tests (tests/test_kitti_eval_referee.py on the CPU,
tests/test_gpu_kitti_eval.py / tests/test_emu_kitti_eval.py against the kernels).  Every scene is float32 data; the referee
(tests/kitti_eval_ref.py) promotes it to fp64 and its answer is computed once per process and shared.

THE KNIFE-EDGE CONDITION (checked while drawing, asserted again by the referee test; MARGIN = 1e-3 against the clip core's 5e-5
bar, the margin tests/test_gpu_det_eval.py uses):
  * every overlap the protocol compares lies more than MARGIN from both MIN_OVERLAP values (0.5 and 0.7);
  * the overlaps above (0.5 - MARGIN) that the detections of a frame have with ONE label differ pairwise by more than MARGIN
    (stricter than "the two best": whatever is already assigned, the best of the rest is decided);
  * every image height lies more than HEIGHT_MARGIN from 25 and 40, every truncation off its limits by construction.
A detection that violates it is redrawn, at most 200 times, then the draw raises; nothing is left out of a comparison."""
import functools

import numpy as np

import kitti_eval_ref as ref

MARGIN, HEIGHT_MARGIN = 1e-3, 0.005       # (a float32 pixel coordinate below 1242 is exact to 6e-5)
SIZE = {ref.CAR: (1.5, 1.6, 3.9), ref.VAN: (2.0, 1.9, 5.0), ref.PEDESTRIAN: (1.75, 0.6, 0.8), ref.PERSON_SITTING: (1.2, 0.6, 0.8),
        ref.CYCLIST: (1.7, 0.6, 1.8), ref.DONTCARE: (1.5, 1.6, 3.9), ref.OTHER: (3.0, 2.5, 8.0)}      # h, w, l
f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)


def _height(rng):
    lo, hi = [(12.0, 24.0), (26.0, 39.0), (41.0, 160.0)][rng.choice(3, p=[0.15, 0.2, 0.65])]
    return rng.uniform(lo, hi)


def label(rng, typ, height=None, occ=None, trunc=None, depth=None, x=None):
    """One label row (14) of type typ: an image box of the given height somewhere in a 1242 x 375 image, a 3-D box of the type's size."""
    h2 = _height(rng) if height is None else height
    w2 = h2 * rng.uniform(0.6, 2.2)
    x1, y1 = rng.uniform(0, 1242 - w2), rng.uniform(0, 375 - min(h2, 370))
    h, w, l = np.asarray(SIZE[typ]) * rng.uniform(0.85, 1.15, 3)
    tz = rng.uniform(5.0, 62.0) if depth is None else depth
    tx = rng.uniform(-0.5, 0.5) * tz if x is None else x
    return f32([rng.choice([0.0, 0.1, 0.2, 0.4, 0.6]) if trunc is None else trunc, rng.integers(0, 4) if occ is None else occ,
                rng.uniform(-np.pi, np.pi), x1, y1, x1 + w2, y1 + h2, h, w, l, tx, rng.uniform(1.2, 2.0), tz, rng.uniform(-np.pi, np.pi)])


def detection(rng, g, jitter, score, alpha=None):
    """A detection row (13) about label row g: the image box and the 3-D box jittered by `jitter` (relative)."""
    w2, h2 = g[5] - g[3], g[6] - g[4]
    x1, y1 = g[3] + rng.normal(0, jitter) * w2, g[4] + rng.normal(0, jitter) * h2
    x2, y2 = g[5] + rng.normal(0, jitter) * w2, g[6] + rng.normal(0, jitter) * h2
    h, w, l = g[7:10] * rng.uniform(1 - jitter, 1 + jitter, 3)
    tx, ty, tz = g[10] + rng.normal(0, jitter) * g[9], g[11] + rng.normal(0, jitter) * g[7], g[12] + rng.normal(0, jitter) * g[9]
    return f32([g[2] + rng.normal(0, 0.3) if alpha is None else alpha, x1, y1, x2, y2, h, w, l, tx, ty, tz, g[13] + rng.normal(0, jitter), score])


def heights_ok(rows, c1, c2):
    h = np.abs(np.asarray(rows)[:, c2] - np.asarray(rows)[:, c1]) if len(rows) else np.zeros(0)
    return bool(((np.abs(h - 25) > HEIGHT_MARGIN) & (np.abs(h - 40) > HEIGHT_MARGIN)).all())


def knife_edge_ok(ov):
    """ov (nd_f, ng_f, 3) of ref.frame_overlaps: the condition of this module's head on one frame."""
    if ov.size == 0:
        return True
    if (np.abs(ov - 0.5) <= MARGIN).any() or (np.abs(ov - 0.7) <= MARGIN).any():
        return False
    for i in range(ov.shape[1]):
        for m in range(3):
            v = np.sort(ov[:, i, m][ov[:, i, m] > 0.5 - MARGIN])
            if len(v) > 1 and (np.diff(v) <= MARGIN).any():
                return False
    return True


def frame(rng, types, n_dets, classes=(0, 1, 2), scores=None, near=0.7):
    """A frame: one label per entry of `types`, n_dets detections -- with probability `near` about a label that is no DontCare
    (its class, or another one now and then), else anywhere.  scores: the values to draw scores from (default: a coarse grid, so
    equal scores are common).  -> det (n,13), det_class (n), gt (m,14), gt_type (m), fp64 holding float32 values."""
    gt = [label(rng, t) for t in types]
    gt_type = np.asarray(types, dtype=np.int32).reshape(-1)
    own = {ref.CAR: 0, ref.VAN: 0, ref.PEDESTRIAN: 1, ref.PERSON_SITTING: 1, ref.CYCLIST: 2}
    grid = np.round(np.arange(0.05, 2.0, 0.05), 2) if scores is None else np.asarray(scores)
    det, det_class = [], []
    ov = np.zeros((0, len(gt), 3))
    for _ in range(n_dets):
        for _try in range(200):
            pick = [i for i, t in enumerate(types) if t != ref.DONTCARE]
            if pick and rng.uniform() < near:
                i = pick[rng.integers(len(pick))]
                d = detection(rng, gt[i], rng.choice([0.02, 0.04, 0.06, 0.15]), rng.choice(grid))
                c = own.get(types[i], rng.choice(classes)) if rng.uniform() < 0.85 else rng.choice(classes)
            else:
                t = [ref.CAR, ref.PEDESTRIAN, ref.CYCLIST][rng.integers(3)]
                d = detection(rng, label(rng, t), 0.0, rng.choice(grid))
                c = own[t]
            if types and ref.DONTCARE in types and rng.uniform() < 0.25:        # now and then inside a DontCare area (image)
                k = types.index(ref.DONTCARE)
                cx, cy = rng.uniform(gt[k][3], gt[k][5]), rng.uniform(gt[k][4], gt[k][6])
                d[1:5] = f32([cx - 15, cy - rng.choice([15.0, 25.0]), cx + 15, cy + rng.choice([15.0, 25.0])])
            row = np.asarray([ref.pair_overlaps(d, g, 0 if t == ref.DONTCARE else -1) for g, t in zip(gt, types)]).reshape(1, len(gt), 3)
            if heights_ok([d], 2, 4) and knife_edge_ok(np.concatenate([ov, row])):
                break
        else:
            raise RuntimeError("re-draw did not terminate")
        ov = np.concatenate([ov, row])
        det.append(d)
        det_class.append(c if c in classes else -1)
    assert heights_ok(gt, 4, 6)                                             # (_height keeps the labels off the limits)
    return (np.asarray(det).reshape(-1, 13), np.asarray(det_class, dtype=np.int32), np.asarray(gt).reshape(-1, 14), gt_type)


def pack(frames):
    """frames: (det, det_class, gt, gt_type) each -> the CSR scene as float32 / int32 / int64 arrays."""
    off = lambda k: np.concatenate([[0], np.cumsum([len(f[k]) for f in frames])]).astype(np.int64)
    cat = lambda k, w, dt: np.concatenate([np.asarray(f[k]).reshape(-1, w) for f in frames] + [np.zeros((0, w))]).astype(dt)
    return {"det": cat(0, 13, np.float32), "det_class": cat(1, 1, np.int32).reshape(-1), "det_off": off(0),
            "gt": cat(2, 14, np.float32), "gt_type": cat(3, 1, np.int32).reshape(-1), "gt_off": off(2)}


ALL_TYPES = [ref.CAR, ref.PEDESTRIAN, ref.CYCLIST, ref.VAN, ref.PERSON_SITTING, ref.DONTCARE, ref.OTHER]


def _mixed_frames(rng, big=True):
    t = lambda n: [ALL_TYPES[i] for i in rng.choice(7, n, p=[0.3, 0.2, 0.15, 0.1, 0.1, 0.1, 0.05])]
    frames = [frame(rng, t(3), 0),                                      # no detection
              frame(rng, [], 4),                                        # no label
              frame(rng, [ref.DONTCARE, ref.DONTCARE], 3)]              # only DontCare
    if big:
        frames += [frame(rng, t(9), 65),                                # past a 64-bit mask / one wave
                   frame(rng, t(70), 130)]                              # past two waves, 70 labels
    frames += [frame(rng, t(8), 10, near=0.85) for _ in range(12 if big else 6)]
    return frames


def _tp_frames(rng, n, typ=ref.CAR):
    """n easy labels of type typ (a class), 8 to a frame and 12 m apart, each under one close detection with a score of its own: n
    true positives in every list of the class."""
    frames, score = [], rng.permutation(n).astype(np.float64) / n + 0.2
    for f0 in range(0, n, 8):
        gt, det = [], []
        for k in range(f0, min(n, f0 + 8)):
            g = label(rng, typ, height=rng.uniform(50, 120), occ=0, trunc=0.0, depth=8.0 + 12.0 * ((k - f0) // 2), x=-8.0 + 16.0 * (k % 2))
            g[3:7] = f32([20 + 150 * (k - f0), 100, 20 + 150 * (k - f0) + 100, 100 + g[6] - g[4]])   # image boxes side by side
            for _try in range(200):
                d = detection(rng, g, 0.02, score[k])
                row = np.asarray(ref.pair_overlaps(d, g, -1)).reshape(1, 1, 3)
                if heights_ok([d], 2, 4) and knife_edge_ok(row) and (row > 0.7).all():
                    break
            else:
                raise RuntimeError("re-draw did not terminate")
            gt.append(g); det.append(d)
        frames.append((np.asarray(det), np.full(len(det), typ, np.int32), np.asarray(gt), np.full(len(gt), typ, np.int32)))
    return frames


# ---- hand-built scenes: tests/test_kitti_eval_referee.py derives their answers by hand
def L(typ, x1, y1, x2, y2, slot, occ=0, trunc=0.0, alpha=0.0):
    """A label with the given image box; its 3-D box (1.5 x 1.6 x 3.9, heading 0) stands at tx = 10 * slot, tz = 20."""
    return f32([trunc, occ, alpha, x1, y1, x2, y2, 1.5, 1.6, 3.9, 10.0 * slot, 1.6, 20.0, 0.0])


def D(x1, y1, x2, y2, slot, score, alpha=0.0):
    """A detection with the given image box; its 3-D box is the slot's, 10 % narrower and shorter (nested: ground and 3-D overlap
    0.81 with the label of the same slot, 0 with any other)."""
    return f32([alpha, x1, y1, x2, y2, 1.5, 1.44, 3.51, 10.0 * slot, 1.6, 20.0, 0.0, score])


def _hand(dets, classes, labels, types):
    return (np.asarray(dets).reshape(-1, 13), np.asarray(classes, np.int32), np.asarray(labels).reshape(-1, 14), np.asarray(types, np.int32))


def hand1():
    """One frame.  Labels: g0 Car 60 px; g1 Car 30 px (too small for 'easy'); g2 Van; g3 DontCare; g4 Car 60 px, missed; g5 Car 60 px.
    Detections (all Car): d0 on g0 (0.9, alpha off by pi / 2), d1 on g1 (0.8, 30 px), d2 on the Van (0.7), d3 inside the DontCare
    box in the image but alone in space (0.6), d4 on nothing (0.5), d5 on g5 (0.3)."""
    labels = [L(ref.CAR, 100, 100, 200, 160, 0), L(ref.CAR, 300, 100, 400, 130, 1), L(ref.VAN, 500, 100, 600, 160, 2),
              L(ref.DONTCARE, 700, 100, 800, 200, 3), L(ref.CAR, 900, 100, 1000, 160, 4), L(ref.CAR, 1100, 100, 1200, 160, 5)]
    dets = [D(100, 100, 200, 160, 0, 0.9, alpha=np.pi / 2), D(300, 100, 400, 130, 1, 0.8), D(500, 100, 600, 160, 2, 0.7),
            D(720, 120, 780, 180, 7, 0.6), D(50, 300, 150, 360, 8, 0.5), D(1100, 100, 1200, 160, 5, 0.3)]
    return [_hand(dets, [0] * 6, labels, [ref.CAR, ref.CAR, ref.VAN, ref.DONTCARE, ref.CAR, ref.CAR])]


def hand_trunc():
    """Two frames, each one Car label of 30 px (moderate) under one detection as wide and 25.9 px / 24.99 px high: the detection's
    height is truncated to int32 (25 / 24) before it meets MIN_HEIGHT = 25, so the first counts and the second is 'ignored'."""
    g = L(ref.CAR, 100, 100, 200, 130, 0)
    return [_hand([D(100, 100, 200, 125.9, 0, 0.9)], [0], [g], [ref.CAR]), _hand([D(100, 100, 200, 124.99, 0, 0.8)], [0], [g], [ref.CAR])]


def hand_ignored():
    """One frame, pedestrians.  g0 (60 px) under d0 (39 px: 'ignored' at easy, overlap 0.65, score 0.5, FIRST in the file) and d1 (exact,
    0.9); g1 (60 px) under d2 (exact, 0.1) -- whose low score makes the threshold at which d0 takes part in the search for g0."""
    labels = [L(ref.PEDESTRIAN, 100, 100, 150, 160, 0), L(ref.PEDESTRIAN, 300, 100, 350, 160, 1)]
    dets = [D(100, 100, 150, 139, 0, 0.5), D(100, 100, 150, 160, 0, 0.9), D(300, 100, 350, 160, 1, 0.1)]
    dets[0][5:8] = f32([1.5, 1.5, 3.6])          # (another nested box: the two candidates of g0 differ in the ground metrics too)
    return [_hand(dets, [1, 1, 1], labels, [ref.PEDESTRIAN, ref.PEDESTRIAN])]


def perfect(rng, n=48):
    """n easy labels of every class, each under one close detection of its class and nothing else: AP 100 everywhere."""
    frames = []
    for c in (ref.CAR, ref.PEDESTRIAN, ref.CYCLIST):
        frames += _tp_frames(rng, n, c)
    return frames


HAND = {"hand1": hand1, "hand_trunc": hand_trunc, "hand_ignored": hand_ignored}
NAMES = ("mixed", "single", "no_cyclist", "alpha10", "tp1", "tp40", "tp41", "tp200", "perfect", "hand1", "hand_trunc", "hand_ignored")


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (the packed scene, the referee's answer): computed once per process."""
    rng = np.random.default_rng({"mixed": 11, "single": 12, "no_cyclist": 13, "alpha10": 14}.get(name, 15))
    if name == "mixed":
        frames = _mixed_frames(rng)
    elif name == "single":
        frames = [frame(rng, [ALL_TYPES[i] for i in (0, 0, 1, 2, 3, 5, 1, 4)], 12)]
    elif name == "no_cyclist":                                   # cyclist labels, no cyclist detection: the class is not evaluated
        frames = [frame(rng, [ref.CAR, ref.CYCLIST, ref.PEDESTRIAN, ref.CYCLIST], 8, classes=(0, 1)) for _ in range(3)]
    elif name == "alpha10":
        frames = _mixed_frames(rng, big=False)
        frames[-1][0][2, 0] = -10.0
    elif name in HAND:
        frames = HAND[name]()
    elif name == "perfect":
        frames = perfect(rng)
    else:
        frames = _tp_frames(rng, int(name[2:]))
    sc = pack(frames)
    want = ref.evaluate(sc["det"], sc["det_class"], sc["det_off"], sc["gt"], sc["gt_type"], sc["gt_off"])
    return sc, want
