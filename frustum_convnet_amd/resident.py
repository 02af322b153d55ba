"""The host side the capturable sources share: what FrameTrainSource, SunrgbdTrainSource, FrameDetectSource, SunrgbdDetectSource
(frustum.py), RefineTrainSource and CascadeLink (cascade.py) do ONCE, in their constructors and fill methods -- convert, refuse,
upload, allocate -- stated once.  Plain functions, and the two tables more than one source holds: LabelTable (the label boxes of the
two first-stage training sources) and DetectTable (the 2-D detections of the two inference sources).  A source keeps what is
particular to it: its calibration, its options, its intermediates and its step().  The reading paths (frustum_candidates and its
kin) referee the sources: of this module they use the input parsing alone (intrinsics)."""
import ctypes

import numpy as np
import torch

from . import _native


def host(a):
    """A host array of a tensor or a sequence."""
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def up(a, dev=None):
    """A contiguous host array as a tensor, on dev when given."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dev is None else t.to(dev)


def class_index(who, classes, types):
    """The index into classes of every name of types; an unknown name is refused."""
    cls = [classes.index(t) if t in classes else -1 for t in types]
    if cls and min(cls) < 0:
        raise ValueError("%s: type %r is not one of %r" % (who, types[cls.index(-1)], tuple(classes)))
    return cls


def need_device_builder(builder):
    if builder.device.type != "cuda":
        raise RuntimeError("frustum_convnet_amd: input construction is a HIP kernel (MI355X only); no CPU fallback")


def held(who, t, name="frame_points", shape="(n >= 1, >= 3)", rule=lambda t: t.shape[0] >= 1):
    """Refuses a tensor a source HOLDS instead of copying unless it can be handed to a kernel as it is; rule: what its shape has
    to satisfy beyond being 2-D."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and rule(t)
            and not t.requires_grad):
        raise ValueError("%s: %s must be a contiguous %s float32 device tensor (it is held, not copied)" % (who, name, shape))


def intrinsics(who, K, Rtilt, F, dev):
    """K and Rtilt of F SUN-RGBD frames as two (F, 9) float64 device tensors."""
    cal = []
    for name, m in (("K", K), ("Rtilt", Rtilt)):
        t = torch.as_tensor(m).to(device=dev, dtype=torch.float64).contiguous()
        if t.numel() != F * 9:
            raise ValueError("%s: %s must hold %d x 9 numbers, got %s" % (who, name, F, tuple(t.shape)))
        cal.append(t.view(F, 9))
    return cal


def limits(entry, n):
    """The n ints a fcn_*_limits entry point writes."""
    v = [ctypes.c_int(0) for _ in range(n)]
    _native.check(getattr(_native.lib(), entry)(*(ctypes.byref(x) for x in v)), entry)
    return tuple(x.value for x in v)


def spare_corners(dev):
    """(24,) float64: the corners of the unit box at the origin, in the order of compute_box_3d_obj_array -- the box of the spare
    row an empty slot gathers."""
    hx, hz = np.asarray([1, 1, -1, -1, 1, 1, -1, -1]) * 0.5, np.asarray([1, -1, -1, 1, 1, -1, -1, 1]) * 0.5
    hy = np.asarray([1, 1, 1, 1, -1, -1, -1, -1]) * 0.5
    return torch.from_numpy(np.stack([hx, hy, hz], 1).reshape(24)).to(dev)


def check_slots(who, B, D, max_d, G=None, b="B"):
    """1 <= B <= D <= the plan's max_d and, with G labels to try them from, D <= G; b: what the source calls its slots."""
    if G is None:
        if not (1 <= B <= D <= max_d):
            raise ValueError("%s: need 1 <= %s <= D <= %d, got %s = %d, D = %d" % (who, b, max_d, b, B, D))
    elif not (1 <= B <= D <= G) or D > max_d:
        raise ValueError("%s: need 1 <= B <= D <= G and D <= %d, got B = %d, D = %d, G = %d" % (who, max_d, B, D, G))


def pick_mode(who, pick, rank, world, seed, dev, D, G, g="G"):
    """A training source's `pick` option -> (the value it stores, its EpochSampler or None).  True: D of the G labels drawn anew
    every step; False: the first D in order; "epoch": a rank window of the epoch's permutation (inputs.EpochSampler keyed `seed`),
    the only mode rank / world go with -- there D * world <= G; g: what the source calls G."""
    if isinstance(pick, str):                                   # (bool("epoch") is True: the string is tested first)
        if pick != "epoch":
            raise ValueError("%s: pick must be True, False or \"epoch\", got %r" % (who, pick))
        rank, world = 0 if rank is None else int(rank), 1 if world is None else int(world)
        if world < 1 or not (0 <= rank < world):
            raise ValueError("%s: need world >= 1 and 0 <= rank < world, got rank = %d, world = %d" % (who, rank, world))
        if D * world > G:
            raise ValueError("%s: pick=\"epoch\" needs D * world <= %s, got D = %d, world = %d, %s = %d" % (who, g, D, world, g, G))
        from .inputs import EpochSampler
        return "epoch", EpochSampler(seed, dev, rank, world)
    if rank is not None or world is not None:
        raise ValueError("%s: rank and world go with pick=\"epoch\"" % who)
    return bool(pick), None


def check_segments(who, D, S, max_segs):
    if D * S > max_segs:
        raise ValueError("%s: D * S = %d * %d segments exceed the plan's %d" % (who, D, S, max_segs))


def check_capacity(who, capacity):
    if capacity < 1:
        raise ValueError("%s: capacity must be >= 1 row, got %d" % (who, capacity))


def check_rows(who, frames, F, groups=None, G=0):
    """The frame column of a table filled from the host: integers in [0, F); with groups, that column too: integers in [0, G)."""
    bad = lambda a, n: len(a) and (a.dtype.kind not in "iu" or a.min() < 0 or a.max() >= n)
    if groups is None:
        if bad(frames, F):
            raise ValueError("%s: frames must be integers in [0, %d)" % (who, F))
    elif bad(frames, F) or bad(groups, G):
        raise ValueError("%s: frames must be integers in [0, %d) and groups integers in [0, %d)" % (who, F, G))


def batch_skeleton(dev, B, units, S, capacity, ps, empty):
    """What every source allocates for its batch of B slots out of `units` boxes of S segments: points (capacity + 1, ps) float32 --
    the spare row is what an empty slot's all-zero choice row reads: fcn_prepare_inputs* indexes off[b] + choice --, seg_off
    (units * S + 1), off (B + 1) and counts (B) int64, the unit of each slot (B) int32 at `empty`, n_kept (1) and status (1) int32."""
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    return (torch.zeros((capacity + 1, ps), dtype=torch.float32, device=dev), torch.zeros((units * S + 1,), **i64),
            torch.zeros((B + 1,), **i64), torch.zeros((B,), **i64), torch.full((B,), empty, **i32), torch.zeros((1,), **i32),
            torch.zeros((1,), **i32))


def adopt(source, table):
    """The table's tensors under their own names on the source, where step(), the tests and the tools read them."""
    for name in table.NAMES:
        setattr(source, name, getattr(table, name))


class LabelTable:
    """The G label boxes of a first-stage training source: validated on the host, resident on the device as g_* tensors, and the D
    rows a step tries (pick_idx) gathered into gt2d / sel2d / gt3d / bframe.  Two calls, because the source's size checks need G and
    come between them: LabelTable(...) parses and checks lengths and frames; load(...) checks the boxes and the class names and
    puts everything on the device."""
    NAMES = ("g_box2d", "g_sel2d", "g_box3d", "g_frame", "g_heading", "g_class", "g_count", "eye", "pick_idx", "pick_scalars",
             "gt2d", "sel2d", "gt3d", "bframe", "boxes")

    def __init__(self, who, gt_box2d, gt_box3d, box_frame, types, F):
        self.who = who
        self.h2d = np.ascontiguousarray(host(gt_box2d), dtype=np.float64).reshape(-1, 4)
        self.h3d = np.ascontiguousarray(host(gt_box3d), dtype=np.float64).reshape(-1, 7)
        self.hframe = bf = np.ascontiguousarray(host(box_frame)).reshape(-1)
        self.G = G = len(bf)
        self.types = [str(t) for t in types]
        if len(self.h2d) != G or len(self.h3d) != G or len(self.types) != G:
            raise ValueError("%s: %d box_frame, %d gt_box2d, %d gt_box3d, %d types" % (who, G, len(self.h2d), len(self.h3d), len(self.types)))
        if bf.dtype.kind not in "iu" or G == 0 or int(bf.min()) < 0 or int(bf.max()) >= F:
            raise ValueError("%s: box_frame must hold integers in [0, %d)" % (who, F))

    def load(self, builder, dev, D, perturb, select_box2d, shift_ratio=0.0, clip_wh=None):
        """clip_wh (F,2) host array: the perturbation clips to the image and draws again (KITTI), so perturb_boxes2d's two refusals
        hold here -- a degenerate label box, and with perturb one that no draw can make valid; None (SUN-RGBD): no clip, no retry,
        nothing to refuse."""
        who, gt2d, G, r = self.who, self.h2d, self.G, shift_ratio
        if clip_wh is not None:
            bad = np.nonzero(~((gt2d[:, 0] < gt2d[:, 2]) & (gt2d[:, 1] < gt2d[:, 3])))[0]
            if len(bad):
                raise ValueError("%s: label box %d is degenerate: %r" % (who, bad[0], tuple(gt2d[bad[0]])))
        if perturb and select_box2d is not None:
            raise ValueError("%s: select_box2d goes with perturb=False" % who)
        if perturb and clip_wh is not None:                     # perturb_boxes2d's second refusal, vectorised
            wh_h = clip_wh[self.hframe]
            w, h = gt2d[:, 2] - gt2d[:, 0], gt2d[:, 3] - gt2d[:, 1]
            cx, cy = (gt2d[:, 0] + gt2d[:, 2]) / 2.0, (gt2d[:, 1] + gt2d[:, 3]) / 2.0
            rx, ry = w * r + w * (1 + r) / 2.0, h * r + h * (1 + r) / 2.0
            bad = np.nonzero(~((cx - rx < wh_h[:, 0] - 1) & (cx + rx > 0) & (cy - ry < wh_h[:, 1] - 1) & (cy + ry > 0)))[0]
            if len(bad):
                raise ValueError("%s: label box %d cannot be perturbed into the %g x %g image: %r" %
                                 (who, bad[0], wh_h[bad[0], 0], wh_h[bad[0], 1], tuple(gt2d[bad[0]])))
        sel2d = gt2d if select_box2d is None else np.ascontiguousarray(host(select_box2d), dtype=np.float64).reshape(-1, 4)
        if len(sel2d) != G:
            raise ValueError("%s: %d select_box2d for %d labels" % (who, len(sel2d), G))
        need_device_builder(builder)
        cls = class_index(who, builder.classes, self.types)
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        # ---- resident: the per-label tensors
        self.g_box2d, self.g_sel2d, self.g_box3d = up(gt2d, dev), up(sel2d, dev), up(self.h3d, dev)
        self.g_frame = up(self.hframe.astype(np.int32), dev)
        self.g_heading = self.g_box3d[:, 6].contiguous()
        self.g_class = up(np.asarray(cls, dtype=np.int64).reshape(G, 1), dev)
        self.eye = torch.eye(len(builder.classes), dtype=torch.float32, device=dev)
        self.g_count = torch.full((1,), G, dtype=torch.int64, device=dev)
        # ---- per step: the D labels tried and their rows
        self.D = D
        self.pick_idx = torch.arange(D, **i32).view(1, D)
        self.pick_scalars = (torch.zeros((1,), **f64), torch.zeros((1,), **f64))
        self.gt2d, self.sel2d, self.gt3d = torch.zeros((D, 4), **f64), torch.zeros((D, 4), **f64), torch.zeros((D, 7), **f64)
        self.bframe = torch.zeros((D,), **i32)
        self.boxes = torch.zeros((D, 4), **f64) if perturb else self.sel2d       # the boxes that select (perturbed or plain)
        del self.h2d, self.h3d, self.hframe
        return self

    def _gather_labels(self):
        idx = self.pick_idx.view(-1)
        for src, dst in ((self.g_box2d, self.gt2d), (self.g_sel2d, self.sel2d), (self.g_box3d, self.gt3d), (self.g_frame, self.bframe)):
            torch.index_select(src, 0, idx, out=dst)

    def pick(self, draws, drawn, advance, sampler=None):
        """The step's D labels: drawn by draws (a DeviceDraws) and gathered, or -- not drawn: the first D in order, gathered once by
        the source -- advance(), the dataset's launch that moves the generator one step on without drawing.  With a sampler (an
        EpochSampler): its window of the epoch's permutation, gathered, and advance() as well."""
        if sampler is not None:
            sampler.pick(self.g_count, self.D, out=self.pick_idx)
            self._gather_labels()
            advance()
        elif drawn:
            draws.draw(self.g_count, self.D, False, False, out=(self.pick_idx,) + self.pick_scalars)
            self._gather_labels()
        else:
            advance()


class DetectTable:
    """The resident table of at most D 2-D detections of an inference source, D + 1 rows: boxes2d (D+1,4) fp64, box_frame, box_class
    (D+1) int32, box_prob (D+1) fp32, n_boxes (1) int32 and, with a spare_group, box_group (D+1) int32.  Row D is the spare row an
    empty slot gathers -- a unit box, frame 0, class 0, spare_group, probability 0 -- written here once."""

    def __init__(self, dev, D, F, classes, spare_group=None):
        self.D, self.F, self.classes, self.spare_group = D, F, classes, spare_group
        i32 = dict(dtype=torch.int32, device=dev)
        self.boxes2d = torch.zeros((D + 1, 4), dtype=torch.float64, device=dev)
        self.boxes2d[D] = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float64, device=dev)
        self.box_frame, self.box_class = torch.zeros((D + 1,), **i32), torch.zeros((D + 1,), **i32)
        self.box_prob, self.n_boxes = torch.zeros((D + 1,), dtype=torch.float32, device=dev), torch.zeros((1,), **i32)
        self.NAMES = ("boxes2d", "box_frame", "box_class", "box_prob", "n_boxes")
        if spare_group is not None:
            self.box_group = torch.full((D + 1,), spare_group, **i32)
            self.NAMES += ("box_group",)

    def set_boxes(self, who, boxes2d, box_frame, types, prob, unit_group=None):
        """Rows 0..n-1 and n_boxes in place from host sequences of n <= D boxes: finite boxes, frames in [0, F), class names of
        classes, finite scores and, in a table with groups, groups in [0, spare_group) (unit_group None: every box its own)."""
        grouped = self.spare_group is not None
        boxes = np.ascontiguousarray(host(boxes2d), dtype=np.float64).reshape(-1, 4)
        fr, pr = np.ascontiguousarray(host(box_frame)).reshape(-1), np.ascontiguousarray(host(prob), dtype=np.float32).reshape(-1)
        n = len(boxes)
        types = [str(t) for t in types]
        cols = [(self.box_frame, fr)]
        if grouped:
            ug = np.arange(n) if unit_group is None else np.ascontiguousarray(host(unit_group)).reshape(-1)
            cols.append((self.box_group, ug))
        if n > self.D or len(pr) != n or len(types) != n or any(len(a) != n for _, a in cols):
            raise ValueError("%s: %d boxes (at most %d), %d frames, %d types, %d scores" % (who, n, self.D, len(fr), len(types), len(pr))
                             + (", %d groups" % len(ug) if grouped else ""))
        check_rows(who, fr, self.F, *((ug, self.spare_group) if grouped else ()))
        if not (np.isfinite(boxes).all() and np.isfinite(pr).all()):
            raise ValueError("%s: boxes and scores must be finite" % who)
        cols.append((self.box_class, class_index(who, self.classes, types)))
        if n:
            self.boxes2d[:n].copy_(up(boxes))
            self.box_prob[:n].copy_(up(pr))
            for dst, src in cols:
                dst[:n].copy_(up(np.asarray(src, dtype=np.int32)))
        self.n_boxes.fill_(n)
