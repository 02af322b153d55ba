"""On-device batch construction from raw frustum records (C-ABI fcn_prepare_inputs, csrc/inputs.hip).

Host-side mirror of the reference's loader for this step (datasets/provider_sample.py): ProviderDataset.__getitem__
(:137-262) builds every sample in numpy on DataLoader workers (cfgs/det_sample.yaml NUM_WORKERS) and default_collate
(:396-397) stacks them; here the raw records of a batch go to the GPU in ONE packed upload and one kernel launch writes
the dict PointNetDet.forward consumes (same keys, shapes and dtypes as the reference's collated batch).

By default randomness stays on the host and follows the reference's call order per sample -- np.random.choice (resample),
np.random.random (flip coin), np.random.randn (depth shift) -- so with the same numpy seed the batch equals the
reference's batch (tests/test_gpu_inputs.py checks that against the golden fixture).  DeviceDraws makes the same draws on the
device from a counter-based stream of its own (C-ABI fcn_draw_batch, csrc/draws.h): every builder takes one as `draws=`.
EpochSampler picks a training step's labels from the same stream as a rank window of the epoch's permutation (C-ABI fcn_epoch_pick,
csrc/epoch_pick.h): what the training sources' pick="epoch" runs.
"""
import ctypes

import numpy as np
import torch

from . import _native
from ._native import InpDesc, Inp5Desc
from .config import cfg
from .dataset_info import DATASET_INFO

RECORD_KEYS = ("points", "seg", "box2d", "P", "box3d", "heading", "size", "frustum_angle", "type")


def draw(counts, npoints, random_flip=True, random_shift=True, rng=np.random):
    """The reference's per-sample random draws, in its order (provider_sample.py:165-168, :225, :238)."""
    choice, coin, normal = [], [], []
    for n in counts:
        choice.append(rng.choice(int(n), npoints, int(n) < npoints))
        coin.append(rng.random() if random_flip else 0.0)
        normal.append(rng.randn() if random_shift else 0.0)
    return np.stack(choice).astype(np.int32), np.asarray(coin, dtype=np.float64), np.asarray(normal, dtype=np.float64)


class DeviceDraws:
    """The same draws made ON THE DEVICE by a counter-based generator (C-ABI fcn_draw_batch, csrc/draws.h): one launch writes
    choice (B,N) int32, coin, normal (and hshift) (B) float64 where fcn_prepare_inputs* reads them -- no host read of the counts, no
    upload, capturable.  The stream is Philox4x32-10 keyed by `seed` and counted by the device-resident step counter `state`
    (INTEGRATION.md "Random draws on the device" states the contract bit for bit); it is NOT numpy's, so the host draw() stays the
    default of every builder and the path the golden fixtures check.  Pass an instance as `draws=` to a builder.
    state: (1,) int64 -- every draw() reads it and leaves it one higher, in stream order; writing a value back reproduces that
    draw.  status: (1,) int32 -- bit 0 is set by a row nothing could be drawn from (see check())."""

    def __init__(self, seed, device="cuda"):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("frustum_convnet_amd: the device draws are a HIP kernel (MI355X only); no CPU fallback")
        self.state = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.device)

    @staticmethod
    def limits():
        """(the largest npoints, the row count up to which a row is sorted whole in LDS) of fcn_draw_batch."""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        _native.check(_native.lib().fcn_draw_limits(ctypes.byref(a), ctypes.byref(b)), "fcn_draw_limits")
        return a.value, b.value

    @staticmethod
    def _want(name, t, dtype, numel=None):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("DeviceDraws.draw: %s must be a device tensor" % name)
        if t.dtype != dtype or not t.is_contiguous():
            raise ValueError("DeviceDraws.draw: %s must be a contiguous %s tensor, got %s" % (name, dtype, t.dtype))
        if numel is not None and t.numel() != numel:
            raise ValueError("DeviceDraws.draw: %s must hold %d elements, got %s" % (name, numel, tuple(t.shape)))
        return t

    def draw(self, counts, npoints, random_flip, random_shift, hshift=False, sub=None, sub_off=None, out=None):
        """counts (B,) int64 on the device: the rows of each sample.  -> (choice (B,npoints) int32, coin (B), normal (B) float64
        [, hshift (B) float64 when hshift]) on the device, into `out` (a tuple of that shape) when given: then there is no
        allocation and no host read, only the two launches -- capturable.  sub (packed int32) / sub_off (B+1 int64), both or
        neither: a sample with a non-empty slice draws from the slice's length and gets sub's values (SUN-RGBD's frustum subsample).
        A sample without a row gets zeros and flags `status`: see check()."""
        N = int(npoints)
        self._want("counts", counts, torch.int64)
        B = int(counts.numel())
        if B <= 0 or N <= 0:
            raise ValueError("DeviceDraws.draw: %d samples of %d points" % (B, N))
        if (sub is None) != (sub_off is None):
            raise ValueError("DeviceDraws.draw: sub and sub_off go together")
        if sub is not None:
            self._want("sub", sub, torch.int32)
            self._want("sub_off", sub_off, torch.int64, B + 1)
        if out is None:
            f64 = dict(dtype=torch.float64, device=self.device)
            out = (torch.empty((B, N), dtype=torch.int32, device=self.device), torch.empty((B,), **f64), torch.empty((B,), **f64))
            if hshift:
                out = out + (torch.empty((B,), **f64),)
        if len(out) != (4 if hshift else 3):
            raise ValueError("DeviceDraws.draw: out must hold %d tensors" % (4 if hshift else 3))
        self._want("out[0] (choice)", out[0], torch.int32, B * N)
        for name, t in zip(("coin", "normal", "hshift"), out[1:]):
            self._want("out (%s)" % name, t, torch.float64, B)
        desc = _native.DrawDesc(B, N, 1 if random_flip else 0, 1 if random_shift else 0)
        p = lambda x: None if x is None else x.data_ptr()
        with torch.cuda.device(self.device):
            _native.check(_native.lib().fcn_draw_batch(
                ctypes.byref(desc), p(counts), p(sub), p(sub_off), self.seed, p(self.state), p(out[0]), p(out[1]), p(out[2]),
                p(out[3]) if hshift else None, p(self.status), _native.current_stream(self.device)), "fcn_draw_batch")
        stream = torch.cuda.current_stream(self.device)
        for t in (counts, sub, sub_off):
            if t is not None:
                t.record_stream(stream)
        return tuple(out)

    def check(self):
        """Reads `status` (a synchronisation: not for a captured region) and raises ValueError when a draw since the last check()
        met a sample with no row, or with 2^31 rows or more; the word is cleared."""
        s = int(self.status.cpu()[0])
        if s:
            self.status.zero_()
            raise ValueError("DeviceDraws: a sample had no row to draw from (or 2^31 rows or more): its choice row is zeros")


class EpochSampler:
    """The labels of a training step as a rank window of the EPOCH's permutation, on the device (C-ABI fcn_epoch_pick,
    csrc/epoch_pick.h): what the reference's DataLoader(shuffle=True, drop_last=True) walks -- a fresh permutation per epoch, every
    label at most once per epoch, the tail that fills no step dropped -- with no G-sized table and no host read, capturable
    (INTEGRATION.md "Epoch-exact label sampling" states the contract bit for bit).  The permutation of epoch e is the order
    DeviceDraws gives row 0 at step e under the same `seed`; a step takes the D labels at ranks (turn * world + rank) * D ...
    state: (2,) int64 -- epoch, turn; every pick() reads it and leaves the next turn (or the next epoch's turn 0) behind, in stream
    order; writing a pair back reproduces that pick, so a checkpoint of the data order is these 16 bytes.  Ranks built with the same
    seed hold the same state and take disjoint windows.  status: (1,) int32 -- bit 0 is set by a pick that had no window (see
    check())."""

    def __init__(self, seed, device="cuda", rank=0, world=1):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("frustum_convnet_amd: the epoch sampler is a HIP kernel (MI355X only); no CPU fallback")
        self.rank, self.world = int(rank), int(world)
        if self.world < 1 or not (0 <= self.rank < self.world):
            raise ValueError("EpochSampler: need world >= 1 and 0 <= rank < world, got rank = %d, world = %d" % (self.rank, self.world))
        self.state = torch.zeros((2,), dtype=torch.int64, device=self.device)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.device)

    @staticmethod
    def limits():
        """(the largest D, the count up to which the permutation is sorted whole in LDS) of fcn_epoch_pick."""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        _native.check(_native.lib().fcn_epoch_pick_limits(ctypes.byref(a), ctypes.byref(b)), "fcn_epoch_pick_limits")
        return a.value, b.value

    def steps_per_epoch(self, G, D):
        """The turns of an epoch over G labels at D per step and rank: floor(G / (D * world))."""
        return int(G) // (int(D) * self.world)

    @staticmethod
    def _want(name, t, dtype, numel):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("EpochSampler.pick: %s must be a device tensor" % name)
        if t.dtype != dtype or not t.is_contiguous():
            raise ValueError("EpochSampler.pick: %s must be a contiguous %s tensor, got %s" % (name, dtype, t.dtype))
        if t.numel() != numel:
            raise ValueError("EpochSampler.pick: %s must hold %d elements, got %s" % (name, numel, tuple(t.shape)))
        return t

    def pick(self, count, D, out=None, advance=True):
        """count (1,) int64 on the device: the number of labels G.  -> pick (D,) int32 on the device, into `out` (D elements) when
        given: then there is no allocation and no host read, only the launch -- capturable.  A state without a window (D * world > G,
        a turn outside the epoch, G outside (0, 2^31)) gives zeros, flags `status` and stays as it was: see check()."""
        D = int(D)
        self._want("count", count, torch.int64, 1)
        if D <= 0:
            raise ValueError("EpochSampler.pick: %d labels per step" % D)
        if out is None:
            out = torch.empty((D,), dtype=torch.int32, device=self.device)
        self._want("out", out, torch.int32, D)
        with torch.cuda.device(self.device):
            _native.check(_native.lib().fcn_epoch_pick(count.data_ptr(), D, self.rank, self.world, self.seed, self.state.data_ptr(),
                                                       1 if advance else 0, out.data_ptr(), self.status.data_ptr(),
                                                       _native.current_stream(self.device)), "fcn_epoch_pick")
        count.record_stream(torch.cuda.current_stream(self.device))
        return out

    def check(self):
        """Reads `status` (a synchronisation: not for a captured region) and raises ValueError when a pick since the last check()
        had no window; the word is cleared."""
        s = int(self.status.cpu()[0])
        if s:
            self.status.zero_()
            raise ValueError("EpochSampler: a pick had no window (D * world > G, a turn outside the epoch, or G outside (0, 2^31)): "
                             "it is zeros and the state stayed")


def _is_device_draws(draws):
    """A tuple of device tensors: used as it is (no np.asarray, no upload)."""
    return isinstance(draws, (tuple, list)) and len(draws) > 0 and all(isinstance(x, torch.Tensor) and x.is_cuda for x in draws)


def _draw_tensors(draws, dev, n):
    """draws as the n device tensors the prepare kernels read: device tensors as they are, host arrays uploaded."""
    if _is_device_draws(draws):
        return tuple(draws[:n])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
    return (up(np.asarray(draws[0], dtype=np.int32)),) + tuple(up(np.asarray(x, dtype=np.float64)) for x in draws[1:n])


def _row_counts(off):
    """(B+1,) offsets on the device -> (B,) int64 row counts on the device."""
    return (off[1:] - off[:-1]).to(torch.int64).contiguous()


# ---- what the three builders share
def _need_device(device):
    """The refusal of every public entry method of the builders off the GPU."""
    if device.type != "cuda":
        raise RuntimeError("frustum_convnet_amd: input construction is a HIP kernel (MI355X only); no CPU fallback")


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)


def _ptr(x):
    return None if x is None else x.data_ptr()


def _pack(records, counts, fields):
    """Host records as the arrays ONE upload each hands a launch: raw (sum n, pt_stride) float32 -- the records' points end to end
    --, off (B+1) int64 and, per (name, record key, shape) of `fields`, the (B, *shape) float64 stack of that key."""
    h = {"raw": np.concatenate([np.ascontiguousarray(r["points"], dtype=np.float32) for r in records], 0),
         "off": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)}
    h.update(_stacks(records, fields))
    return h


def _stacks(records, fields):
    return {name: np.stack([np.asarray(r[key], dtype=np.float64).reshape(shape) for r in records]) for name, key, shape in fields}


def _class_rows(b, d, names, size_class=True):
    """Into d, uploaded: size_class (B,1) int64, the class names' indices in builder b's table, and -- where b has one_hot -- their
    one-hot rows (B, classes) float32.  The names are looked up (an unknown one raises ValueError) only where one of the two is
    written: an inference batch without one_hot takes any name."""
    if not (size_class or b.one_hot):
        return
    idx = [b.classes.index(n) for n in names]
    if size_class:
        d["size_class"] = torch.tensor(idx, dtype=torch.int64).view(len(idx), 1).to(b.device, non_blocking=True)
    if b.one_hot:
        oh = np.zeros((len(idx), len(b.classes)), dtype=np.float32)
        oh[np.arange(len(idx)), idx] = 1.0
        d["one_hot"] = _up(oh, b.device)


def _desc_refs(desc, B, N, pt_stride, L, strides, out, *tail):
    """A launch's descriptor (desc: its ctypes class; tail: the fields behind the strides) and the pointer array of out's center_ref*."""
    n = len(strides)
    refs = (ctypes.c_void_p * n)(*[out["center_ref%d" % (s + 1)].data_ptr() for s in range(n)])
    return desc(B, N, pt_stride, (ctypes.c_int32 * n)(*L), (ctypes.c_double * n)(*strides), *tail), refs


def _record(t, dev):
    """The tensors of t are read by the kernel just enqueued on the current stream."""
    for v in t.values():
        if isinstance(v, torch.Tensor):
            v.record_stream(torch.cuda.current_stream(dev))


class _FirstStageBuilder:
    """The first stage's builder at NSC strides: InputBuilder and SunrgbdInputBuilder are this class with their parameters --
    DESC (the descriptor), ENTRY / ENTRY_INFER (the C entries), DATASET (the class table; None: cfg.DATA.DATASET_NAME), CALIB (per
    calibration matrix: its key in t, its key in a record, its shape there), DRAW (the reference's draws) and DRAW_KEYS (their keys
    in t) -- and with what is their own: how the boxes of a device selection are skipped, drawn for and calibrated."""

    def __init__(self, npoints, strides=None, max_depth=None, random_flip=False, random_shift=False, one_hot=True,
                 device="cuda"):
        self.npoints = int(npoints)
        self.strides = tuple(float(s) for s in (cfg.DATA.STRIDE if strides is None else strides))
        self.max_depth = float(cfg.DATA.MAX_DEPTH if max_depth is None else max_depth)
        assert len(self.strides) == self.NSC
        self.L = [len(np.arange(0, self.max_depth, s)) for s in self.strides]
        self.random_flip, self.random_shift, self.one_hot = bool(random_flip), bool(random_shift), bool(one_hot)
        self.device = torch.device(device)
        self.classes = DATASET_INFO[self.DATASET or cfg.DATA.DATASET_NAME].CLASSES

    def build(self, records, draws=None, with_seg=True):
        """records: list of dicts with RECORD_KEYS (points (n,>=3) float32 in rect camera coordinates, seg (n,), box2d (4,),
        P (3,4), box3d (8,3) corners, heading, size (l,w,h), frustum_angle, type); SUN-RGBD: K, Rtilt for P, see the class.
        draws: (choice (B,N) int32, coin (B), normal (B)[, hshift (B)]) -- host arrays, or device tensors used as they are -- a
        DeviceDraws to draw on the device, or None to draw like the reference (here and wherever a builder takes `draws`).  Returns
        the batch dict on the device.
        = the upload (host -> device copies of the raw records and the draws) + launch() (the kernel)."""
        return self.launch(self._upload(records, draws, with_seg))

    def _upload(self, records, draws, with_seg):
        """The raw records of a batch and their random draws as device tensors (ONE packed point buffer): launch()'s `t`."""
        _need_device(self.device)
        B, N, dev = len(records), self.npoints, self.device
        counts = [len(r["points"]) for r in records]
        if draws is None:
            draws = self.DRAW(counts, N, self.random_flip, self.random_shift)
        pt_stride = int(records[0]["points"].shape[1])
        fields = (("fangle", "frustum_angle", ()), ("box2d", "box2d", (4,))) + self.CALIB + (
            ("corners", "box3d", (24,)), ("heading", "heading", ()), ("size", "size", (3,)))
        t = {k: _up(v, dev) for k, v in _pack(records, counts, fields).items()}
        if isinstance(draws, DeviceDraws):          # drawn on the device from the uploaded offsets (re-draw into these any time)
            draws = draws.draw(_row_counts(t["off"]), N, self.random_flip, self.random_shift, hshift=len(self.DRAW_KEYS) == 4)
        t.update(zip(self.DRAW_KEYS, _draw_tensors(draws, dev, len(self.DRAW_KEYS))))
        t["seg"] = _up(np.concatenate([np.asarray(r["seg"]).astype(np.int64) for r in records], 0), dev) if with_seg else None
        _class_rows(self, t, [r["type"] for r in records])
        t["B"], t["pt_stride"] = B, pt_stride
        return t

    def alloc(self, B, with_seg=True):
        """Output tensors of launch() for a batch of B frustums (pass as `out` to write the same buffers every step)."""
        dev, N = self.device, self.npoints
        f32 = dict(dtype=torch.float32, device=dev)
        out = {"point_cloud": torch.empty((B, 3, N), **f32), "rot_angle": torch.empty((B, 1), **f32),
               "cls_label": torch.empty((B, self.L[1]), dtype=torch.int64, device=dev),
               "box3d_center": torch.empty((B, 3), **f32), "box3d_heading": torch.empty((B, 1), **f32),
               "box3d_size": torch.empty((B, 3), **f32)}
        for s in range(self.NSC):
            out["center_ref%d" % (s + 1)] = torch.empty((B, 3, self.L[s]), **f32)
        if with_seg:
            out["seg_label"] = torch.empty((B, N), dtype=torch.int64, device=dev)
        return out

    def launch(self, t, out=None):
        """ONE kernel launch on the current stream: device tensors `t` -- raw, off, seg (or None), choice, fangle, box2d, the
        calibration (P; SUN-RGBD: K, R), corners, heading, size, coin, normal (, hshift), size_class (, one_hot), B, pt_stride: the
        uploaded records -- -> the batch dict (into `out` when given: capturable into a hipGraph, no allocation, no host work besides
        the call).  size_class / one_hot are t's tensors."""
        dev = self.device
        if out is None:
            out = self.alloc(t["B"], with_seg=t["seg"] is not None)
        desc, refs = _desc_refs(self.DESC, t["B"], self.npoints, t["pt_stride"], self.L, self.strides, out, self.max_depth,
                                1 if self.random_flip else 0, 1 if self.random_shift else 0)
        ins = ("raw", "off", "seg", "choice", "fangle", "box2d") + tuple(c[0] for c in self.CALIB) + (
            "corners", "heading", "size") + self.DRAW_KEYS[1:]
        outs = ("cls_label", "box3d_center", "box3d_heading", "box3d_size", "rot_angle")
        with torch.cuda.device(dev):
            _native.check(getattr(_native.lib(), self.ENTRY)(
                ctypes.byref(desc), *[_ptr(t[k]) for k in ins], _ptr(out["point_cloud"]), refs, *[_ptr(out[k]) for k in outs],
                _ptr(out.get("seg_label")) if t["seg"] is not None else None, _native.current_stream(dev)), self.ENTRY)
        _record(t, dev)                            # the uploads are read by the kernel just enqueued
        out["size_class"] = t["size_class"]
        if "one_hot" in t:
            out["one_hot"] = t["one_hot"]
        return out

    def alloc_infer(self, B):
        """Output tensors of launch_infer() for a batch of B frustums: the dict of build_device() without 'kept' -- point_cloud,
        rot_angle, center_ref1..NSC, rgb_prob (B,1) and, with one_hot, one_hot (B, classes), both zeros for the caller to fill."""
        dev, N = self.device, self.npoints
        f32 = dict(dtype=torch.float32, device=dev)
        out = {"point_cloud": torch.empty((B, 3, N), **f32), "rot_angle": torch.empty((B, 1), **f32)}
        for s in range(self.NSC):
            out["center_ref%d" % (s + 1)] = torch.empty((B, 3, self.L[s]), **f32)
        out["rgb_prob"] = torch.zeros((B, 1), **f32)
        if self.one_hot:
            out["one_hot"] = torch.zeros((B, len(self.classes)), **f32)
        return out

    def launch_infer(self, t, out):
        """ONE launch of ENTRY_INFER on the current stream: device tensors `t` -- raw, off, choice (SUN-RGBD: indices into the full
        packed selection), fangle, box2d, the calibration (P; SUN-RGBD: K, R), B, pt_stride -- into the caller-owned `out` of
        alloc_infer(): no allocation, no host work besides the call (capturable into a hipGraph).  rgb_prob / one_hot are the
        caller's to write.  Returns out."""
        dev = self.device
        desc, refs = _desc_refs(self.DESC, t["B"], self.npoints, t["pt_stride"], self.L, self.strides, out, self.max_depth, 0, 0)
        ins = ("raw", "off", "choice", "fangle", "box2d") + tuple(c[0] for c in self.CALIB)
        with torch.cuda.device(dev):
            _native.check(getattr(_native.lib(), self.ENTRY_INFER)(
                ctypes.byref(desc), *[t[k].data_ptr() for k in ins], out["point_cloud"].data_ptr(), refs, out["rot_angle"].data_ptr(),
                _native.current_stream(dev)), self.ENTRY_INFER)
        return out

    def _calib(self, box_frame, *mats):
        """The frames' calibration matrices (CALIB's, in its order) gathered per box through box_frame: {key in t: (B, 12 or 9) float64}."""
        idx = box_frame.to(torch.int64)
        return {k: torch.as_tensor(m).to(device=self.device, dtype=torch.float64).reshape((-1,) + shape).index_select(0, idx).contiguous()
                for (k, _, shape), m in zip(self.CALIB, mats)}

    def _picker(self, kept):
        """x -> the rows `kept` (host indices) of a device tensor."""
        idx = _up(kept, self.device)
        return lambda x: x.index_select(0, idx).contiguous()

    def _infer(self, sel, kept, pick, choice, calib, types, prob):
        """What build_device() does once it knows the survivors `kept`, their choice table and calibration rows: ONE launch of
        ENTRY_INFER through alloc_infer() / launch_infer(), the 2-D scores and the one-hot rows, 'kept'."""
        B = len(kept)
        t = dict(calib, raw=sel["points"], choice=choice, off=pick(sel["off"]),      # (the kernel reads a sample's first row only)
                 fangle=pick(sel["frustum_angle"]), box2d=pick(sel["box2d"]))
        out = self.launch_infer(dict(t, B=B, pt_stride=int(sel["points"].shape[1])), self.alloc_infer(B))
        _record(t, self.device)
        out["rgb_prob"] = _up(np.asarray(prob, dtype=np.float32)[kept].reshape(B, 1), self.device)
        _class_rows(self, out, [types[i] for i in kept], size_class=False)
        out["kept"] = kept
        return out

    def _train(self, sel, kept, drawn, calib, types, with_seg, out=None):
        """What build_device_train() does once it has the draws' device tensors `drawn` (DRAW_KEYS' order) and the calibration rows:
        the selection as launch()'s `t`, ONE launch of ENTRY."""
        K = len(kept)
        t = {"raw": sel["points"], "off": sel["off"], "seg": sel["seg"] if with_seg else None, "fangle": sel["frustum_angle"],
             "box2d": sel["box2d"], "corners": sel["box3d"].reshape(K, 24), "heading": sel["heading"], "size": sel["size"]}
        t.update(calib)
        t.update(zip(self.DRAW_KEYS, drawn))
        _class_rows(self, t, [types[i] for i in kept])
        t["B"], t["pt_stride"] = K, int(sel["points"].shape[1])
        return self.launch(t, out)


class InputBuilder(_FirstStageBuilder):
    """npoints / strides / max_depth as cfg.DATA.{NUM_SAMPLES, STRIDE, MAX_DEPTH}; one_hot over the dataset's classes."""
    NSC, DESC, DATASET = 4, InpDesc, None
    ENTRY, ENTRY_INFER = "fcn_prepare_inputs", "fcn_prepare_inputs_infer"
    CALIB = (("P", "P", (12,)),)
    DRAW, DRAW_KEYS = staticmethod(draw), ("choice", "coin", "normal")

    def upload(self, records, draws=None, with_seg=True):
        """The raw records of a batch and their random draws as device tensors (ONE packed point buffer): what a loader hands
        the GPU.  The returned dict feeds launch() any number of times (a resident raw batch re-built every step: bench.py)."""
        return self._upload(records, draws, with_seg)

    def build_device(self, sel, P, types, prob, draws=None, img_height_threshold=5, lidar_point_threshold=1):
        """The first stage's inference batch (the reference's from_rgb_detection dict, provider_sample.py:184-195: point_cloud,
        rot_angle, rgb_prob, center_ref1..4, one_hot) straight from the device tensors of frustum.frustum_candidates: no point
        leaves the device.  sel: its dict; P (F,3,4): the frames' projection matrices (calib["P"]), gathered per box through
        sel["box_frame"]; types / prob: the class name and the 2-D detector's score of each of the D boxes; draws: (choice (B,N)
        int32, ...) for the B surviving boxes, or None to draw like draw() from their counts (no flip, no shift: inference).
        A box is dropped when ymax - ymin < img_height_threshold, xmax - xmin < 1 or count < lidar_point_threshold
        (prepare_data.py:546-548; a box without a point cannot be resampled and is dropped in any case); 'kept' (B,) int64 (host) lists the survivors' box indices.  The host reads the D boxes here.
        ONE launch of fcn_prepare_inputs_infer.  With no survivor the dict holds 'kept' alone."""
        _need_device(self.device)
        counts = np.asarray(sel["counts"], dtype=np.int64)
        D, N = len(counts), self.npoints
        if len(types) != D or len(prob) != D:
            raise ValueError("build_device: %d boxes, %d types, %d prob" % (D, len(types), len(prob)))
        box = sel["box2d"].cpu().numpy().reshape(D, 4)                        # D boxes: the skip rules
        skip = (box[:, 3] - box[:, 1] < img_height_threshold) | (box[:, 2] - box[:, 0] < 1) | (counts < lidar_point_threshold)
        kept = np.nonzero(~skip & (counts > 0))[0]
        if len(kept) == 0:
            return {"kept": kept}
        if draws is None:
            draws = draw(counts[kept], N, False, False)
        pick = self._picker(kept)
        if isinstance(draws, DeviceDraws):
            draws = draws.draw(pick(_row_counts(sel["off"])), N, False, False)
        return self._infer(sel, kept, pick, _draw_tensors(draws, self.device, 1)[0], self._calib(pick(sel["box_frame"]), P), types, prob)

    def build_device_train(self, sel, P, types, draws=None, with_seg=True, out=None):
        """The first stage's TRAINING batch -- the dict of build(), same keys, shapes and dtypes -- straight from the device
        tensors of frustum.frustum_training_candidates: no point, label or corner leaves the device.  sel: its dict; P (F,3,4):
        the frames' projection matrices, gathered per box through sel["box_frame"]; types: the class name of each of the D boxes
        frustum_training_candidates was given (the kept ones are looked up through sel["kept"]); draws: (choice (K,N) int32,
        coin (K), normal (K)) for the K kept boxes, or None to draw like the reference from their counts; out: launch()'s.
        ONE launch of fcn_prepare_inputs.  With no kept box the dict holds 'kept' alone."""
        _need_device(self.device)
        kept = np.asarray(sel["kept"], dtype=np.int64)
        if len(kept) == 0:
            return {"kept": kept}
        if draws is None:
            draws = draw(sel["counts"], self.npoints, self.random_flip, self.random_shift)
        if isinstance(draws, DeviceDraws):
            draws = draws.draw(_row_counts(sel["off"]), self.npoints, self.random_flip, self.random_shift)
        return self._train(sel, kept, _draw_tensors(draws, self.device, 3), self._calib(sel["box_frame"], P), types, with_seg, out)

    def algorithmic_bytes(self, B, with_seg=True, pt_stride=4):
        """HBM bytes one launch has to move (the roofline's numerator): per frustum N gathered raw points + their draw indices
        (+ seg labels) in, point cloud + window centres + labels (+ seg) out; the per-frustum scalars (~400 B) ignored."""
        N = self.npoints
        per = N * (4 * pt_stride + 4) + 12 * N + 12 * sum(self.L) + 8 * self.L[1] + (16 * N if with_seg else 0)
        return B * per


def draw_sunrgbd(counts, npoints, random_flip=True, random_shift=True, rng=np.random):
    """The SUN-RGBD loader's per-sample draws, in its order (provider_sample_sunrgbd.py:144, :211, :224, :228): resample
    (WITH replacement only when the frustum has fewer points than npoints), flip coin, depth-shift normal, height-shift
    uniform."""
    choice, coin, normal, hshift = [], [], [], []
    for n in counts:
        choice.append(rng.choice(int(n), npoints, int(n) < npoints))
        coin.append(rng.random() if random_flip else 0.0)
        normal.append(rng.randn() if random_shift else 0.0)
        hshift.append(rng.random() if random_shift else 0.5)
    f = lambda v: np.asarray(v, dtype=np.float64)
    return np.stack(choice).astype(np.int32), f(coin), f(normal), f(hshift)


class SunrgbdInputBuilder(_FirstStageBuilder):
    """Batch construction of datasets/provider_sample_sunrgbd.py::ProviderDataset (+ default_collate) on the device: five
    strides, window centres through the camera matrix K and the tilt rotation Rtilt.  Records: points (n,>=3) float32 in
    upright camera coordinates, seg (n,), box2d (4,), K (3,3), Rtilt (3,3), box3d (8,3), heading, size (l,w,h),
    frustum_angle, type.  draws: (choice (B,N) int32, coin (B), normal (B), hshift (B)) or None to draw like the reference."""
    NSC, DESC, DATASET = 5, Inp5Desc, "SUNRGBD"
    ENTRY, ENTRY_INFER = "fcn_prepare_inputs_sunrgbd", "fcn_prepare_inputs_sunrgbd_infer"
    CALIB = (("K", "K", (9,)), ("R", "Rtilt", (9,)))
    DRAW, DRAW_KEYS = staticmethod(draw_sunrgbd), ("choice", "coin", "normal", "hshift")

    def _compose(self, choice, sub):
        """The builder's draw through the reference's frustum subsample: choice (B,N) indexes the subsampled record where a box
        has one, sub[b][choice[b]] the box's slice of the full packed selection."""
        choice = np.array(choice, dtype=np.int32)
        for b, ix in enumerate(sub):
            if ix is not None:
                choice[b] = np.asarray(ix, dtype=np.int32)[choice[b]]
        return choice

    def _device_draw(self, dd, cnt, sub, flip, shift):
        """dd.draw over the records' rows with the frustum subsamples composed in the kernel: cnt (B,) the boxes' full row counts
        on the device, sub: per box the host's subsample indices or None -- packed and uploaded (a box without one draws from
        its cnt rows)."""
        counts = cnt.to(torch.int64).contiguous()
        if all(ix is None for ix in sub):
            return dd.draw(counts, self.npoints, flip, shift, hshift=True)
        lens = [0 if ix is None else len(ix) for ix in sub]
        sub_off = _up(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), self.device)
        flat = _up(np.concatenate([np.asarray(ix, dtype=np.int32) for ix in sub if ix is not None]), self.device)
        return dd.draw(counts, self.npoints, flip, shift, hshift=True, sub=flat, sub_off=sub_off)

    def _choice(self, draws, sub):
        """The choice table the kernel reads: a device tensor as it is -- indices into the full packed selection, as
        DeviceDraws writes them through `sub` -- a host table composed with the subsamples and uploaded."""
        return draws[0] if _is_device_draws(draws) else _up(self._compose(draws[0], sub), self.device)

    def build_device(self, sel, K, Rtilt, types, prob, draws=None, point_threshold=5):
        """The five-scale model's inference batch (the reference's from_rgb_detection dict, provider_sample_sunrgbd.py:165-186:
        point_cloud, rot_angle, rgb_prob, center_ref1..5, one_hot) straight from the device tensors of frustum.sunrgbd_candidates:
        no point leaves the device.  sel: its dict; K, Rtilt (F,3,3): the frames' calibration, gathered per box through
        sel["box_frame"]; types / prob: the class name and the 2-D detector's score of each of the D boxes; draws: (choice (B,N)
        int32, ...) for the B surviving boxes -- indices into each box's RECORD, i.e. into its subsample where sel["sub"] has one
        -- or None to draw like draw_sunrgbd from the records' row counts (no flip, no shift: inference).
        A box whose record has fewer than point_threshold rows is skipped (sunrgbd/prepare_data.py:352); 'kept' (B,) int64 (host)
        lists the survivors' box indices.  ONE launch of fcn_prepare_inputs_sunrgbd_infer, which gathers from the full packed
        selection through sub[choice].  With no survivor the dict holds 'kept' alone."""
        from .frustum import subsampled_counts
        _need_device(self.device)
        D, N = len(sel["counts"]), self.npoints
        if len(types) != D or len(prob) != D:
            raise ValueError("build_device: %d boxes, %d types, %d prob" % (D, len(types), len(prob)))
        rows = subsampled_counts(sel["counts"], sel["sub"])
        kept = np.nonzero(rows >= max(1, int(point_threshold)))[0]
        if len(kept) == 0:
            return {"kept": kept}
        if draws is None:
            draws = draw_sunrgbd(rows[kept], N, False, False)
        pick, sub = self._picker(kept), [sel["sub"][d] for d in kept]
        if isinstance(draws, DeviceDraws):
            draws = self._device_draw(draws, pick(sel["cnt"]), sub, False, False)
        return self._infer(sel, kept, pick, self._choice(draws, sub), self._calib(pick(sel["box_frame"]), K, Rtilt), types, prob)

    def build_device_train(self, sel, K, Rtilt, types, draws=None, with_seg=True):
        """The five-scale model's TRAINING batch -- the dict of build(), same keys, shapes and dtypes -- straight from the device
        tensors of frustum.sunrgbd_training_candidates: no point, label or corner leaves the device.  sel: its dict; K, Rtilt
        (F,3,3), gathered per box through sel["box_frame"]; types: the class name of each of the D boxes
        sunrgbd_training_candidates was given (the kept ones are looked up through sel["kept"]); draws: (choice (K,N) int32, coin,
        normal, hshift) for the K kept boxes -- choice indexes each box's RECORD, i.e. its subsample where sel["sub"] has one -- or
        None to draw like the reference from the records' row counts.  ONE launch of fcn_prepare_inputs_sunrgbd, which gathers
        points and labels from the full packed selection through sub[choice].  With no kept box the dict holds 'kept' alone."""
        from .frustum import subsampled_counts
        _need_device(self.device)
        kept = np.asarray(sel["kept"], dtype=np.int64)
        if len(kept) == 0:
            return {"kept": kept}
        if draws is None:
            draws = draw_sunrgbd(subsampled_counts(sel["counts"], sel["sub"]), self.npoints, self.random_flip, self.random_shift)
        if isinstance(draws, DeviceDraws):
            draws = self._device_draw(draws, sel["cnt"], sel["sub"], self.random_flip, self.random_shift)
        drawn = (self._choice(draws, sel["sub"]),) + _draw_tensors(draws, self.device, 4)[1:]
        return self._train(sel, kept, drawn, self._calib(sel["box_frame"], K, Rtilt), types, with_seg)


def sunrgbd_records_from_fixture(g):
    """tests/golden/inputs_sunrgbd_b6.npz (make_golden_inputs_sunrgbd.py) as a list of records."""
    offs = np.concatenate([[0], np.cumsum(g["raw_counts"])])
    recs = []
    for b in range(len(g["raw_counts"])):
        sl = slice(int(offs[b]), int(offs[b + 1]))
        recs.append({"points": g["raw_points"][sl], "seg": g["raw_seg"][sl], "box2d": g["box2d"][b], "K": g["K"][b],
                     "Rtilt": g["Rtilt"][b], "box3d": g["box3d_corners"][b], "heading": float(g["heading"][b]),
                     "size": g["size"][b], "frustum_angle": float(g["frustum_angle"][b]), "type": str(g["types"][b])})
    return recs


def records_from_fixture(g):
    """The golden fixture's packed arrays (tests/golden/make_golden_inputs.py) as a list of records."""
    offs = np.concatenate([[0], np.cumsum(g["raw_counts"])])
    recs = []
    for b in range(len(g["raw_counts"])):
        sl = slice(int(offs[b]), int(offs[b + 1]))
        recs.append({"points": g["raw_points"][sl], "seg": g["raw_seg"][sl], "box2d": g["box2d"][b], "P": g["P"][b],
                     "box3d": g["box3d_corners"][b], "heading": float(g["heading"][b]), "size": g["size"][b],
                     "frustum_angle": float(g["frustum_angle"][b]), "type": "Car"})
    return recs


# ------------------------------------------------------------------------------------------------
REFINE_KEYS = ("points", "box3d", "heading", "size", "pred_box3d", "pred_angle", "pred_size", "type")


def draw_refine(counts, npoints, random_flip=True, random_shift=True, rng=np.random):
    """The refine dataset's per-sample draws in its order (provider_sample_refine.py:209, :268, :282)."""
    return draw(counts, npoints, random_flip, random_shift, rng)


class RefineInputBuilder:
    """Refinement-stage batches (cfgs/refine_car.yaml) from raw records + first-stage predictions, on the device
    (C-ABI fcn_prepare_inputs_refine).  Mirrors datasets/provider_sample_refine.py::ProviderDataset.__getitem__ + collate_fn:
    per-sample window counts differ, center_ref* / cls_label are edge-padded to the batch maximum.  The batch maxima
    (tensor shapes) are decided on the host from the predicted box widths -- B numbers -- everything per point / per window
    runs in the kernel."""

    def __init__(self, npoints, strides=None, random_flip=False, random_shift=False, one_hot=True, device="cuda"):
        self.npoints = int(npoints)
        self.strides = tuple(float(s) for s in (cfg.DATA.STRIDE if strides is None else strides))
        assert len(self.strides) == 4
        self.random_flip, self.random_shift, self.one_hot = bool(random_flip), bool(random_shift), bool(one_hot)
        self.device = torch.device(device)
        self.classes = DATASET_INFO[cfg.DATA.DATASET_NAME].CLASSES
        if not cfg.DATA.RTC:
            # provider_sample_refine.py:225-262: without RTC generate_ref() runs on the UN-rotated predicted box (z extent, a
            # line through the box) and rot_angle / ref_center are zeros -- a different geometry from the kernel's
            raise NotImplementedError("RefineInputBuilder implements the cfg.DATA.RTC = True geometry only (every shipped "
                                      "refine cfg sets it: cfgs/refine_car.yaml, cfgs/refine_people.yaml)")

    def alloc(self, B, lpad, with_labels=True):
        """Output tensors of launch() for a batch of B samples at the padded window counts lpad (four ints), zero-filled (pass as
        `out` to write the same buffers every step)."""
        dev, N = self.device, self.npoints
        f32 = dict(dtype=torch.float32, device=dev)
        out = {"point_cloud": torch.zeros((B, 3, N), **f32), "rot_angle": torch.zeros((B, 1), **f32),
               "ref_center": torch.zeros((B, 3), **f32), "lens": torch.zeros((B, 4), dtype=torch.int32, device=dev)}
        if with_labels:
            out.update(cls_label=torch.zeros((B, lpad[1]), dtype=torch.int64, device=dev),
                       box3d_center=torch.zeros((B, 3), **f32), box3d_heading=torch.zeros((B, 1), **f32),
                       box3d_size=torch.zeros((B, 3), **f32))
        for s in range(4):
            out["center_ref%d" % (s + 1)] = torch.zeros((B, 3, lpad[s]), **f32)
        return out

    def launch(self, t, out, pt_stride, lpad, with_labels=True):
        """ONE launch of fcn_prepare_inputs_refine on the current stream: the device tensors `t` (raw, off, choice, pcorners, pangle,
        psize; with labels also corners, heading, size, coin, normal) -> `out` (alloc(B, lpad, with_labels)).  No allocation, no
        host read: capturable into a hipGraph.  Returns `out`."""
        from ._native import InpRefineDesc
        dev, p = self.device, _ptr
        desc, refs = _desc_refs(InpRefineDesc, int(out["point_cloud"].shape[0]), self.npoints, pt_stride, lpad, self.strides, out,
                                1 if (self.random_flip and with_labels) else 0, 1 if (self.random_shift and with_labels) else 0)
        lab = (lambda k: p(t.get(k))) if with_labels else (lambda k: None)
        olab = (lambda k: p(out.get(k))) if with_labels else (lambda k: None)
        with torch.cuda.device(dev):
            _native.check(_native.lib().fcn_prepare_inputs_refine(
                ctypes.byref(desc), p(t["raw"]), p(t["off"]), p(t["choice"]), p(t["pcorners"]), p(t["pangle"]), p(t["psize"]),
                lab("corners"), lab("heading"), lab("size"), lab("coin"), lab("normal"),
                p(out["point_cloud"]), refs, olab("cls_label"), olab("box3d_center"), olab("box3d_heading"),
                olab("box3d_size"), p(out["rot_angle"]), p(out["ref_center"]), p(out["lens"]),
                _native.current_stream(dev)), "fcn_prepare_inputs_refine")
        return out

    def _launch(self, t, B, pt_stride, Lpad, with_labels):
        """alloc() + launch() on the device tensors `t`: the part build(), build_device() and build_device_train() share."""
        out = self.launch(t, self.alloc(B, Lpad, with_labels), pt_stride, Lpad, with_labels)
        _record(t, self.device)
        return out

    def _lpad(self, widths):
        """Batch maxima of len(np.arange(-w/2, w/2, s)) over the predicted widths: the padded widths of the outputs.
        A width that is not a positive finite number (untrained first-stage weights can decode one) has no window on any
        stride: the reference's collate cannot pad such a sample, and the kernel would leave its cls_label row unwritten --
        refused here, where build(), build_device() and build_device_train() all pass."""
        widths = np.asarray(widths, dtype=np.float64).reshape(-1)
        for i, w in enumerate(widths):
            if not (w > 0.0 and np.isfinite(w)):
                raise ValueError("RefineInputBuilder: sample %d has predicted width %r: no window on any stride "
                                 "(fcn_prepare_inputs_refine needs every pred_size width > 0)" % (i, float(w)))
        return [int(max(len(np.arange(-w / 2.0, w / 2.0, s)) for w in widths)) for s in self.strides]

    def build_device(self, cands, types, prob=None, draws=None):
        """The inference batch (build(..., with_labels=False)) straight from the device tensors of cascade.refine_candidates:
        no point leaves the device.  cands: its dict (points, off, pred_box3d, pred_angle, pred_size, score on the device,
        counts on the host); types: the class name of each of the D candidates; prob: their 'rgb_prob' (D) when it is not the
        first-stage score (the reference's result files carry exactly that score); draws: (choice (B,N) int32, coin, normal)
        for the B surviving candidates, or None to draw like draw_refine from their counts.
        Candidates without a point are dropped before the launch (prepare_data_refine.py:739-741, lidar_point_threshold = 1);
        'kept' (B,) int64 (host) lists the survivors' candidate indices.  The host reads D numbers here: the predicted widths,
        which decide the padded window counts.  With no survivor the dict holds 'kept' alone."""
        _need_device(self.device)
        counts = np.asarray(cands["counts"], dtype=np.int64)
        D, N = len(counts), self.npoints
        if len(types) != D or (prob is not None and len(prob) != D):
            raise ValueError("build_device: %d candidates, %d types%s" % (D, len(types), "" if prob is None else ", %d prob" % len(prob)))
        kept = np.nonzero(counts > 0)[0]
        B = len(kept)
        if B == 0:
            return {"kept": kept}
        if draws is None:
            draws = draw_refine(counts[kept], N, False, False)
        dev = self.device
        widths = cands["pred_size"][:, 1].cpu().numpy()                       # D numbers: the tensor shapes depend on them
        sel = None if B == D else _up(kept, dev)
        pick = lambda x: x.contiguous() if sel is None else x.index_select(0, sel).contiguous()
        off = cands["off"]
        if isinstance(draws, DeviceDraws):
            draws = draws.draw(pick(_row_counts(off)), N, False, False)
        t = {"raw": cands["points"], "choice": _draw_tensors(draws, dev, 1)[0],
             # the kernel reads a sample's first row only: the survivors' starts (+ the end of the last one, for the (B+1) form)
             "off": off if sel is None else torch.cat([off.index_select(0, sel), off[int(kept[-1]) + 1:int(kept[-1]) + 2]]),
             "pcorners": pick(cands["pred_box3d"]), "pangle": pick(cands["pred_angle"]), "psize": pick(cands["pred_size"])}
        out = self._launch(t, B, int(cands["points"].shape[1]), self._lpad(widths[kept]), False)
        _class_rows(self, out, [types[i] for i in kept], size_class=False)
        if prob is None:
            out["rgb_prob"] = pick(cands["score"]).to(torch.float32).reshape(B, 1)
        else:
            out["rgb_prob"] = _up(np.asarray(prob, dtype=np.float32)[kept].reshape(B, 1), dev)
        out["kept"] = kept
        return out

    def build_device_train(self, sel, types, draws=None):
        """The TRAINING batch -- the dict of build(records, with_labels=True), same keys, shapes and dtypes -- straight from the
        device tensors of cascade.refine_training_candidates: no point, corner or label box leaves the device.  sel: its dict;
        types: the class name of each of the D CANDIDATES (a kept unit's is looked up through sel["unit_cand"]); draws: (choice
        (K,N) int32, coin (K), normal (K)) for the K kept units, or None to draw like draw_refine from their counts under the
        builder's random_flip / random_shift.  The host reads K numbers here: the predicted widths, which decide the padded
        window counts.  ONE launch of fcn_prepare_inputs_refine.  With no kept unit the dict holds 'kept' alone."""
        _need_device(self.device)
        kept = np.asarray(sel["kept"], dtype=np.int64)
        K = len(kept)
        if K == 0:
            return {"kept": kept}
        if draws is None:
            draws = draw_refine(sel["counts"], self.npoints, self.random_flip, self.random_shift)
        dev = self.device
        if isinstance(draws, DeviceDraws):
            draws = draws.draw(_row_counts(sel["off"]), self.npoints, self.random_flip, self.random_shift)
        choice, coin, normal = _draw_tensors(draws, dev, 3)
        widths = sel["pred_size"][:, 1].cpu().numpy()                         # K numbers: the tensor shapes depend on them
        t = {"raw": sel["points"], "off": sel["off"], "choice": choice,
             "pcorners": sel["pred_box3d"].reshape(K, 24), "pangle": sel["pred_angle"], "psize": sel["pred_size"],
             "corners": sel["box3d"].reshape(K, 24), "heading": sel["heading"], "size": sel["size"],
             "coin": coin, "normal": normal}
        out = self._launch(t, K, int(sel["points"].shape[1]), self._lpad(widths), True)
        _class_rows(self, out, [types[i] for i in sel["unit_cand"]])
        return out

    def build(self, records, draws=None, with_labels=True):
        """records: dicts with REFINE_KEYS (points (n,>=3) float32 rect camera coordinates; box3d (8,3), heading, size (l,w,h)
        of the label box; pred_box3d (8,3), pred_angle, pred_size of the first-stage prediction; type).  Returns the batch
        dict on the device (+ 'lens' (B,4) int32: the per-sample window counts before padding)."""
        _need_device(self.device)
        B, N = len(records), self.npoints
        counts = [len(r["points"]) for r in records]
        if draws is None:
            draws = draw_refine(counts, N, self.random_flip and with_labels, self.random_shift and with_labels)
        pt_stride = int(records[0]["points"].shape[1])
        h = _pack(records, counts, (("pcorners", "pred_box3d", (24,)), ("pangle", "pred_angle", ()), ("psize", "pred_size", (3,))))
        # batch maxima of len(np.arange(-w/2, w/2, s)): the padded widths of the outputs
        Lpad = self._lpad(h["psize"][:, 1])
        dev = self.device
        t = {k: _up(v, dev) for k, v in h.items()}
        if isinstance(draws, DeviceDraws):
            draws = draws.draw(_row_counts(t["off"]), N, self.random_flip and with_labels, self.random_shift and with_labels)
        choice, coin, normal = _draw_tensors(draws, dev, 3)
        t["choice"] = choice
        if with_labels:
            labels = _stacks(records, (("corners", "box3d", (24,)), ("heading", "heading", ()), ("size", "size", (3,))))
            t.update({k: _up(v, dev) for k, v in labels.items()}, coin=coin, normal=normal)
        out = self._launch(t, B, pt_stride, Lpad, with_labels)
        names = [r["type"] for r in records]
        if not (with_labels or self.one_hot):
            [self.classes.index(n) for n in names]                 # this path refuses an unknown class whatever it writes
        _class_rows(self, out, names, size_class=with_labels)
        if not with_labels:
            # from_rgb_detection path (provider_sample_refine.py:404-419): the 2-D detector's score travels with the sample and
            # becomes the detection score's prior in detect() (train/test_net_det.py:214,279)
            out["rgb_prob"] = _up(np.asarray([float(r.get("prob", 1.0)) for r in records], dtype=np.float32).reshape(B, 1), dev)
        return out


def refine_records_from_fixture(g):
    """tests/golden/inputs_refine_b6.npz (make_golden_inputs_refine.py) as a list of records."""
    offs = np.concatenate([[0], np.cumsum(g["raw_counts"])])
    recs = []
    for b in range(len(g["raw_counts"])):
        sl = slice(int(offs[b]), int(offs[b + 1]))
        recs.append({"points": g["raw_points"][sl], "box3d": g["box3d_corners"][b], "heading": float(g["heading"][b]),
                     "size": g["size"][b], "pred_box3d": g["pred_corners"][b], "pred_angle": float(g["pred_angle"][b]),
                     "pred_size": g["pred_size"][b], "type": "Car"})
    return recs
