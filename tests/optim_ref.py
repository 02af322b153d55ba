"""fp64 restatement of the optimiser kernels of csrc/optim.hip (adam_kernel, sgd_kernel) with an A-PRIORI elementwise error
bound, plus the seeded inputs the tests of tests/test_gpu_optim.py and tests/test_optim_referee.py share.  Plain numpy, no
import from the package.

Arithmetic: torch.optim.Adam (L2 weight decay folded into the gradient, lerp form of the first moment, eps added after the
bias-corrected square root) and torch.optim.SGD (dampening 0, no Nesterov):
    g' = wd*p + g*gs
    m' = m + (g' - m)(1 - b1)             v' = b2*v + (1 - b2) g'^2
    p' = p - lr/(1 - b1^(t+1)) * m' / (sqrt(v') / sqrt(1 - b2^(t+1)) + eps)          t = steps already done for the element
    buf' = mu*buf + g'                    p' = p - lr*buf'
The state (p, g, m, v) is the fp32 state BEFORE the step promoted exactly to fp64; the hyper-parameters are the float32-rounded
values promoted to fp64, because the kernel reads fp32 from device memory.

Error bound.  The kernel evaluates the expression in fp32, one correctly rounded operation at a time (build.py compiles with
-fno-fast-math -ffp-contract=off: no fused multiply-add, no reassociation; hipcc's default keeps fp32 division and sqrtf
correctly rounded; fp32 subnormals are kept on gfx9).  Every value below carries (fp64 value, bound on |fp32 value - fp64
value|); each fp32 operation of the kernel, IN THE ORDER THE KERNEL WRITES IT, propagates the bounds of its operands to first
order and adds u = 2^-24 times the absolute values of its terms (|a| + |b| for a sum or difference, |result| for a product,
quotient or square root).  The error of v' enters the square root with 1/(2 v') relative, zero where v' = 0 (then g' = 0 and
v = 0 exactly and the kernel's value is exact too).  Rounded operations per output element:
    Adam   g'  3 (wd*p, g*gs, +)                      m'  g' + 4 (g'-m, 1-b1, *, +)        v'  g' + 5 (v*b2, 1-b2, *g', *g', +)
           p'  m', v' + 12: two bias corrections (the fp64 pow -- 2^-52 relative -- and its rounding to fp32), lr/bc1, sqrt(bc2),
               1/., sqrt(v'), *, +eps, m'/., lr_c*., p-.
    SGD    buf' 5 (mu*buf, wd*p, g*gs, +, +)          p'  buf' + 2 (lr*buf', p-.)
The propagated bound is multiplied by SAFETY = 2 (second-order terms; not 4: neither sqrtf nor the division is approximate in
the product build, see the flags above) and an absolute 2^-126 is added (a product that lands in the subnormal range is rounded
to a multiple of 2^-149 and no longer to relative u; the test inputs keep every intermediate of g'^2 normal or exactly 0, the
floor covers what is left).  No constant here is fitted to a kernel's output.

`variant` selects one deliberately WRONG formulation (values only matter then): tests/test_optim_referee.py shows that each
lies at least 100 bounds away from the right one on the inputs the GPU tests use, so a GPU test that passes excludes it."""
import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -126
SAFETY = 2.0
STEP_SPAN = 2048            # elements per workgroup of adam_kernel: 256 threads x 2 four-vectors

ADAM_VARIANTS = ("bc_late", "no_bc2", "eps_in_sqrt", "adamw", "no_gs")
SGD_VARIANTS = ("wd_after", "lr_on_grad")


class _V:
    """fp64 value(s) + bound on the distance of the kernel's fp32 value from it."""
    __slots__ = ("x", "e")

    def __init__(self, x, e=0.0):
        self.x = np.asarray(x, dtype=np.float64)
        self.e = np.asarray(e, dtype=np.float64)


def _add(a, b):
    return _V(a.x + b.x, a.e + b.e + U * (np.abs(a.x) + np.abs(b.x)))


def _sub(a, b):
    return _V(a.x - b.x, a.e + b.e + U * (np.abs(a.x) + np.abs(b.x)))


def _mul(a, b):
    x = a.x * b.x
    return _V(x, np.abs(a.x) * b.e + np.abs(b.x) * a.e + a.e * b.e + U * np.abs(x))


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        x = a.x / b.x
        return _V(x, (a.e + np.abs(x) * b.e) / (np.abs(b.x) - b.e) + U * np.abs(x))


def _sqrt(a):
    x = np.sqrt(a.x)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(a.x > 0, a.e / (2.0 * a.x) * x, 0.0)
    return _V(x, e + U * x)


def _bias_correction(b, tt):
    """1 - b^tt as the kernel has it: pow() and the subtraction in fp64 (2^-52 relative each), the result rounded to fp32."""
    with np.errstate(divide="ignore", invalid="ignore"):
        pw = np.power(b, tt)
    x = 1.0 - pw
    return _V(x, U * np.abs(x) + 2.0 ** -52 * (1.0 + np.abs(pw)))


def _bound(v):
    return SAFETY * v.e + FLOOR


def _hyper(h, n):
    h = np.asarray(h, dtype=np.float32).astype(np.float64)
    assert h.shape == (n,), h.shape
    return [_V(x) for x in h]


def adam_step(p, g, m, v, hyper6, t, variant=None):
    """One Adam step of every element.  p, g, m, v: the fp32 state before the step (any float array, promoted to fp64); hyper6:
    lr, beta1, beta2, eps, weight_decay, grad_scale; t: steps already done (scalar or one per element).
    Returns (p', m', v'), (bound_p, bound_m, bound_v)."""
    assert variant is None or variant in ADAM_VARIANTS, variant
    lr, b1, b2, eps, wd, gs = _hyper(hyper6, 6)
    p, g, m, v = (_V(np.asarray(a, dtype=np.float64)) for a in (p, g, m, v))
    t = np.asarray(t, dtype=np.float64)
    one = _V(1.0)
    gsc = g if variant == "no_gs" else _mul(g, gs)
    gp = gsc if variant == "adamw" else _add(_mul(wd, p), gsc)
    m1 = _add(m, _mul(_sub(gp, m), _sub(one, b1)))
    v1 = _add(_mul(v, b2), _mul(_mul(_sub(one, b2), gp), gp))
    tt = t if variant == "bc_late" else t + 1.0
    lr_c = _div(lr, _bias_correction(b1.x, tt))
    rsq = one if variant == "no_bc2" else _div(one, _sqrt(_bias_correction(b2.x, tt)))
    if variant == "eps_in_sqrt":
        den = _sqrt(_add(_mul(v1, _mul(rsq, rsq)), eps))
    else:
        den = _add(_mul(_sqrt(v1), rsq), eps)
    with np.errstate(invalid="ignore"):
        upd = _mul(lr_c, _div(m1, den))
        p0 = _mul(p, _sub(one, _mul(lr, wd))) if variant == "adamw" else p
        p1 = _sub(p0, upd)
    return (p1.x, m1.x, v1.x), (_bound(p1), _bound(m1), _bound(v1))


def sgd_step(p, g, buf, hyper4, variant=None):
    """One SGD step.  hyper4: lr, momentum, weight_decay, grad_scale.  Returns (p', buf'), (bound_p, bound_buf)."""
    assert variant is None or variant in SGD_VARIANTS, variant
    lr, mu, wd, gs = _hyper(hyper4, 4)
    p, g, buf = (_V(np.asarray(a, dtype=np.float64)) for a in (p, g, buf))
    if variant == "wd_after":               # weight decay applied to the parameter behind the momentum update
        b1 = _add(_mul(mu, buf), _mul(g, gs))
        p1 = _sub(p, _mul(lr, _add(b1, _mul(wd, p))))
    elif variant == "lr_on_grad":           # lr scales the gradient entering the buffer instead of the buffer
        b1 = _add(_mul(mu, buf), _mul(lr, _add(_mul(wd, p), _mul(g, gs))))
        p1 = _sub(p, b1)
    else:
        b1 = _add(_mul(mu, buf), _add(_mul(wd, p), _mul(g, gs)))
        p1 = _sub(p, _mul(lr, b1))
    return (p1.x, b1.x), (_bound(p1), _bound(b1))


# ------------------------------------------------------------------------------------------------
# what the GPU tests and their referee share: sizes, hyper-parameter schedules, seeded inputs

# on and around every edge of adam_kernel: a workgroup covers 2048 elements, its second four-vector starts at element 1024,
# the scalar tail is n & 3, out-of-range loads are clamped to the last four-vector
SIZES = (4, 5, 6, 7, 1023, 1024, 1025, 2044, 2047, 2048, 2049, 2051, 2052, 4095, 4096, 4097, 3 * 2048 + 1027)

# three consecutive steps; the values are rewritten in device memory between them.  lr, beta1, beta2, eps, weight_decay, grad_scale
ADAM_HYPER = ((1e-3, 0.9, 0.999, 1e-8, 1e-4, 0.125),
              (0.0, 0.9, 0.999, 1e-8, 0.0, 1.0),
              (3e-4, 0.85, 0.99, 1e-8, 1e-4, 0.125))
# lr, momentum, weight_decay, grad_scale
SGD_HYPER = ((1e-2, 0.9, 1e-4, 0.125),
             (5e-3, 0.0, 0.0, 1.0),
             (3e-3, 0.9, 1e-4, 0.125))

SLOT_VALUES = (0, 3, 10000, 1)          # starting step counts, a different one per workgroup


def adam_blocks(n):
    """fcn_adam_step_slots(n) restated: workgroups (= step slots) of one launch over n elements."""
    return 0 if n < 4 else ((n >> 2) + 511) // 512


def slot_init(n):
    return np.array([SLOT_VALUES[(w + n) % 4] for w in range(adam_blocks(n))], dtype=np.int64)


def element_slots(n):
    """Index of the step slot every element is updated with: its workgroup's, and workgroup 0's for the n & 3 tail."""
    s = np.arange(n) // STEP_SPAN
    s[(n >> 2) << 2:] = 0
    return s


def gradients(rng, n):
    """Per-element magnitudes 10^U(-6, 3) times a normal draw, about 5 % exact zeros; |g| >= 1e-10 otherwise (with |p| >= 1e-6
    below that keeps (1 - b2) g'^2 a normal fp32 number for every schedule above -- normal_range_ok() checks it)."""
    mag = 10.0 ** rng.uniform(-6.0, 3.0, n)
    g = mag * rng.standard_normal(n)
    g = np.where(np.abs(g) < 1e-10, np.copysign(1e-10, g), g)
    g[rng.random(n) < 0.05] = 0.0
    return g.astype(np.float32), mag


def make_inputs(n, seed):
    """p ~ N(0, 1); g as gradients(); m and v non-zero and of the gradients' scale.  float32 arrays p, g, m, v (SGD: m is the
    momentum buffer)."""
    rng = np.random.default_rng([seed, n])
    g, mag = gradients(rng, n)
    p = rng.standard_normal(n)
    p = np.where(np.abs(p) < 1e-6, np.copysign(1e-6, p), p)
    m = 0.3 * mag * rng.standard_normal(n)
    m = np.where(m == 0, 0.3 * mag, m)
    v = mag * mag * rng.uniform(0.25, 1.0, n)
    return p.astype(np.float32), g, m.astype(np.float32), v.astype(np.float32)


def normal_range_ok(p, g, hyper, adam=True):
    """True when every intermediate of g'^2 is a normal fp32 number or exactly 0 (Adam), g' itself for SGD."""
    h = np.asarray(hyper, dtype=np.float32).astype(np.float64)
    wd, gs, omb2 = (h[4], h[5], 1.0 - h[2]) if adam else (h[2], h[3], 1.0)
    gp = np.abs(wd * np.asarray(p, np.float64) + np.asarray(g, np.float64) * gs)
    tiny = 2.0 ** -125
    small = np.minimum(gp, omb2 * gp * gp if adam else gp)
    return bool(np.all((gp == 0) | (small >= tiny)))
