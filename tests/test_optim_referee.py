"""Who checks the checker: tests/optim_ref.py (the fp64 restatement of csrc/optim.hip and its a-priori error bound, which
tests/test_gpu_optim.py holds the kernels to) against torch.optim.Adam / torch.optim.SGD in fp64, against a numpy float32
restatement of the kernels' own operation order, and against deliberately wrong formulations -- each must lie at least 100
bounds away on the inputs the GPU tests use, so a GPU test that passes excludes it.  CPU only."""
import numpy as np
import pytest
import torch

import optim_ref as R

f32 = np.float32


def _torch_stream(n, steps, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    grads = [torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** torch.empty(n, dtype=torch.float64).uniform_(-4, 2, generator=g)
             for _ in range(steps)]
    return p0, grads


def _close(got, want, what):
    want = want.detach().numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (what, np.abs(got - want).max(), np.abs(want).max())


@pytest.mark.parametrize("lr,betas,eps,wd,gs", [(1e-3, (0.9, 0.999), 1e-8, 0.0, 1.0),
                                                (1e-3, (0.9, 0.999), 1e-8, 1e-4, 0.125),
                                                (2.5e-2, (0.8, 0.95), 1e-6, 1e-2, 0.5)])
def test_restatement_is_torch_adam_in_fp64(lr, betas, eps, wd, gs):
    n = 257
    p0, grads = _torch_stream(n, 50, 1)
    # the restatement takes the float32-rounded hyper-parameters: torch gets the same numbers
    h = [float(f32(x)) for x in (lr, betas[0], betas[1], eps, wd, gs)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=h[0], betas=(h[1], h[2]), eps=h[3], weight_decay=h[4])
    p, m, v = p0.numpy().copy(), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads):
        ref.grad = g * h[5]                     # the gradient scale applied beforehand
        opt.step()
        (p, m, v), _ = R.adam_step(p, g.numpy(), m, v, h, t)
        _close(p, ref, ("p", t))
        _close(m, opt.state[ref]["exp_avg"], ("m", t))
        _close(v, opt.state[ref]["exp_avg_sq"], ("v", t))


@pytest.mark.parametrize("lr,mu,wd,gs", [(1e-2, 0.9, 0.0, 1.0), (1e-2, 0.9, 1e-4, 0.125), (3e-3, 0.0, 1e-2, 0.5), (5e-2, 0.5, 1e-3, 0.25)])
def test_restatement_is_torch_sgd_in_fp64(lr, mu, wd, gs):
    n = 257
    p0, grads = _torch_stream(n, 50, 2)
    h = [float(f32(x)) for x in (lr, mu, wd, gs)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([ref], lr=h[0], momentum=h[1], weight_decay=h[2])
    p, buf = p0.numpy().copy(), np.zeros(n)
    for t, g in enumerate(grads):
        ref.grad = g * h[3]
        opt.step()
        (p, buf), _ = R.sgd_step(p, g.numpy(), buf, h)
        _close(p, ref, ("p", t))
        if mu > 0:                              # (torch keeps no buffer with momentum 0)
            _close(buf, opt.state[ref]["momentum_buffer"], ("buf", t))


# ------------------------------------------------------------------------------------------------
# numpy float32 in the kernels' own operation order (csrc/optim.hip: adam_moments, adam_kernel, sgd_kernel)

def adam_f32(p, g, m, v, hyper, t):
    lr, b1, b2, eps, wd, gs = (f32(x) for x in hyper)
    one = f32(1)
    tt = np.asarray(t, dtype=np.float64) + 1.0
    bc1 = (1.0 - np.power(np.float64(b1), tt)).astype(f32)
    bc2 = (1.0 - np.power(np.float64(b2), tt)).astype(f32)
    gp = wd * p + g * gs
    m1 = m + (gp - m) * (one - b1)
    v1 = v * b2 + (one - b2) * gp * gp
    lr_c, rsq = lr / bc1, one / np.sqrt(bc2)
    p1 = p - lr_c * (m1 / (np.sqrt(v1) * rsq + eps))
    assert p1.dtype == f32 and m1.dtype == f32 and v1.dtype == f32
    return p1, m1, v1


def sgd_f32(p, g, buf, hyper):
    lr, mu, wd, gs = (f32(x) for x in hyper)
    b = mu * buf + (wd * p + g * gs)
    p1 = p - lr * b
    assert p1.dtype == f32 and b.dtype == f32
    return p1, b


def _ratio(got, want, bound):
    """Worst |got - want| / bound; a non-finite value of a wrong variant counts as infinitely far."""
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(got, dtype=np.float64) - want)
    d = np.where(np.isfinite(d), d, np.inf)
    return float((d / bound).max())


def _adam_walk():
    """The float32 trajectory over every size and schedule of the GPU test: yields the state before each step and after it."""
    for n in R.SIZES:
        p, g, m, v = R.make_inputs(n, 0)
        slots = R.slot_init(n)
        el = R.element_slots(n)
        for k, h in enumerate(R.ADAM_HYPER):
            if k:
                g, _ = R.gradients(np.random.default_rng([7, n, k]), n)
            assert R.normal_range_ok(p, g, h)
            t = slots[el]
            new = adam_f32(p, g, m, v, h, t)
            yield n, k, h, t, (p, g, m, v), new
            p, m, v = new
            slots = slots + 1


def _sgd_walk():
    for n in R.SIZES:
        p, g, buf, _ = R.make_inputs(n, 0)
        for k, h in enumerate(R.SGD_HYPER):
            if k:
                g, _ = R.gradients(np.random.default_rng([7, n, k]), n)
            assert R.normal_range_ok(p, g, h, adam=False)
            new = sgd_f32(p, g, buf, h)
            yield n, k, h, (p, g, buf), new
            p, buf = new


def test_float32_restatement_stays_inside_the_bound():
    worst = {"adam": 0.0, "sgd": 0.0}
    for n, k, h, t, (p, g, m, v), new in _adam_walk():
        want, bound = R.adam_step(p, g, m, v, h, t)
        for got, w, b, what in zip(new, want, bound, "pmv"):
            r = _ratio(got, w, b)
            assert r <= 1.0, ("adam", n, k, what, r)
            worst["adam"] = max(worst["adam"], r)
        if h[0] == 0.0:
            assert np.array_equal(new[0], p)
    for n, k, h, (p, g, buf), new in _sgd_walk():
        want, bound = R.sgd_step(p, g, buf, h)
        for got, w, b, what in zip(new, want, bound, ("p", "buf")):
            r = _ratio(got, w, b)
            assert r <= 1.0, ("sgd", n, k, what, r)
            worst["sgd"] = max(worst["sgd"], r)
    print("numpy float32 restatement, worst error / bound: adam %.3f  sgd %.3f" % (worst["adam"], worst["sgd"]))


def test_wrong_variants_lie_outside_the_bound():
    far = {}
    for n, k, h, t, (p, g, m, v), _ in _adam_walk():
        want, bound = R.adam_step(p, g, m, v, h, t)
        for var in R.ADAM_VARIANTS:
            wrong, _ = R.adam_step(p, g, m, v, h, t, variant=var)
            far[var] = max(far.get(var, 0.0), max(_ratio(x, w, b) for x, w, b in zip(wrong, want, bound)))
    for n, k, h, (p, g, buf), _ in _sgd_walk():
        want, bound = R.sgd_step(p, g, buf, h)
        for var in R.SGD_VARIANTS:
            wrong, _ = R.sgd_step(p, g, buf, h, variant=var)
            far[var] = max(far.get(var, 0.0), max(_ratio(x, w, b) for x, w, b in zip(wrong, want, bound)))
    finite = {k: v for k, v in far.items() if np.isfinite(v)}
    print("wrong variants, largest distance in bounds: " + "  ".join("%s %.3g" % kv for kv in sorted(far.items())))
    print("smallest over the variants: %.3g" % min(far.values()), "(finite ones: %.3g)" % min(finite.values()) if finite else "")
    assert set(far) == set(R.ADAM_VARIANTS + R.SGD_VARIANTS)
    for var, r in far.items():
        assert r >= 100.0, (var, r)


def test_wrong_bias_correction_shows_at_finite_values_too():
    """bc_late divides by 1 - b^0 = 0 where no step was done (an infinite distance above); where steps were done the distance is
    finite and still far outside the bound."""
    p, g, m, v = R.make_inputs(2048, 0)
    h = R.ADAM_HYPER[0]
    want, bound = R.adam_step(p, g, m, v, h, 3)
    wrong, _ = R.adam_step(p, g, m, v, h, 3, variant="bc_late")
    r = _ratio(wrong[0], want[0], bound[0])
    print("bc_late at t = 3: %.3g bounds" % r)
    assert np.isfinite(r) and r >= 100.0, r
