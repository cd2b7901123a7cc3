"""The pieces the device L-BFGS and L-BFGS-B share (``optim/_quasi_newton.py``): the line
search against the recorded steps of the two loops it replaced, the pair ring's bookkeeping,
and the one replicated objective."""
import gc
import json
import math
import os

import numpy as np
import pytest
import torch

from multigrad_amd.optim._quasi_newton import PairRing, strong_wolfe
from multigrad_amd.optim.lbfgs import GenericObjective
from multigrad_amd.optim.lbfgsb import BoxObjective

INF = math.inf

# ---------------------------------------------------------------------------- the search
# phi(a) -> (value, slope) in host float64 with + - * / and math.sqrt only, so the recorded
# steps do not depend on a libm.  `pole` as specified never shows a non-finite value (its value
# at 2 already fails the decrease test, so no search reaches 2.5); `pole_wide` is the same
# shape with the pole at 3.5, which the doubling from 2 to 4 steps over.
FUNCS = {
    "quad_far": lambda a: ((a - 5.0) * (a - 5.0), 2.0 * (a - 5.0)),
    "quad_near": lambda a: ((a - 0.3) * (a - 0.3), 2.0 * (a - 0.3)),
    "quartic": lambda a: ((a - 1.5) * (a - 1.5) * (a - 1.5) * (a - 1.5) - 2.0 * a,
                          4.0 * (a - 1.5) * (a - 1.5) * (a - 1.5) - 2.0),
    "rational": lambda a: (-a / (1.0 + a * a),
                           (a * a - 1.0) / ((1.0 + a * a) * (1.0 + a * a))),
    "sqrtwell": lambda a: (math.sqrt(1.0 + 100.0 * (a - 0.7) * (a - 0.7)),
                           100.0 * (a - 0.7) / math.sqrt(1.0 + 100.0 * (a - 0.7) * (a - 0.7))),
    "ascent": lambda a: (a + a * a, 1.0 + 2.0 * a),
    "pole": lambda a: (INF, INF) if a >= 2.5 else (1.0 / (2.5 - a) - a,
                                                    1.0 / ((2.5 - a) * (2.5 - a)) - 1.0),
    "pole_wide": lambda a: (INF, INF) if a >= 3.5 else (1.0 / (3.5 - a) - a,
                                                         1.0 / ((3.5 - a) * (3.5 - a)) - 1.0),
    "flatslope": lambda a: (-1e-3 * a + 1e-9 * a * a, -1e-3 + 2e-9 * a),
}

with open(os.path.join(os.path.dirname(__file__), "golden", "strong_wolfe_steps.json")) as _fh:
    GOLDEN = json.load(_fh)


def test_golden_cases_reach_every_exit():
    """Every function at a1 in {1, 0.125}, c2 in {0.9, 0.1}, in both forms (the ascent only in
    the deferred form: the unbounded driver never searches along one)."""
    cases = GOLDEN["cases"]
    want = {(f, a1, c2, form) for f in FUNCS for a1 in (1.0, 0.125) for c2 in (0.9, 0.1)
            for form in ("float", "deferred") if not (f == "ascent" and form == "float")}
    assert {(c["function"], c["a1"], c["c2"], c["form"]) for c in cases} == want
    assert len(cases) == len(want) == 68
    assert {c["exit"] for c in cases} == {
        "accept_first", "accept_doubled", "zoom_decrease", "zoom_slope", "zoom_nonfinite",
        "cap_accept", "ascent_none", "maxls"}


@pytest.mark.parametrize("case", GOLDEN["cases"],
                         ids=lambda c: f"{c['function']}-{c['a1']}-{c['c2']}-{c['form']}")
def test_strong_wolfe_probes_the_recorded_steps(case):
    """The same float64 steps and the same result as the loop it replaced: the unbounded
    driver's inline loop (float slope, no cap) and L-BFGS-B's (deferred slope, cap 1)."""
    fn = FUNCS[case["function"]]
    f0, d0 = fn(0.0)
    steps = []

    def phi(a):
        steps.append(float(a))
        return fn(a)

    if case["form"] == "float":
        got = strong_wolfe(phi, f0, d0, case["a1"], GOLDEN["c1"], case["c2"], GOLDEN["maxls"])
    else:
        def slope():
            assert len(steps) == 1  # read after the first evaluation, and only once
            return d0
        got = strong_wolfe(phi, f0, slope, case["a1"], GOLDEN["c1"], case["c2"], GOLDEN["maxls"],
                           amax=1.0)
    assert steps == case["steps"]
    assert got == case["result"]


# ---------------------------------------------------------------------------- the ring
def test_pair_ring_bookkeeping():
    """Seven pairs through a ring of m = 3; the fourth has s.y < 0 and the sixth y = 0.  The
    pairs are small integers, so every inner product is exact whatever the summation order."""
    m, n = 3, 6
    R = m + 1
    rng = np.random.default_rng(0)
    ring = PairRing(m, n, torch.device("cpu"))
    assert ring.HS.shape == (2 * R, n) and ring.HX.shape == (2 * R, n)
    assert PairRing(m, n, torch.device("cpu"), extra_rows=1).HX.shape == (2 * R + 1, n)
    S, Y = np.zeros((R, n)), np.zeros((R, n))
    for i in range(7):
        s = rng.integers(1, 5, size=n).astype(np.float64)
        y = s + rng.integers(0, 3, size=n)
        if i == 3:
            y = -y
        if i == 5:
            y = np.zeros(n)
        q = ring.spare()
        assert q not in ring.order and 0 <= q < R
        before = (list(ring.order), ring.SY.copy(), ring.SS.copy(), ring.YY.copy(),
                  ring.gamma, ring.theta)
        S[q], Y[q] = s, y
        HS = np.concatenate([S, Y])
        dots = np.stack([HS @ s, HS @ y], 1)
        ok = ring.accept(q, dots)
        assert ok == (i not in (3, 5))
        if not ok:
            assert ring.order == before[0] and (ring.gamma, ring.theta) == before[4:]
            for a, b in zip((ring.SY, ring.SS, ring.YY), before[1:4]):
                np.testing.assert_array_equal(a, b)
            continue
        assert ring.order == (before[0] + [q])[-m:]          # oldest first, at most m
        assert len(set(ring.order)) == len(ring.order) <= m
        assert ring.spare() not in ring.order
        o = np.ix_(ring.order, ring.order)
        So, Yo = S[ring.order], Y[ring.order]
        np.testing.assert_array_equal(ring.SY[o], So @ Yo.T)
        np.testing.assert_array_equal(ring.SS[o], So @ So.T)
        np.testing.assert_array_equal(ring.YY[o], Yo @ Yo.T)
        assert ring.gamma == (s @ y) / (y @ y) and ring.theta == (y @ y) / (s @ y)
        assert abs(ring.gamma * ring.theta - 1.0) <= np.finfo(np.float64).eps
    assert len(ring.order) == m


def test_pair_ring_lincomb_reuses_one_buffer():
    ring = PairRing(2, 5, torch.device("cpu"))
    ring.HS.copy_(torch.arange(30, dtype=torch.float32).reshape(6, 5))
    v = torch.ones(5)
    out = torch.empty(5)
    buf = ring._coef.data_ptr()
    c = np.array([1.0, 0.0, -2.0, 0.5, 0.0, 0.25])
    ring.lincomb(c, 3.0, v, out)
    np.testing.assert_array_equal(out.numpy(), (3.0 + c @ ring.HS.double().numpy()).astype(np.float32))
    ring.lincomb(-c, 0.0, None, out)
    np.testing.assert_array_equal(out.numpy(), (-c @ ring.HS.double().numpy()).astype(np.float32))
    assert ring._coef.data_ptr() == buf


def test_a_run_frees_its_ring_on_return():
    """``hess_inv=False`` frees the ring when the driver returns: nothing of a run may sit in a
    reference cycle that only the next garbage collection breaks (at 1e7 parameters the ring
    is 0.9 GB of device memory, and the next run would allocate a second one)."""
    from multigrad_amd.optim.lbfgs import lbfgs_minimize
    from multigrad_amd.optim.lbfgsb import lbfgsb_minimize

    def lg(x):
        r = x.double() - 0.5
        return (r * r).sum() + 0.25 * (r ** 4).sum(), (2 * r + r ** 3).float()

    x0 = torch.linspace(-1.0, 2.0, 7)
    gc.collect()
    gc.disable()
    try:
        a = lbfgs_minimize(GenericObjective(lg, x0), maxiter=5, hess_inv=False)
        b = lbfgsb_minimize(BoxObjective(lg, x0), torch.zeros(7), torch.ones(7), maxiter=5,
                            hess_inv=False)
        assert a.nit > 1 and b.nit > 1
        assert not [o for o in gc.get_objects() if isinstance(o, PairRing)]
    finally:
        gc.enable()


# ---------------------------------------------------------------------------- the objective
def test_box_objective_is_the_generic_objective_without_bounds():
    def lg(x, shift=0.0):
        r = x.double() - shift
        return (r * r * r).sum(), (3 * r * r).float()

    x0 = torch.tensor([[0.5, -1.25], [3.0, 0.1]], dtype=torch.float64)
    a, b = BoxObjective(lg, x0, shift=0.25), GenericObjective(lg, x0, shift=0.25)
    assert isinstance(a, GenericObjective) and a.bounds is None
    assert torch.equal(a.x0(), b.x0()) and a.x0().dtype == torch.float32 and a.n_local == 4
    u = a.x0() * 1.5
    (fa, ga), (fb, gb) = a(u), b(u)
    assert fa == fb and torch.equal(ga, gb)
    assert a.full(u) is u and a.vector_layout().P == 4
    with pytest.raises(TypeError):
        BoxObjective(lg, x0, bounds=None)
