"""The box-constrained Gauss-Newton step and driver on the CPU: the op's composition against
a float64 formula, the inner solve against the unconstrained dual step and against BVLS, a
fit whose optimum lies on a bound against scipy's L-BFGS-B, the inner failure path, two gloo
ranks and the model front end."""
import os
import sys
from dataclasses import dataclass

import numpy as np
import pytest
import scipy.optimize
import torch

from multigrad_amd.optim.gauss_newton_box import box_step, run_gauss_newton_box

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from distributed import run_distributed  # noqa: E402

F64 = torch.float64
U = 2.0 ** -53
EDGES = (9.2, 9.5, 9.8, 10.1, 10.4)
PARAMS = (0.1, -0.2, -0.6)
BOUNDS = [(-1.0, 1.0), (-1.0, 1.0), (-0.5, 0.0)]   # the free optimum has log width -5.76


# ---------------------------------------------------------------- 1. the op's composition
def _formula(J, a, d, lam, lo, hi):
    J, d, lo, hi = (np.asarray(x, dtype=np.float64) for x in (J, d, lo, hi))
    t = a @ J
    sigma = -t / (lam * d)
    delta = np.clip(sigma, lo, hi)
    free = (sigma > lo) & (sigma < hi)
    W = (J * (free / (lam * d))) @ J.T
    s = np.sum(t * delta + 0.5 * lam * d * delta * delta)
    return J @ delta, W, s, int(free.sum()), delta, np.abs(J) @ np.abs(delta), \
        (np.abs(J) * (free / (lam * d))) @ np.abs(J).T, \
        np.sum(np.abs(t * delta) + 0.5 * lam * d * delta * delta)


def _pass(J, a, d, lam, lo, hi, dtype):
    from multigrad_amd.ops.box_dual import box_dual_pass
    Jt, dt, lot, hit = (torch.as_tensor(x, dtype=dtype) for x in (J, d, lo, hi))
    delta = torch.full((Jt.shape[1],), float("nan"), dtype=dtype)
    blk = box_dual_pass(Jt, torch.as_tensor(a, dtype=F64), dt, lam, lot, hit, delta).numpy()
    none = box_dual_pass(Jt, torch.as_tensor(a, dtype=F64), dt, lam, lot, hit).numpy()
    assert np.array_equal(blk, none)
    K = Jt.shape[0]
    return blk[:K], blk[K:K + K * K].reshape(K, K), blk[-2], blk[-1], delta.numpy()


def _check_pass(J, a, d, lam, lo, hi, dtype=torch.float64):
    """The composition is float64 on the CPU: a few dozen roundings per term and a pairwise
    or BLAS sum on both sides, far inside ``(P + 64) u sum |terms|``."""
    if dtype == torch.float32:   # the formula sees what the op sees
        J, d, lo, hi = (np.asarray(x, dtype=np.float32) for x in (J, d, lo, hi))
    v, W, s, nfree, delta = _pass(J, a, d, lam, lo, hi, dtype)
    rv, rW, rs, rfree, rdelta, av, aW, asum = _formula(J, a, d, lam, lo, hi)
    g = (np.shape(J)[1] + 64) * U
    assert nfree == rfree
    assert (np.abs(v - rv) <= g * av).all()
    assert (np.abs(W - rW) <= g * aW).all()
    assert abs(s - rs) <= g * asum
    # t is a sum of K products on either side (sigma two roundings more); delta_out is
    # rounded to its dtype
    J64, d64 = np.asarray(J, dtype=np.float64), np.asarray(d, dtype=np.float64)
    et = 2 * (J64.shape[0] + 8) * U * (np.abs(a) @ np.abs(J64)) / (lam * d64)
    e = 2.0 ** -24 if dtype == torch.float32 else 0.0
    assert (np.abs(delta - rdelta) <= et + e * np.abs(rdelta)).all()
    return v, W, s, nfree, delta


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("K,P", [(1, 1), (1, 7), (3, 5), (10, 39), (20, 64)])
def test_composition_matches_the_formula(K, P, dtype):
    rng = np.random.default_rng(100 * K + P)
    J = rng.normal(size=(K, P)) * 10.0 ** rng.uniform(-3, 1, size=P)
    a = rng.normal(size=K)
    d = rng.random(P) + 0.1
    sigma = -(a @ J) / (0.7 * d)
    lo = -np.abs(sigma) * rng.random(P) * 2.0
    hi = np.abs(sigma) * rng.random(P) * 2.0
    lo[rng.random(P) < 0.2] = -np.inf
    hi[rng.random(P) < 0.2] = np.inf
    _, _, _, nfree, delta = _check_pass(J, a, d, 0.7, lo, hi, dtype)
    assert (delta >= lo.astype(delta.dtype)).all() and (delta <= hi.astype(delta.dtype)).all()
    if P >= 39:
        assert 0 < nfree < P


def test_composition_exact_ties():
    rng = np.random.default_rng(5)
    K, P = 4, 12
    J = rng.normal(size=(K, P))
    d = rng.random(P) + 0.1
    hi = rng.random(P)
    # a = 0: t = 0 and sigma = -0 everywhere; with lo = 0 no column is free and delta = 0
    v, W, s, nfree, delta = _check_pass(J, np.zeros(K), d, 0.5, np.zeros(P), hi)
    assert nfree == 0 and not delta.any() and not v.any() and not W.any() and s == 0.0
    # with lo < 0 the same columns are free, at delta = 0
    _, W, _, nfree, delta = _check_pass(J, np.zeros(K), d, 0.5, -hi, hi)
    assert nfree == P and not delta.any() and W.any()
    # lo = hi = 0: a column that is never free, whatever sigma
    a = rng.normal(size=K)
    lo = -rng.random(P)
    fixed = np.arange(P) % 3 == 0
    lo[fixed], hi[fixed] = 0.0, 0.0
    _, _, _, nfree, delta = _check_pass(J, a, d, 0.5, lo, hi)
    assert not delta[fixed].any()
    sigma = -(a @ J) / (0.5 * d)
    assert nfree == int(((sigma > lo) & (sigma < hi))[~fixed].sum())
    # every side open: all free, delta = sigma
    inf = np.full(P, np.inf)
    _, _, _, nfree, delta = _check_pass(J, a, d, 0.5, -inf, inf)
    assert nfree == P and np.allclose(delta, sigma, rtol=1e-14, atol=0.0)


def test_float64_path_in_chunks(monkeypatch):
    """The path the GPU takes for what the kernel does not (K > 10, other dtypes), run here on
    CPU tensors with 16 columns per chunk: the same float64 formula, so the same bounds."""
    from multigrad_amd.ops import box_dual
    monkeypatch.setattr(box_dual, "_CHUNK", 16)
    monkeypatch.setattr(box_dual, "_composed", box_dual._float64_pass)
    rng = np.random.default_rng(77)
    for K, P, dtype in [(12, 50, torch.float32), (3, 16, torch.float64), (16, 1, torch.float32)]:
        J = rng.normal(size=(K, P)) * 10.0 ** rng.uniform(-3, 1, size=P)
        a = rng.normal(size=K)
        d = rng.random(P) + 0.1
        sigma = -(a @ J) / (0.7 * d)
        lo = -np.abs(sigma) * rng.random(P) * 2.0
        hi = np.abs(sigma) * rng.random(P) * 2.0
        hi[rng.random(P) < 0.2] = np.inf
        _check_pass(J, a, d, 0.7, lo, hi, dtype)


def test_op_refuses_bad_arguments():
    from multigrad_amd.ops.box_dual import box_dual_pass
    J, a, vec = torch.zeros(3, 8), torch.zeros(3, dtype=F64), torch.ones(8)
    assert box_dual_pass(J, a, vec, 1.0, -vec, vec).shape == (3 + 9 + 2,)
    for args in [(torch.zeros(0, 8), torch.zeros(0, dtype=F64), vec, 1.0, -vec, vec),
                 (torch.zeros(257, 8), torch.zeros(257, dtype=F64), vec, 1.0, -vec, vec),
                 (torch.zeros(8, 3).T, a, vec, 1.0, -vec, vec),
                 (J, a.float(), vec, 1.0, -vec, vec),
                 (J, a[:2], vec, 1.0, -vec, vec),
                 (J, a, vec[:7], 1.0, -vec, vec),
                 (J, a, vec, 1.0, -vec, torch.ones(16)[::2]),
                 (J, a, vec, 1.0, -vec, vec, torch.zeros(7)),
                 (J, a, vec, 1.0, -vec, vec, torch.zeros(8, dtype=torch.int32))]:
        with pytest.raises(ValueError):
            box_dual_pass(*args)


# ---------------------------------------------------------------- 2. the inner solve
def _random_case(rng, lam_range, trial):
    """The distribution of the design study: K in 1..10, P in 1..39, column scales
    10^U(-3, 1), 80 % of the sides bounded in U(0, 1) (a fifth of those at 0), 20 % open, a
    rank-deficient H every third case."""
    K, P = int(rng.integers(1, 11)), int(rng.integers(1, 40))
    J = rng.normal(size=(K, P)) * 10.0 ** rng.uniform(-3, 1, size=P)
    c = rng.normal(size=K)
    H = rng.normal(size=(K, K))
    H = H @ H.T
    if trial % 3 == 0:
        H[:, -1] = 0.0
        H[-1, :] = 0.0
    lam = 10.0 ** rng.uniform(*lam_range)
    lo = -rng.uniform(0, 1, size=P) * (rng.random(P) < 0.8)
    hi = rng.uniform(0, 1, size=P) * (rng.random(P) < 0.8)
    lo[rng.random(P) < 0.2] = -np.inf
    hi[rng.random(P) < 0.2] = np.inf
    return J, c, H, lam, lo, hi


def _least_squares_form(J, c, H, lam):
    """``m(delta) = 1/2 |A delta - b|^2`` (the damped model plus a constant), with ``L`` and
    ``d`` as the driver forms them."""
    from multigrad_amd.optim.gauss_newton import _psd_factor
    L = _psd_factor(H)
    dd = np.einsum("kp,kl,lp->p", J, L @ L.T, J)
    d = np.maximum(dd, 1e-12 * dd.max())
    A = np.vstack([L.T @ J, np.diag(np.sqrt(lam * d))])
    b = np.concatenate([np.zeros(L.shape[1]), -(J.T @ c) / np.sqrt(lam * d)])
    return A, b, L, d


def test_no_box_is_the_dual_step_in_one_pass():
    """With every side open the start ``z0`` already solves the dual.  ``z0`` comes from an
    ``r x r`` Cholesky solve, backward stable, so ``|grad q| <= 8 r u cond(A) (|L^T J delta| +
    |z|)`` with ``A = I + L^T W L``, plus what evaluating ``grad q`` itself rounds: ``P + K``
    terms per sum and the error ``(K + 8) u sum_k |J_kp a_k| / (lam d_p)`` of ``delta_p``.  The step is ``-J^T a / (lam d)`` with ``a = c + L z0``
    here and ``a = c - y`` in ``dual_step``: two roundings of the same vector, each off by at
    most ``8 r u cond(A) (|c| + |y|)`` per entry, then ``K`` products and adds and two
    divisions, so ``|delta - dual_step| <= (16 r cond(A) + K + 8) u sum_k |J_kp| (|c_k| +
    |y_k|) / (lam d_p)``."""
    from multigrad_amd.optim.gauss_newton import _DualFactors, dual_step
    rng = np.random.default_rng(11)
    for trial in range(20):
        J, c, H, lam, _, _ = _random_case(rng, (-3, 3), trial)
        K, P = J.shape
        inf = torch.full((P,), float("inf"), dtype=F64)
        Jt = torch.from_numpy(J)
        delta, info = box_step(Jt, c, H, lam, -inf, inf)
        fac = _DualFactors(Jt, c, H, [])
        r = fac.L.shape[1]
        cond = np.linalg.cond(np.eye(r) + fac.L.T @ (fac.W1 / lam) @ fac.L) if r else 1.0
        if not fac.dmax > 0.0:     # K = 1 with H = 0: J^T H+ J = 0, no step (as dual_step)
            assert info.passes == 0 and not delta.any()
            continue
        assert info.converged and info.passes == 1 and info.free == P
        a = c + fac.L @ info.z
        d = 1.0 / fac.inv_d.numpy()
        dn = delta.numpy()
        e_delta = (K + 8) * U * (np.abs(J).T @ np.abs(a)) / (lam * d)
        e_eval = np.abs(fac.L).T @ ((P + K + 16) * U * (np.abs(J) @ np.abs(dn)) + np.abs(J) @ e_delta)
        scale = np.linalg.norm(fac.L.T @ (J @ dn)) + np.linalg.norm(info.z)
        assert info.residual * scale <= 8 * max(r, 1) * U * cond * scale + np.linalg.norm(e_eval)
        ref = dual_step(Jt, c, H, lam).numpy()
        y = c - lam * fac.coefficients(lam)
        bound = (16 * max(r, 1) * cond + K + 8) * U * (np.abs(J).T @ (np.abs(c) + np.abs(y))) / (lam * d)
        assert (np.abs(delta.numpy() - ref) <= bound).all()


@pytest.mark.parametrize("P", [2000, 20000])
def test_float32_jacobian_with_an_open_box_converges(P):
    """A float32 ``J`` is what the GPU fits use.  ``W1`` is then built from the float32-rounded
    ``1 / d`` while a pass divides by ``lam d`` in float64, so the start is off by about 6e-8
    relative and one Newton step has to repair it; its gain in ``q``, about (6e-8)^2 |q|, is
    far below the rounding of ``q`` (a sum over P terms), so an acceptance test on ``q``
    alone rejects it.  Every solve must converge, in at most 3 passes, K on both sides of
    the fused limit."""
    rng = np.random.default_rng(3)
    for trial in range(24):
        K = 1 + trial % 16
        J = (rng.normal(size=(K, P)) * 10.0 ** rng.uniform(-3, 1, size=P)).astype(np.float32)
        c = rng.normal(size=K)
        H = rng.normal(size=(K, K))
        H = H @ H.T
        lam = 10.0 ** rng.uniform(-3, 3)
        inf = torch.full((P,), float("inf"))
        delta, info = box_step(torch.from_numpy(J), c, H, lam, -inf, inf)
        assert delta.dtype == torch.float32
        assert info.converged and info.passes <= 3 and info.free == P, (trial, K, info.passes,
                                                                         info.residual)


TAU = 2.2e-10   # three times the largest gap measured (below)


def test_box_step_against_bvls():
    """500 cases, lambda in [1e-3, 1e3]: at most 5 unconverged in 40 passes; every converged
    step has a model value within TAU (relative) of BVLS's and a scaled KKT residual below
    1e-9.  Measured: 1 of 500 unconverged (20 more have K = 1 and H = 0, where there is no
    model and no step), median 3 passes, largest gap to BVLS 7.227e-11 (BVLS's own stopping
    tolerance: the gap is negative where it stopped early), largest KKT residual 8.7e-13."""
    rng = np.random.default_rng(0)
    unconverged, degenerate, worst_gap, worst_kkt, passes = 0, 0, -np.inf, 0.0, []
    for trial in range(500):
        J, c, H, lam, lo, hi = _random_case(rng, (-3, 3), trial)
        delta, info = box_step(torch.from_numpy(J), c, H, lam, torch.from_numpy(lo),
                               torch.from_numpy(hi))
        delta = delta.numpy()
        assert (delta >= lo).all() and (delta <= hi).all()       # converged or not
        if not H.any():            # K = 1 with H = 0: J^T H+ J = 0, no step and no model
            assert info.passes == 0 and not delta.any()
            degenerate += 1
            continue
        if not info.converged:
            unconverged += 1
            continue
        passes.append(info.passes)
        A, b, _, _ = _least_squares_form(J, c, H, lam)
        ref = scipy.optimize.lsq_linear(A, b, bounds=(lo - 1e-15, hi + 1e-15), method="bvls",
                                        tol=1e-14).x

        def m(x):
            return 0.5 * float(np.sum((A @ x - b) ** 2))

        gap = (m(delta) - m(ref)) / abs(m(ref)) if m(ref) else m(delta)
        worst_gap = max(worst_gap, gap)
        grad = A.T @ (A @ delta - b)
        diag = np.einsum("ij,ij->j", A, A)
        kkt = np.abs(np.clip(delta - grad / diag, lo, hi) - delta).max()
        top = np.abs(delta).max()
        worst_kkt = max(worst_kkt, kkt / top if top else kkt)
        assert gap <= TAU, (trial, gap)
    print(f"unconverged {unconverged} of 500 ({degenerate} with H = 0), median passes {np.median(passes)}, largest gap "
          f"to BVLS {worst_gap:.3e}, largest KKT residual {worst_kkt:.3e}")
    assert unconverged <= 5
    assert worst_kkt <= 1e-9


# ---------------------------------------------------------------- 3. fits
def _user_model(rank=0, size=1):
    """The 3-parameter model of tests/test_gauss_newton.py (two group offsets and one log
    width, 2000 objects in two groups, a loss nonlinear in the sumstats); this rank's shard."""
    import multigrad_amd as mg
    from multigrad_amd.ops import gaussian_binned_sum
    from multigrad_amd.ops.groups import GroupIndex
    g = torch.Generator().manual_seed(21)
    x = 9.0 + 1.5 * torch.rand(2000, generator=g, dtype=F64)
    grp = torch.randint(0, 2, (2000,), generator=g)
    x, grp = (torch.tensor_split(t, size)[rank] for t in (x, grp))
    target = torch.tensor([310.0, 420.0, 95.0, 330.0], dtype=F64)

    @dataclass(eq=False)
    class UserModel(mg.OnePointModel):
        def __post_init__(self):
            super().__post_init__()
            self.plan = GroupIndex(grp, 2)

        def calc_partial_sumstats_from_params(self, params, randkey=None):
            (shift,) = self.plan.gather(params[:2])
            return gaussian_binned_sum(x + shift, torch.pow(10.0, params[2:]), EDGES)

        def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
            r = torch.log(sumstats / target)
            return (r * r).sum() + 0.3 * r[0] * r[1]

    return UserModel(device="cpu", dtype=F64)


def _recorded_fit(model, **kw):
    """``run_gauss_newton_box`` on the model's hooks with every point the loss saw."""
    seen = []

    def loss_fn(x):
        seen.append(x.detach().clone().numpy())
        return model.calc_loss_from_params(x)

    res = run_gauss_newton_box(lambda x: model._gauss_newton_factors(x, None, "auto", True),
                               loss_fn, torch.tensor(PARAMS, dtype=F64), **kw)
    return res, np.array(seen)


@pytest.fixture(scope="module")
def lbfgsb():
    model = _user_model()

    def f(x):
        loss, grad = model.calc_loss_and_grad_from_params(torch.tensor(x, dtype=F64))
        return float(loss), grad.numpy().astype(np.float64)

    return scipy.optimize.minimize(f, np.array(PARAMS), jac=True, method="L-BFGS-B", bounds=BOUNDS,
                                   options=dict(ftol=1e-15, gtol=1e-12, maxiter=500))


X_TOL = 3.9e-5   # ten times the distance measured without a cap (below)


@pytest.mark.parametrize("max_step", [None, 0.05, (0.05, 0.2, 0.01)], ids=["free", "cap", "caps"])
def test_fit_with_the_optimum_on_a_bound(max_step, lbfgsb):
    """The log width ends on its lower bound.  ``x`` agrees with scipy's L-BFGS-B (float64,
    ftol 1e-15) within X_TOL.  Measured distance: 3.9e-6 without a cap (the fit stops on
    ftol = 2.2e-9, a loss 3.6e-11 above L-BFGS-B's), 5.7e-6 and 3.0e-6 with the caps."""
    model = _user_model()
    res, seen = _recorded_fit(model, param_bounds=BOUNDS, max_step=max_step)
    lo, hi = np.array(BOUNDS).T
    print(f"max_step={max_step}: x={res.x.numpy()} fun={res.fun:.12e} nit={res.nit} "
          f"nfev={res.nfev} passes={res.inner_passes} ({res.message}); L-BFGS-B x={lbfgsb.x} "
          f"fun={lbfgsb.fun:.12e}; distance {np.abs(res.x.numpy() - lbfgsb.x).max():.3e}")
    assert res.success and res.solver == "dual-box"
    assert res.active.dtype == torch.int8 and res.active.tolist() == [0, 0, -1]
    assert float(res.x[2]) == lo[2]
    assert len(seen) == res.nfev and (seen >= lo).all() and (seen <= hi).all()
    assert np.abs(res.x.numpy() - lbfgsb.x).max() <= X_TOL
    assert res.fun <= lbfgsb.fun + 2.2e-9 * max(lbfgsb.fun, 1.0)
    if max_step is not None:
        # accepted points in order: the start, then every trial that lowered the loss
        accepted = [t[3] for t in res.trials if t[2]]
        assert len(accepted) == len(seen)
        path = np.vstack([np.clip(np.array(PARAMS), lo, hi), seen[np.array(accepted)]])
        assert len(path) == res.nit + 1
        cap = np.broadcast_to(np.asarray(max_step, dtype=np.float64), (3,))
        assert (np.abs(np.diff(path, axis=0)) <= cap * (1.0 + 2.0 ** -23)).all()
    # the operator ignores the active column
    dense = res.hess_inv.todense()
    assert not dense[2].any() and not dense[:, 2].any() and dense[:2, :2].any()


def test_start_outside_the_bounds_is_clamped():
    model = _user_model()
    bounds = [(0.3, 1.0), (-1.0, -0.4), (-0.5, 0.0)]
    res, seen = _recorded_fit(model, param_bounds=bounds, maxsteps=3)
    lo, hi = np.array(bounds).T
    assert (seen >= lo).all() and (seen <= hi).all()
    assert (res.x.numpy() >= lo).all() and (res.x.numpy() <= hi).all()
    with pytest.raises(ValueError):
        _recorded_fit(model, param_bounds=[(1.0, 0.0)] * 3)
    with pytest.raises(ValueError):
        _recorded_fit(model, max_step=-1.0)
    with pytest.raises(ValueError):
        _recorded_fit(model, max_step=[0.1, 0.2])


def test_inner_failure_raises_the_damping_and_costs_no_loss_evaluation():
    """One pass per solve is not enough while a bound is active: those trials are rejected
    without a loss evaluation and lambda never returns below ten times the lambda of the last
    failure."""
    model = _user_model()
    res, seen = _recorded_fit(model, param_bounds=BOUNDS, inner_passes=1)
    failed = [t for t in res.trials if not t[2]]
    assert res.inner_unconverged == len(failed) > 0
    assert res.nfev == len(seen) == len(res.trials) - len(failed)
    assert res.inner_passes == len(res.trials)         # one pass each
    assert res.message                                  # the run ended by one of its rules
    floor = 1e-4
    for lam, npass, converged, _ in res.trials:
        assert lam >= floor and npass == 1
        if not converged:
            floor = max(floor, 10.0 * lam)
    assert res.damping_floor == floor and res.damping >= floor
    # the same fit with the default budget converges in every trial after the first
    full, _ = _recorded_fit(model, param_bounds=BOUNDS)
    assert full.inner_unconverged < len(failed) and full.fun < res.fun


def test_min_damping_is_the_floor():
    model = _user_model()
    res, _ = _recorded_fit(model, min_damping=0.5, damping=1e-3)
    assert min(t[0] for t in res.trials) == 0.5 and res.damping_floor == 0.5


# ---------------------------------------------------------------- 4. several ranks
def _ranks_fit(rank, size):
    model = _user_model(rank, size)
    res = model.run_gauss_newton_box(torch.tensor(PARAMS, dtype=F64), param_bounds=BOUNDS,
                                     max_step=0.2)
    return dict(x=res.x.numpy(), fun=float(res.fun), nit=int(res.nit), nfev=int(res.nfev),
                inner_passes=int(res.inner_passes), active=res.active.numpy())


def test_two_ranks_take_the_same_steps():
    res = run_distributed(_ranks_fit, 2)
    for k, v in res[0].items():            # identical on both ranks, bit for bit
        assert np.array_equal(np.asarray(res[1][k]), np.asarray(v)), k
    assert res[0]["nit"] > 0 and res[0]["active"].tolist() == [0, 0, -1]


# ---------------------------------------------------------------- 5. front end
def test_front_end():
    model = _user_model()
    p = torch.tensor(PARAMS, dtype=F64)
    with pytest.raises(ValueError, match="run_gauss_newton_box"):
        model.run_gauss_newton(p, param_bounds=BOUNDS)
    res = model.run_gauss_newton_box(p, param_bounds=BOUNDS, max_step=0.2, maxsteps=4)
    assert res.solver == "dual-box" and res.nit == 4 and res.jac_mode == "forward"
    assert res.x.shape == p.shape and res.x.dtype == F64 and res.jac.shape == p.shape
    for k in ("inner_passes", "inner_unconverged", "active", "hess_inv", "host_copy_sizes"):
        assert k in res, k
    K = len(EDGES) - 1
    assert set(res.host_copy_sizes) == {1, K * K + K + 2}
    import multigrad_amd.optim as optim
    assert optim.run_gauss_newton_box is run_gauss_newton_box
    free = model.run_gauss_newton_box(p, maxsteps=4)
    dual = model.run_gauss_newton(p, maxsteps=4, solver="dual")
    assert np.abs(free.x.numpy() - dual.x.numpy()).max() <= 1e-9    # no box: the dual driver's path


def test_example_runs():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MULTIGRAD_PROGRESS="0")
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "population_gauss_newton_box.py"),
                          "--num-params", "8", "--num-halos", "4000"], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Gauss-Newton in the box" in out.stdout and "parameters on a bound" in out.stdout
