"""The dual (K x K) Gauss-Newton solve, its inverse-Hessian operator, weighted_gram's
PyTorch form and the CPU form of the one-pass SMF Jacobian: one dual step against the dense
solve, whole fits of a float64 user model by both solvers, the population model with its
native Jacobian on one and two gloo ranks, and the example."""
import os
import subprocess
import sys
from dataclasses import dataclass

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from distributed import run_distributed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
EDGES = (9.2, 9.5, 9.8, 10.1, 10.4)
PARAMS = (0.1, -0.2, -0.6)
FTOL = 2.2e-9   # the drivers' default


# ---------------------------------------------------------------- 1. one step
def _step_inputs(K, P, seed, zero_column=False):
    g = torch.Generator().manual_seed(seed)
    J = torch.randn(K, P, generator=g, dtype=F64)
    if zero_column:
        J[:, P // 3] = 0.0
    A = torch.randn(K, K, generator=g, dtype=F64)
    lam, vec = torch.linalg.eigh(A + A.T)
    assert float(lam.min()) < 0.0 < float(lam.max())   # indefinite before clipping
    H = (vec * lam) @ vec.T
    Hp = (vec * lam.clamp_min(0.0)) @ vec.T
    c = torch.randn(K, generator=g, dtype=F64)
    return J, c, 0.5 * (H + H.T), Hp


def _step_error(J, c, H, Hp, lam):
    from multigrad_amd.optim import gauss_newton as gn
    dense = gn._solve((J.T @ Hp @ J).numpy(), lam, (J.T @ c).numpy())
    dual = gn.dual_step(J, c, H, lam)
    assert dual.dtype == F64 and dual.shape == (J.shape[1],)
    return float(np.abs(dual.numpy() - dense).max() / np.abs(dense).max())


@pytest.mark.parametrize("lam", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("K,P", [(4, 50), (10, 2000), (5, 2)])
def test_dual_step_equals_dense_solve(K, P, lam):
    err = _step_error(*_step_inputs(K, P, seed=K * P), lam)
    print(f"K={K} P={P} lambda={lam:g}: |dual - dense| / max|dense| = {err:.2e}")
    assert err <= 1e-9


def test_dual_step_with_a_zero_column():
    """The floored d makes the damped system ill-conditioned at a small lambda."""
    err = _step_error(*_step_inputs(10, 2000, seed=5, zero_column=True), 1e-3)
    print(f"zero column: |dual - dense| / max|dense| = {err:.2e}")
    assert err <= 1e-7


# ---------------------------------------------------------------- 2. the 3-parameter model
def _user_model():
    """The model of tests/test_gauss_newton.py: 3 parameters, 2000 objects in two groups, a
    loss whose Hessian at PARAMS is indefinite."""
    import multigrad_amd as mg
    from multigrad_amd.ops import gaussian_binned_sum
    from multigrad_amd.ops.groups import GroupIndex
    g = torch.Generator().manual_seed(21)
    x = 9.0 + 1.5 * torch.rand(2000, generator=g, dtype=F64)
    grp = torch.randint(0, 2, (2000,), generator=g)
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


@pytest.fixture(scope="module")
def user_fits():
    import multigrad_amd.parallel.comm as C
    C.set_world_comm(None)
    model = _user_model()
    p = torch.tensor(PARAMS, dtype=F64)
    return model, model.run_gauss_newton(p, solver="dual"), model.run_gauss_newton(p, solver="dense")


def test_user_model_fits_agree(user_fits):
    _, dual, dense = user_fits
    assert dual.success and dense.success, (dual.message, dense.message)
    assert dual.solver == "dual"
    for k in ("x", "fun", "jac", "nit", "nfev", "njev", "success", "message", "jac_mode",
              "hess_inv"):
        assert k in dual, k
    assert torch.is_tensor(dual.x) and dual.x.shape == (3,) and dual.x.dtype == F64
    print(f"dual: fun={dual.fun:.12e} nit={dual.nit}; dense: fun={dense.fun:.12e} nit={dense.nit}")
    assert abs(dual.fun - dense.fun) <= 10 * FTOL * max(abs(dense.fun), 1.0)


def test_user_model_hess_inv_operator(user_fits):
    model, dual, _ = user_fits
    _, _, J, H = model.calc_gauss_newton_factors_from_params(dual.x)
    assert J.shape == (4, 3) and H.shape == (4, 4) and H.dtype == F64
    ref = np.linalg.pinv((J.T @ H @ J).numpy())
    op = dual.hess_inv
    dense = op.todense()
    assert op.shape == (3, 3) and dense.dtype == np.float64
    assert np.abs(dense - ref).max() <= 1e-8 * np.abs(ref).max()
    assert np.abs(op.diagonal().numpy() - np.diag(dense)).max() <= 1e-12 * np.abs(dense).max()
    v = np.array([0.3, -1.1, 0.7])
    assert np.abs(op @ v - dense @ v).max() <= 1e-12 * np.abs(dense @ v).max()
    V = np.stack([v, v[::-1], 2 * v, v * v, -v], axis=1)      # more than one 4-column pass
    assert np.abs(op @ V - dense @ V).max() <= 1e-12 * np.abs(dense @ V).max()


def test_factors_agree_with_the_dense_matrix():
    model = _user_model()
    p = torch.tensor(PARAMS, dtype=F64)
    loss, grad, J, H = model.calc_gauss_newton_factors_from_params(p)
    loss_d, grad_d, G = model.calc_gauss_newton_from_params(p)
    assert float(abs(loss - loss_d)) == 0.0
    assert float((grad - grad_d).abs().max()) <= 1e-12 * float(grad_d.abs().max())
    assert float((J.T @ H @ J - G).abs().max()) <= 1e-12 * float(G.abs().max())
    with pytest.raises(ValueError):
        model.run_gauss_newton(p, solver="sparse")


def test_non_finite_jacobian_ends_the_fit_without_success():
    from multigrad_amd.optim import gauss_newton as gn
    J = torch.randn(3, 7, generator=torch.Generator().manual_seed(2), dtype=F64)
    J[1, 2] = float("nan")
    res = gn.run_gauss_newton_dual(
        lambda x: (torch.tensor(1.0), torch.ones(3), J, torch.eye(3), "forward"),
        lambda x: torch.tensor(0.5), torch.zeros(7, dtype=F64))
    assert not res.success and "not finite" in res.message and res.nit == 0
    assert np.isnan(res.hess_inv.todense()).all()


# ---------------------------------------------------------------- 3. weighted_gram fallback
GRAM_SHAPES = [(1, 37), (10, 1001), (16, 64), (17, 259), (40, 130)]


def _gram_bound(J, w, n):
    a = np.abs(J.astype(np.float64))
    aw = a if w is None else a * np.abs(w.astype(np.float64))
    return (n + 4) * 2.0 ** -53 * (aw @ a.T)


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("K,n", GRAM_SHAPES)
def test_weighted_gram_fallback(K, n, weighted):
    from multigrad_amd.ops.gram import weighted_gram
    g = torch.Generator().manual_seed(K * n)
    # integer data: exact
    Ji = torch.randint(-8, 9, (K, n), generator=g)
    wi = torch.randint(-8, 9, (n,), generator=g) if weighted else None
    out = weighted_gram(Ji.float(), None if wi is None else wi.float())
    assert out.dtype == F64 and out.shape == (K, K)
    exact = (Ji if wi is None else Ji * wi) @ Ji.T
    assert torch.equal(out, exact.double())
    # normal data: the float64 summation bound
    J = torch.randn(K, n, generator=g)
    w = torch.rand(n, generator=g) + 0.1 if weighted else None
    out = weighted_gram(J, w).numpy()
    Jn, wn = J.numpy(), None if w is None else w.numpy()
    ref = (Jn.astype(np.float64) * (1.0 if wn is None else wn.astype(np.float64))) @ Jn.astype(np.float64).T
    assert (np.abs(out - ref) <= _gram_bound(Jn, wn, n)).all()
    # float64 input and a row count
    out64 = weighted_gram(J.double(), None if w is None else w.double(), nrows=max(K - 1, 1))
    k = max(K - 1, 1)
    assert (np.abs(out64.numpy() - ref[:k, :k]) <= _gram_bound(Jn, wn, n)[:k, :k]).all()


def test_weighted_gram_refuses_bad_arguments():
    from multigrad_amd.ops.gram import weighted_gram
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(0, 5))
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(257, 5))
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(3, 5), torch.zeros(4))
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(5, 3).T)
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(3, 5), nrows=4)


# ---------------------------------------------------------------- 4. smf_jacobian_into, CPU
def _cpu_shard(nb, chunks=1):
    from multigrad_amd.ops import smf as S
    g = torch.Generator().manual_seed(nb)
    npop, n = 40, 3000
    x = 10.0 + torch.rand(n, generator=g, dtype=F64)
    pop = torch.randint(0, npop - 1, (n,), generator=g)     # population 39 has no halos
    theta = torch.empty(2 * npop, dtype=F64)
    theta[0::2] = -2.0 + 0.2 * (torch.rand(npop, generator=g, dtype=F64) - 0.5)
    theta[1::2] = -0.5 + 0.2 * (torch.rand(npop, generator=g, dtype=F64) - 0.5)
    bins = S.SmfBins.make(np.linspace(8.0, 9.6, nb + 1), volume=1e4)
    shard = S.PopulationShard(x.float(), pop.int(), npop, device="cpu", chunks=chunks)
    xf = x.float().double()
    ref = torch.autograd.functional.jacobian(
        lambda t: S.smf_sumstats_reference(t, xf, pop, bins, True), theta)
    return shard, bins, theta, ref


@pytest.mark.parametrize("nb", [10, 7])
def test_smf_jacobian_cpu_matches_functional_jacobian(nb):
    from multigrad_amd.ops import smf as S
    shard, bins, theta, ref = _cpu_shard(nb)
    assert int(shard.counts[39]) == 0 and not ref[:, 78:].any()
    jac = torch.full((nb, theta.numel()), float("nan"), dtype=F64)
    assert S.smf_jacobian_into(theta, shard, bins, True, jac) is jac
    assert float((jac - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    s, j2 = S.smf_sumstats_and_jacobian(theta, shard, bins)
    assert torch.equal(j2, jac) and j2.dtype == F64
    assert torch.equal(s, S.smf_sumstats(theta, shard, bins))
    with pytest.raises(ValueError):
        S.smf_jacobian_into(theta, shard, bins, True, torch.zeros(nb + 1, theta.numel(), dtype=F64))


def test_smf_jacobian_cpu_chunks_tile_the_matrix():
    from multigrad_amd.ops import smf as S
    shard, bins, theta, ref = _cpu_shard(10, chunks=3)
    assert shard.nchunks == 3
    jac = torch.full((10, theta.numel()), float("nan"), dtype=F64)
    for c in range(3):
        before = jac.clone()
        S.smf_jacobian_into(theta, shard, bins, True, jac, chunk=c)
        p0, p1 = shard.chunk_pops[c], shard.chunk_pops[c + 1]
        changed = ~((jac == before) | (jac.isnan() & before.isnan()))
        assert not changed[:, :2 * p0].any() and not changed[:, 2 * p1:].any()
    assert float((jac - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# ---------------------------------------------------------------- 5. the population model
def _population_model():
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    data = make_population_data(400, 40_000, seed=3, device=torch.device("cpu"))
    model = PopulationSMFModel(aux_data=data)
    model.set_target_from_truth()
    return model, data["guess"]


@pytest.fixture(scope="module")
def population_one_rank():
    import multigrad_amd.parallel.comm as C
    C.set_world_comm(None)
    model, guess = _population_model()
    return model, guess, model.run_gauss_newton(guess, maxsteps=20, solver="dual")


def test_population_model_dual_fit(population_one_rank):
    model, guess, dual = population_one_rank
    dense = model.run_gauss_newton(guess, maxsteps=20, solver="dense", mode="reverse")
    print(f"dual: fun={dual.fun:.3e} nit={dual.nit} njev={dual.njev} nfev={dual.nfev}; "
          f"dense: fun={dense.fun:.3e} nit={dense.nit}")
    assert dual.success, dual.message
    assert dual.jac_mode == "native" and dual.solver == "dual" and dense.jac_mode == "reverse"
    assert dual.fun <= 10.0 * dense.fun + 1e-12
    assert dual.x.shape == guess.shape and dual.x.dtype == guess.dtype
    # one packed [K*K + K + 2] block per Jacobian is all the driver copied to the host
    assert dual.host_copy_sizes == [10 * 10 + 10 + 2] * dual.njev
    assert dual.hess_inv.shape == (400, 400) and bool((dual.hess_inv.diagonal() >= 0).all())


def test_native_jacobian_matches_reverse(population_one_rank):
    model, guess, _ = population_one_rank
    s_n, j_n = model.calc_sumstats_jacobian_from_params(guess, mode="native")
    s_r, j_r = model.calc_sumstats_jacobian_from_params(guess, mode="reverse")
    assert model._sumstats_jacobian(guess)[3] == "native"
    assert torch.equal(s_n, s_r)
    # float32 parameters: the reverse pass differentiates in float32, the native rows are
    # float64 autograd rounded once
    assert float((j_n - j_r).abs().max()) <= 1e-5 * float(j_r.abs().max())


def test_native_mode_needs_the_hook():
    model = _user_model()
    with pytest.raises(ValueError, match="calc_partial_sumstats_and_jacobian_from_params"):
        model.calc_sumstats_jacobian_from_params(torch.tensor(PARAMS, dtype=F64), mode="native")


# ---------------------------------------------------------------- 6. two gloo ranks
def _ranks_population(rank, size):
    model, guess = _population_model()
    assert model.comm.size == size
    res = model.run_gauss_newton(guess, maxsteps=20, solver="dual")
    return {"x": res.x.numpy(), "fun": float(res.fun), "success": bool(res.success),
            "jac_mode": res.jac_mode}


def test_two_ranks_give_identical_iterates(population_one_rank):
    _, _, one = population_one_rank
    res = run_distributed(_ranks_population, 2)
    assert res[0]["success"] and res[0]["jac_mode"] == "native"
    assert np.array_equal(res[0]["x"], res[1]["x"]) and res[0]["fun"] == res[1]["fun"]
    print(f"two ranks: fun={res[0]['fun']:.3e}; one rank: fun={one.fun:.3e}")
    assert abs(res[0]["fun"] - one.fun) <= 10 * FTOL


# ---------------------------------------------------------------- 7. the example
def test_example_runs():
    env = dict(os.environ, MULTIGRAD_PROGRESS="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "population_gauss_newton.py")],
                         env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "jac_mode native" in out.stdout and "hess_inv diagonal" in out.stdout
