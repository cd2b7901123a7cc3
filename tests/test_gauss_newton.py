"""The sumstat Jacobian, the Gauss-Newton and Fisher matrices and run_gauss_newton on the
CPU: a float64 user model against torch.autograd.functional.jacobian, several gloo ranks
against one, the reverse fallback, and the convergence budgets of the shipped models."""
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


def _user_model(rank=0, size=1):
    """3 parameters (two group offsets and one log width), 2000 objects in two groups; this
    rank's shard of the objects.  The loss is nonlinear in the sumstats, couples two of
    them, and its Hessian at PARAMS is indefinite (a squared log residual is concave beyond
    a residual of 1, and the third target is far off), so psd=True matters."""
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


def _params():
    return torch.tensor(PARAMS, dtype=F64)


def _reference_jacobian(model):
    return torch.autograd.functional.jacobian(model.calc_partial_sumstats_from_params, _params())


@pytest.mark.parametrize("mode", ["forward", "reverse", "auto"])
def test_jacobian_matches_functional_jacobian(mode):
    model = _user_model()
    ref = _reference_jacobian(model)
    s, jac = model.calc_sumstats_jacobian_from_params(_params(), mode=mode)
    assert jac.shape == (4, 3) and jac.dtype == F64
    assert torch.equal(s, model.calc_sumstats_from_params(_params()))
    assert float((jac - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


def test_gauss_newton_matches_hand_algebra():
    model = _user_model()
    p = _params()
    J = _reference_jacobian(model)
    s = model.calc_sumstats_from_params(p)
    H = torch.autograd.functional.hessian(model.calc_loss_from_sumstats, s)
    H = 0.5 * (H + H.T)
    gS = torch.autograd.functional.jacobian(model.calc_loss_from_sumstats, s)
    lam, vec = torch.linalg.eigh(H)
    assert float(lam.min()) < 0.0 < float(lam.max())   # the projection changes H
    Hp = (vec * lam.clamp_min(0.0)) @ vec.T
    loss, grad, G = model.calc_gauss_newton_from_params(p)
    _, grad_raw, G_raw = model.calc_gauss_newton_from_params(p, psd=False)
    assert G.dtype == F64 and G.shape == (3, 3) and grad.shape == (3,)
    assert float(abs(loss - model.calc_loss_from_params(p))) <= 1e-12
    scale = float((J.T @ H.abs() @ J).abs().max())
    assert float((G - J.T @ Hp @ J).abs().max()) <= 1e-9 * scale
    assert float((G_raw - J.T @ H @ J).abs().max()) <= 1e-9 * scale
    assert float(torch.linalg.eigvalsh(G).min()) >= -1e-9 * scale
    ref_grad = model.calc_dloss_dparams(p)
    for g in (grad, grad_raw):
        assert float((g - J.T @ gS).abs().max()) <= 1e-9 * float(ref_grad.abs().max())
        assert float((g - ref_grad).abs().max()) <= 1e-9 * float(ref_grad.abs().max())


def test_linear_loss_has_zero_gauss_newton_matrix():
    model = _user_model()
    model.calc_loss_from_sumstats = lambda s, *a, **k: (s * 0.5).sum()
    loss, grad, G = model.calc_gauss_newton_from_params(_params())
    assert not G.any() and grad.abs().max() > 0


def test_fisher_variances_and_covariance_agree():
    model = _user_model()
    p = _params()
    J = _reference_jacobian(model)
    var = torch.tensor([4.0, 9.0, 2.5, 7.0], dtype=F64)
    F1 = model.calc_fisher_from_params(p, var)
    F2 = model.calc_fisher_from_params(p, torch.diag(var))
    ref = J.T @ torch.diag(1.0 / var) @ J
    assert F1.dtype == F64 and F1.shape == (3, 3)
    assert float((F1 - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    assert float((F2 - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    cov = torch.diag(var) + 0.5
    F3 = model.calc_fisher_from_params(p, cov)
    ref3 = J.T @ torch.linalg.inv(cov) @ J
    assert float((F3 - ref3).abs().max()) <= 1e-9 * float(ref3.abs().max())
    for bad in (var[:3], torch.ones(4, 3, dtype=F64), torch.ones(4, 4, 1, dtype=F64)):
        with pytest.raises(ValueError):
            model.calc_fisher_from_params(p, bad)


def test_bad_mode_raises():
    with pytest.raises(ValueError):
        _user_model().calc_sumstats_jacobian_from_params(_params(), mode="sideways")


# ---------------------------------------------------------------- several ranks
def _ranks_all(rank, size):
    model = _user_model(rank, size)
    p = _params()
    out = {}
    for mode in ("forward", "reverse"):
        s, jac = model.calc_sumstats_jacobian_from_params(p, mode=mode)
        out["s_" + mode], out["jac_" + mode] = s.numpy(), jac.numpy()
    loss, grad, G = model.calc_gauss_newton_from_params(p)
    out["grad"], out["G"] = grad.numpy(), G.numpy()
    res = model.run_gauss_newton(p, maxsteps=6)
    out["x"], out["fun"], out["nit"] = np.asarray(res.x), float(res.fun), int(res.nit)
    out["hess_inv"] = np.asarray(res.hess_inv)
    return out


@pytest.fixture(scope="module")
def one_rank():
    import multigrad_amd.parallel.comm as C
    C.set_world_comm(None)
    return _ranks_all(0, 1)


@pytest.mark.parametrize("size", [2, 3])
def test_several_ranks_match_one_rank(size, one_rank):
    res = run_distributed(_ranks_all, size)
    for r in res[1:]:
        for k, v in res[0].items():            # identical on all ranks, bit for bit
            assert np.array_equal(np.asarray(r[k]), np.asarray(v)), k
    for k in ("s_forward", "jac_forward", "s_reverse", "jac_reverse", "grad", "G", "x"):
        ref = one_rank[k]
        assert np.abs(res[0][k] - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1.0), k
    assert res[0]["nit"] == one_rank["nit"]
    assert abs(res[0]["fun"] - one_rank["fun"]) <= 1e-9


# ---------------------------------------------------------------- reverse fallback
def _joint_model():
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (JointBinnedPopulationSMFModel,
                                                       joint_population_data)
    data = make_population_data(8, 4000, seed=3, device=torch.device("cpu"))
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    return JointBinnedPopulationSMFModel(aux_data=joint_population_data(data)), data["guess"]


def test_auto_falls_back_to_reverse_for_an_op_without_a_forward_rule():
    model, guess = _joint_model()
    s, jac = model.calc_sumstats_jacobian_from_params(guess)
    s_rev, jac_rev = model.calc_sumstats_jacobian_from_params(guess, mode="reverse")
    assert jac.shape == s.shape + (8,) and jac.abs().max() > 0
    assert torch.equal(jac, jac_rev) and torch.equal(s, s_rev)
    assert model._sumstats_jacobian(guess)[3] == "reverse"
    with pytest.raises(NotImplementedError):
        model.calc_sumstats_jacobian_from_params(guess, mode="forward")
    res = model.run_gauss_newton(guess, maxsteps=2)
    assert res.jac_mode == "reverse" and res.nit >= 1


# ---------------------------------------------------------------- run_gauss_newton
def _check_result(res, ndim):
    for k in ("x", "fun", "jac", "nit", "nfev", "njev", "success", "message", "jac_mode",
              "hess_inv"):
        assert k in res, k
    assert np.asarray(res.x).shape == (ndim,) and np.asarray(res.jac).shape == (ndim,)
    assert np.asarray(res.hess_inv).shape == (ndim, ndim)
    assert np.asarray(res.hess_inv).dtype == np.float64
    assert res.success, res.message


def test_docs_model_converges():
    from multigrad_amd.models.smf import DocsSMFModel, make_docs_data
    model = DocsSMFModel(aux_data=make_docs_data(device="cpu"), device="cpu")
    res = model.run_gauss_newton([-1.0, 0.0])
    print(f"DocsSMFModel: x={res.x} loss={res.fun:.3e} nit={res.nit} nfev={res.nfev}")
    _check_result(res, 2)
    assert res.nit <= 50
    assert np.abs(np.asarray(res.x) - np.array([-2.0, -0.5])).max() <= 1e-4


def test_test_suite_model_converges():
    from multigrad_amd.models.smf import MySMFModel, make_test_data
    model = MySMFModel(aux_data=make_test_data(), device="cpu")
    res = model.run_gauss_newton([-1.0, 0.5])
    print(f"MySMFModel: x={res.x} loss={res.fun:.3e} nit={res.nit} nfev={res.nfev}")
    _check_result(res, 2)
    assert res.nit <= 50
    assert np.abs(np.asarray(res.x) - np.array([-2.0, 0.2])).max() <= 1e-4


def test_grouped_model_converges():
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (GroupedBinnedPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(8, 20_000, seed=3, device=torch.device("cpu"))
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    model = GroupedBinnedPopulationSMFModel(aux_data=torch_population_data(data))
    res = model.run_gauss_newton(data["guess"])
    print(f"grouped model: loss={res.fun:.3e} nit={res.nit} nfev={res.nfev}")
    _check_result(res, 8)
    assert res.jac_mode == "forward"
    assert res.nit <= 20 and res.fun <= 1e-6


def test_param_bounds_are_refused_and_psd_is_not_an_option():
    model = _user_model()
    with pytest.raises(ValueError):
        model.run_gauss_newton(_params(), param_bounds=[(-1.0, 1.0)] * 3)
    with pytest.raises(TypeError):
        model.run_gauss_newton(_params(), psd=False)


def test_example_runs():
    env = dict(os.environ, MULTIGRAD_PROGRESS="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "user_model_gauss_newton.py"),
                          "--num-pops", "2", "--num-halos", "4000"], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Gauss-Newton" in out.stdout and "Fisher" in out.stdout
