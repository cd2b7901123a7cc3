"""``res.hess_inv`` of the device L-BFGS / L-BFGS-B (optim/invhess.py): CPU / gloo coverage.

The CPU fallbacks of the operator's kernels accumulate in fp64 and store fp32, and both
sides of every comparison see the same fp32 pairs, so the bound on a product is the fp32
rounding of the output: ``atol = 4 * 2**-24 * max|ref|``.
"""
import numpy as np
import pytest
import scipy.optimize
import torch

import multigrad_amd as mg
from multigrad_amd.models.population import PopulationSMFModel, make_population_data
from multigrad_amd.models.smf import DocsSMFModel, make_docs_data
from multigrad_amd.optim import lbfgs as L
from multigrad_amd.optim import lbfgsb as LB
from multigrad_amd.optim.invhess import DeviceLbfgsInvHessProduct
from multigrad_amd.optim.transforms import Bounds
from multigrad_amd.parallel import comm as C

from distributed import run_distributed

U = 2.0 ** -24
N, M = 12, 5


def _atol(ref):
    return 4 * U * np.abs(ref).max()


def _rosen_lg(x):
    xx = x.detach().double().requires_grad_(True)
    with torch.enable_grad():
        f = (100 * (xx[1:] - xx[:-1] ** 2) ** 2 + (1 - xx[:-1]) ** 2).sum()
        (g,) = torch.autograd.grad(f, xx)
    return f.detach(), g.float()


def _x0():
    return 0.3 + 0.1 * torch.arange(N, dtype=torch.float32) / N


def _run(kind, **kw):
    if kind == "lbfgs":
        return L.run_lbfgs_device(_rosen_lg, _x0(), maxsteps=40, history=M, **kw)
    if kind == "lbfgsb":  # a box that stays inactive
        return LB.run_lbfgsb_device(_rosen_lg, _x0(), maxsteps=40, history=M,
                                    param_bounds=[(-10.0, 10.0)] * N, **kw)
    return L.run_lbfgs_device(_rosen_lg, _x0(), maxsteps=40, history=M,
                              param_bounds=[(0.0, 2.0)] * N, **kw)


_CACHE = {}


def _res(kind):
    if kind not in _CACHE:
        _CACHE[kind] = _run(kind)
    return _CACHE[kind]


def _dense_bfgs(sk, yk, h0):
    """The BFGS recursion over the pairs (oldest first) from ``h0 I``, in fp64."""
    n = sk.shape[1]
    H = h0 * np.eye(n)
    for s, y in zip(sk, yk):
        rho = 1.0 / (s @ y)
        V = np.eye(n) - rho * np.outer(s, y)
        H = V @ H @ V.T + rho * np.outer(s, s)
    return H


# ------------------------------------------------------------------ contract
@pytest.mark.parametrize("bounds", [None, [(-5.0, 0.0), (-3.0, 3.0)]])
def test_run_bfgs_device_returns_hess_inv(bounds):
    C.set_world_comm(None)
    model = DocsSMFModel(aux_data=make_docs_data(device="cpu"), device="cpu")
    res = model.run_bfgs(torch.tensor([-3.5, 0.2]), method="device", param_bounds=bounds)
    assert isinstance(res.hess_inv, DeviceLbfgsInvHessProduct)
    assert res.hess_inv.shape == (2, 2) and res.hess_inv.dtype == np.float64
    assert res.hess_inv.todense().shape == (2, 2)
    off = model.run_bfgs(torch.tensor([-3.5, 0.2]), method="device", param_bounds=bounds,
                         hess_inv=False)
    assert "hess_inv" not in off
    np.testing.assert_array_equal(off.x.numpy(), res.x.numpy())  # nothing else changes


def test_hess_inv_keyword_of_the_drivers():
    for kind in ("lbfgs", "lbfgsb", "transform"):
        assert "hess_inv" not in _run(kind, hess_inv=False)
        assert "hess_inv" in _res(kind)


# ------------------------------------------------------------------ scipy parity
@pytest.mark.parametrize("kind", ["lbfgs", "lbfgsb"])
def test_with_h0_one_is_scipys_operator(kind):
    op = _res(kind).hess_inv
    assert op.n_corrs == M and op.shape == (N, N)
    sk, yk = op.pairs()
    assert sk.shape == yk.shape == (M, N) and sk.dtype == np.float64
    ref = scipy.optimize.LbfgsInvHessProduct(sk, yk)
    op1 = op.with_h0(1.0)
    assert op1.h0 == 1.0 and op1.HS is op.HS
    rng = np.random.default_rng(1)
    for _ in range(3):
        v = rng.normal(size=N)
        want = ref @ v
        np.testing.assert_allclose(op1 @ v, want, rtol=0, atol=_atol(want))
    D = ref.todense()
    np.testing.assert_allclose(op1.todense(), D, rtol=0, atol=_atol(D))


# ------------------------------------------------------------------ default scaling
@pytest.mark.parametrize("kind", ["lbfgs", "lbfgsb"])
def test_default_scaling_is_the_optimizers(kind):
    res = _res(kind)
    op = res.hess_inv
    sk, yk = op.pairs()
    gamma = (sk[-1] @ yk[-1]) / (yk[-1] @ yk[-1])
    assert op.h0 == pytest.approx(gamma, rel=1e-12)
    H = _dense_bfgs(sk, yk, gamma)
    v = np.random.default_rng(2).normal(size=N)
    np.testing.assert_allclose(op @ v, H @ v, rtol=0, atol=_atol(H @ v))
    # the next unbounded direction: -(H g) from the optimizer's own coefficients
    g = res.jac.double().numpy()
    order = list(range(M))
    gm, a, b = L.compact_coefficients(sk @ yk.T, yk @ yk.T, sk @ g, yk @ g, order)
    d = -(gm * g + sk.T @ a + gm * (yk.T @ b))
    got = -op.apply(res.jac).double().numpy()
    np.testing.assert_allclose(got, d, rtol=0, atol=_atol(d))


# ------------------------------------------------------------------ diagonal, chunks
@pytest.mark.parametrize("kind", ["lbfgs", "lbfgsb", "transform"])
def test_diagonal_and_column_chunks(kind):
    op = _res(kind).hess_inv
    D = op.todense()
    dg = op.diagonal()
    assert dg.dtype == torch.float32 and dg.shape == (N,)
    np.testing.assert_allclose(dg.double().numpy(), np.diag(D), rtol=0, atol=_atol(np.diag(D)))
    X = np.random.default_rng(3).normal(size=(N, 7))  # chunks of 4 + 3 columns
    got = op.matmat(X)
    assert got.shape == (N, 7) and got.dtype == np.float64
    for c in range(7):
        np.testing.assert_array_equal(got[:, c], op.matvec(X[:, c]))
    out = op.apply(torch.from_numpy(X))
    assert out.dtype == torch.float32 and out.shape == (N, 7)


# ------------------------------------------------------------------ transform mode
def test_transform_mode_is_J_Hu_J():
    res = _res("transform")
    op = res.hess_inv
    b = Bounds.from_spec([(0.0, 2.0)] * N, N, device="cpu", dtype=torch.float32)
    J = op.jac.double().numpy()
    np.testing.assert_allclose(J, b.dpdu(b.forward(res.x)).double().numpy(), rtol=1e-4)
    assert (J > 0).all() and not np.allclose(J, 1.0)
    sk, yk = op.pairs()  # u-space pairs
    Hu = _dense_bfgs(sk, yk, op.h0)
    want = J[:, None] * Hu * J[None, :]
    np.testing.assert_allclose(op.todense(), want, rtol=0, atol=_atol(want))
    want1 = J[:, None] * scipy.optimize.LbfgsInvHessProduct(sk, yk).todense() * J[None, :]
    np.testing.assert_allclose(op.with_h0(1.0).todense(), want1, rtol=0, atol=_atol(want1))


# ------------------------------------------------------------------ pending pair, no pair
def test_lbfgsb_counts_the_pending_pair():
    xs = []
    res = LB.run_lbfgsb_device(_rosen_lg, _x0(), maxsteps=200, history=100, ftol=1e-7,
                               param_bounds=[(-10.0, 10.0)] * N,
                               callback=lambda x: xs.append(x.clone()))
    assert "REL_REDUCTION" in res.message, res.message
    op = res.hess_inv
    assert res.nit < 100 and op.n_corrs == res.nit  # the last step's pair included
    sk, _ = op.pairs()
    last = (xs[-1].double() - xs[-2].double()).numpy()
    torch.testing.assert_close(xs[-1], res.x)
    np.testing.assert_allclose(sk[-1], last, rtol=0, atol=4 * U * np.abs(xs[-1].numpy()).max())


@pytest.mark.parametrize("kind", ["lbfgs", "lbfgsb"])
def test_no_pair_gives_the_identity(kind):
    run = L.run_lbfgs_device if kind == "lbfgs" else LB.run_lbfgsb_device
    kw = {} if kind == "lbfgs" else dict(param_bounds=[(-10.0, 10.0)] * N)
    op = run(_rosen_lg, _x0(), maxsteps=0, history=M, **kw).hess_inv
    assert op.n_corrs == 0 and op.h0 == 1.0
    np.testing.assert_array_equal(op.todense(), np.eye(N))
    np.testing.assert_array_equal(op.diagonal().numpy(), np.ones(N, dtype=np.float32))
    sk, yk = op.pairs()
    assert sk.shape == yk.shape == (0, N)


def test_limits():
    op = _res("lbfgs").hess_inv
    big = DeviceLbfgsInvHessProduct.__new__(DeviceLbfgsInvHessProduct)
    big.__dict__.update(op.__dict__)
    big.shape = (8193, 8193)
    with pytest.raises(ValueError):
        big.todense()
    big.shape = ((1 << 27) // M + 1,) * 2
    with pytest.raises(ValueError):
        big.pairs()
    with pytest.raises(ValueError):
        op.apply(torch.zeros(N + 1))


# ------------------------------------------------------------------ several ranks (gloo)
def _pop_hess(rank, size, zero, placement="hashed"):
    """The population model of tests/test_lbfgs.py (80 parameters, 3000 halos)."""
    comm = mg.get_world_comm()
    data = make_population_data(num_params=80, num_halos=3000, seed=3, comm=comm, device="cpu",
                                placement=placement)
    m = PopulationSMFModel(aux_data=data, comm=comm)
    m.set_target_from_truth()
    xs = []
    res = m.run_bfgs(data["guess"], maxsteps=30, method="device", zero=zero, chunks=3,
                     callback=lambda x: xs.append(x.detach().clone()))
    # run_bfgs leaves the model's engine cached and open: close it (collective) and spoil
    # what the layout must own a copy of, then use the operator
    engines = list(m._engine_cache.values())
    assert engines and not any(e.closed for e in engines)
    for e in engines:
        e.close()
        if e.pidx is not None:
            e.pidx.zero_()
            e.inv_pidx.zero_()
        e.theta = None
        e.pb, e.lengths = [], []
    assert all(e.closed for e in engines)
    op = res.hess_inv
    v = np.random.default_rng(5).normal(size=80)
    sk, yk = op.pairs()
    last = (xs[-1].double() - xs[-2].double()).numpy()
    return (op @ v, op.diagonal().numpy(), sk, yk, op.with_h0(1.0) @ v, op.n_corrs,
            res.x.numpy(), last)


@pytest.mark.parametrize("size,zero,placement", [(2, True, "hashed"), (3, True, "owner")])
def test_sharded_operator(size, zero, placement):
    res = run_distributed(_pop_hess, size, zero, placement)
    v = np.random.default_rng(5).normal(size=80)
    for r in res[1:]:
        for a, b in zip(r, res[0]):
            np.testing.assert_array_equal(a, b)
    hv, dg, sk, yk, hv1, k, x, last = res[0]
    assert k == sk.shape[0] > 0 and sk.shape == yk.shape == (k, 80)
    # user order: the newest s is the optimizer's last step as the callback saw it (x in
    # the user's order; x_new = fl(x_old + s) in fp32, so to one rounding of x)
    np.testing.assert_allclose(sk[-1], last, rtol=0, atol=4 * U * np.abs(x).max())
    assert np.abs(sk[-1]).max() > 100 * 4 * U * np.abs(x).max()  # the check can tell orders apart
    want = scipy.optimize.LbfgsInvHessProduct(sk, yk) @ v
    np.testing.assert_allclose(hv1, want, rtol=0, atol=_atol(want))
    gamma = (sk[-1] @ yk[-1]) / (yk[-1] @ yk[-1])
    H = _dense_bfgs(sk, yk, gamma)
    np.testing.assert_allclose(hv, H @ v, rtol=0, atol=_atol(H @ v))
    np.testing.assert_allclose(dg, np.diag(H), rtol=0, atol=_atol(np.diag(H)))


def test_engine_layout_follows_the_engines_permutation():
    """``_EngineLayout`` against the engine's own order maps (``to_user``, the ``p0[pidx]`` of
    setup) on a stand-in engine with a non-trivial, padded internal order."""
    from types import SimpleNamespace
    from multigrad_amd.engine.fused import _EngineLayout
    P, P_pad = 10, 12
    pidx = torch.tensor([4, 5, 0, 1, 8, 9, 2, 3, 6, 7])
    inv = torch.empty_like(pidx)
    inv[pidx] = torch.arange(P)
    eng = SimpleNamespace(comm=None, size=1, rank=0, device=torch.device("cpu"), P=P, P_pad=P_pad,
                          pidx=pidx, inv_pidx=inv, pb=[0, P_pad], lengths=[P_pad], owner=False,
                          zero=False)
    lay = _EngineLayout(eng)
    v = torch.arange(2 * P, dtype=torch.float32).reshape(2, P)
    loc = lay.to_local(v)
    assert loc.shape == (2, P_pad)
    torch.testing.assert_close(loc[:, :P], v[:, pidx])          # as setup: theta[:P] = p0[pidx]
    assert float(loc[:, P:].abs().max()) == 0.0
    torch.testing.assert_close(lay.from_local(loc), v)           # as to_user: t[..., inv_pidx]
    torch.testing.assert_close(lay.from_local(loc), loc[:, :P][:, inv])
    eng.pidx.zero_()                                             # the layout owns its copies
    torch.testing.assert_close(lay.from_local(lay.to_local(v)), v)


def test_objective_without_vector_layout():
    """An objective of the documented protocol (no ``vector_layout``) still gets its operator."""
    class Plain:
        def __init__(self):
            self.comm, self.sharded, self.device = None, False, torch.device("cpu")
            self.n_local = N

        def x0(self):
            return _x0()

        def full(self, x):
            return x

        def __call__(self, x):
            f, g = _rosen_lg(x)
            return float(f), g

    for res in (L.lbfgs_minimize(Plain(), maxiter=10, m=M),
                LB.lbfgsb_minimize(Plain(), maxiter=10, m=M)):
        op = res.hess_inv
        sk, yk = op.pairs()
        want = scipy.optimize.LbfgsInvHessProduct(sk, yk).todense()
        np.testing.assert_allclose(op.with_h0(1.0).todense(), want, rtol=0, atol=_atol(want))
