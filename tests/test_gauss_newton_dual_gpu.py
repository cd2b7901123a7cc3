"""The one-pass SMF Jacobian kernel, the weighted_gram kernel and the dual Gauss-Newton fit
on the MI355X, against float64 oracles."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64


def _S():
    from multigrad_amd.ops import smf
    return smf


def _check_rows(jac, ref):
    """The project's gradient contract, per row of the Jacobian."""
    jac, ref = jac.double().cpu().numpy(), ref.cpu().numpy()
    assert np.isfinite(jac).all()
    for k in range(ref.shape[0]):
        np.testing.assert_allclose(jac[k], ref[k], rtol=2e-4, atol=2e-5 * np.abs(ref[k]).max(),
                                   err_msg=f"row {k}")


# ---------------------------------------------------------------- 1. smf_jacobian_into
@functools.lru_cache(maxsize=None)
def _case(giant, nb):
    """Halos, parameters, bins and the float64 Jacobian of the PyTorch reference on the
    float32-rounded inputs (computed once per case, on the device)."""
    S = _S()
    n, npop = 200_000, 300
    g = torch.Generator().manual_seed(0)
    x = 10.0 + torch.rand(n, generator=g, dtype=F64)
    pop = torch.randint(0, npop, (n,), generator=g)
    if giant is not None:   # half the halos in one population: split into parts
        pop[: n // 2] = giant
    g = torch.Generator().manual_seed(1)
    theta = torch.empty(2 * npop, dtype=F64)
    theta[0::2] = -2.0 + 0.2 * (torch.rand(npop, generator=g, dtype=F64) - 0.5)
    theta[1::2] = -0.5 + 0.2 * (torch.rand(npop, generator=g, dtype=F64) - 0.5)
    bins = S.SmfBins.make(np.linspace(8.0, 9.6, nb + 1), volume=1e4)
    xf, th = x.float(), theta.float()
    xd, pd = xf.double().to(DEV), pop.to(DEV)
    ref = torch.autograd.functional.jacobian(
        lambda t: S.smf_sumstats_reference(t, xd, pd, bins, True), th.double().to(DEV))
    return xf, pop, th.to(DEV), bins, ref


def _shard(giant, nb, **kw):
    xf, pop, th, bins, ref = _case(giant, nb)
    shard = _S().PopulationShard(xf, pop.int().to(DEV), 300, device=DEV, chunks=3, **kw)
    return shard, th, bins, ref


@pytest.mark.parametrize("nb", [10, 7, 3])
@pytest.mark.parametrize("giant", [None, 3])
def test_lanes_jacobian_matches_fp64(giant, nb):
    S = _S()
    shard, th, bins, ref = _shard(giant, nb)
    assert shard.layout == "lanes" and not shard.vjp_recompute
    assert (shard.giant.shape[0] > 0) == (giant is not None)
    jac = torch.full((nb, th.numel()), float("nan"), device=DEV)
    assert S.smf_jacobian_into(th, shard, bins, True, jac) is jac
    _check_rows(jac, ref)
    # a second call, and one on residuals the caller has just written: the same bits
    again = torch.full_like(jac, float("nan"))
    S.smf_jacobian_into(th, shard, bins, True, again)
    assert torch.equal(again, jac)
    out = torch.zeros(bins.nbp, device=DEV)
    S.smf_forward_into(th, shard, bins, True, out, resid=True)
    ready = torch.full_like(jac, float("nan"))
    S.smf_jacobian_into(th, shard, bins, True, ready, residuals_ready=True)
    assert torch.equal(ready, jac)
    # the convenience form
    s, j2 = S.smf_sumstats_and_jacobian(th, shard, bins)
    assert torch.equal(j2, jac) and torch.allclose(s, out[:nb], rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("nb", [10, 7, 3])
@pytest.mark.parametrize("giant", [None, 3])
def test_lanes_jacobian_per_chunk(giant, nb):
    S = _S()
    shard, th, bins, ref = _shard(giant, nb)
    assert shard.nchunks == 3
    jac = torch.full((nb, th.numel()), float("nan"), device=DEV)
    for c in range(3):
        before = jac.clone()
        S.smf_jacobian_into(th, shard, bins, True, jac, chunk=c)
        p0, p1 = shard.chunk_pops[c], shard.chunk_pops[c + 1]
        same = (jac == before) | (jac.isnan() & before.isnan())
        assert bool(same[:, :2 * p0].all()) and bool(same[:, 2 * p1:].all())
        assert not bool(jac[:, 2 * p0:2 * p1].isnan().any())
    _check_rows(jac, ref)


@pytest.mark.parametrize("kw", [dict(lane_order="local"), dict(layout="tiles")],
                         ids=["lanes-local", "tiles"])
@pytest.mark.parametrize("nb", [10, 7, 3])
@pytest.mark.parametrize("giant", [None, 3])
def test_fallback_jacobian_matches_fp64(giant, nb, kw):
    """The nb-pass path (one VJP per unit cotangent) under the same contract, whole and per
    chunk."""
    S = _S()
    shard, th, bins, ref = _shard(giant, nb, **kw)
    assert shard.vjp_recompute or shard.layout == "tiles"
    jac = torch.full((nb, th.numel()), float("nan"), device=DEV)
    S.smf_jacobian_into(th, shard, bins, True, jac)
    _check_rows(jac, ref)
    per_chunk = torch.full_like(jac, float("nan"))
    for c in range(3):
        S.smf_jacobian_into(th, shard, bins, True, per_chunk, chunk=c)
    _check_rows(per_chunk, ref)


# ---------------------------------------------------------------- 2. narrow populations
def test_lanes_jacobian_with_per_edge_groups():
    """log10 sigma = -1.1 on every tenth population: bin width 1.26 sigma, outside the
    Euler-Maclaurin range, so their lane groups take the forward's per-edge path."""
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    S = _S()
    data = make_population_data(num_params=4000, num_halos=400_000, seed=5, device=DEV)
    shard, bins = data["shard"], data["bins"]
    th = data["guess"].clone()
    th[1::20] = -1.1
    fallback, groups = PopulationSMFModel(aux_data=data).lane_fallback_groups(th)
    assert 0 < fallback <= groups
    ref = torch.autograd.functional.jacobian(
        lambda t: S.smf_sumstats_reference(t, shard.x.double(), shard.pop, bins, True), th.double())
    jac = torch.full((bins.nb, th.numel()), float("nan"), device=DEV)
    S.smf_jacobian_into(th, shard, bins, True, jac)
    _check_rows(jac, ref)


# ---------------------------------------------------------------- 3. weighted_gram
GRAM_SHAPES = [
    pytest.param(1, 1003, False, id="K1-float4-plus-tail"),
    pytest.param(10, 4096, False, id="K10-float4"),
    pytest.param(10, 37, False, id="K10-one-workgroup-scalar"),
    pytest.param(10, 4096, True, id="K10-misaligned-scalar"),
    pytest.param(16, 2052, False, id="K16-float4"),
    pytest.param(17, 1028, False, id="K17-tiled-float4"),
    pytest.param(40, 515, False, id="K40-tiled-scalar"),
    pytest.param(10, 1_100_000, False, id="K10-second-grid-stride-trip"),
]


def _on_device(t, misaligned):
    """A contiguous device copy of ``t``; ``misaligned``: 4 bytes past a 16-byte boundary."""
    if t is None:
        return None
    if not misaligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("K,n,misaligned", GRAM_SHAPES)
def test_weighted_gram_kernel(K, n, misaligned, weighted):
    from multigrad_amd.ops.gram import weighted_gram
    g = torch.Generator().manual_seed(K * n + weighted)
    # integer data: every product and sum is exact in float64
    Ji = torch.randint(-8, 9, (K, n), generator=g)
    wi = torch.randint(-8, 9, (n,), generator=g) if weighted else None
    out = weighted_gram(_on_device(Ji.float(), misaligned),
                        _on_device(None if wi is None else wi.float(), misaligned))
    assert out.dtype == F64 and out.shape == (K, K) and out.device == DEV
    exact = (Ji if wi is None else Ji * wi) @ Ji.T
    assert torch.equal(out.cpu(), exact.double())
    # normal data: the float64 summation bound, and the same bits from a second call
    J = torch.randn(K, n, generator=g)
    w = torch.rand(n, generator=g) + 0.1 if weighted else None
    Jd, wd = _on_device(J, misaligned), _on_device(w, misaligned)
    out = weighted_gram(Jd, wd)
    assert torch.equal(weighted_gram(Jd, wd), out)
    J64 = J.numpy().astype(np.float64)
    w64 = np.ones(n) if w is None else w.numpy().astype(np.float64)
    ref = (J64 * w64) @ J64.T
    bound = (n + 4) * 2.0 ** -53 * ((np.abs(J64) * np.abs(w64)) @ np.abs(J64).T)
    err = np.abs(out.cpu().numpy() - ref)
    print(f"K={K} n={n}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert torch.equal(out, out.T)
    # fewer rows of the same matrix
    k = max(K - 1, 1)
    sub = weighted_gram(Jd, wd, nrows=k).cpu().numpy()
    assert sub.shape == (k, k) and (np.abs(sub - ref[:k, :k]) <= bound[:k, :k]).all()


def test_weighted_gram_refuses_bad_arguments():
    from multigrad_amd.ops.gram import weighted_gram
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(0, 5, device=DEV))
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(257, 5, device=DEV))
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(3, 5, device=DEV), torch.zeros(4, device=DEV))
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(5, 3, device=DEV).T)
    with pytest.raises(ValueError):
        weighted_gram(torch.zeros(3, 5, device=DEV), torch.zeros(5))


# ---------------------------------------------------------------- 4. end to end
def test_population_model_dual_fit_beats_adam():
    """2 000 parameters, 54 000 halos: the dual fit succeeds on the native Jacobian and ends
    at or below the loss of 200 Adam steps from the same guess.  Nothing of the parameters'
    size is copied to the host by the driver: its own device->host copies are the packed
    K*K + K + 2 block per Jacobian (``host_copy_sizes``); copies made inside the model's
    hooks are not counted by this test."""
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    data = make_population_data(2000, 54_000, seed=3, device=DEV)
    model = PopulationSMFModel(aux_data=data)
    model.set_target_from_truth()
    guess = data["guess"]
    res = model.run_gauss_newton(guess, solver="dual")
    traj = model.run_adam(guess, nsteps=200, learning_rate=0.01)
    adam = float(model.calc_loss_from_params(traj[-1]))
    print(f"dual: fun={res.fun:.3e} nit={res.nit} njev={res.njev} nfev={res.nfev} "
          f"({res.message}); adam 200 steps: {adam:.3e}")
    assert res.success, res.message
    assert res.jac_mode == "native" and res.solver == "dual"
    assert res.fun <= adam
    assert res.x.is_cuda and res.x.shape == guess.shape and res.jac.is_cuda
    K = data["bins"].nb
    assert res.host_copy_sizes == [K * K + K + 2] * res.njev
    assert max(res.host_copy_sizes) < guess.numel()
    diag = res.hess_inv.diagonal()
    assert diag.is_cuda and diag.shape == (2000,) and bool(torch.isfinite(diag).all())
