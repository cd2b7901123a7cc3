"""The inverse-Hessian operator's kernels (csrc/lbfgs.hip: lincomb_cols, compact_diag) against
fp64 references with derived bounds, and the operator end to end (run on an MI355X)."""
import numpy as np
import pytest
import scipy.linalg
import scipy.optimize
import torch

from multigrad_amd.ops.lbfgs import MultiDot, compact_diag_, lincomb_, lincomb_cols_

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
# the grid is capped at 2048 workgroups of 256 threads, a float4 each: one sweep covers at
# most 2048 * 256 * 4 elements, so here the grid-stride loop runs a second time
N_TWO_SWEEPS = 2048 * 256 * 4 + 1028
# 1, 255, 1_000_003: odd row stride -> scalar path; 1_000_000 and N_TWO_SWEEPS: float4 path;
# (255, 256): float4 path with a 3-element scalar tail
SIZES = [(1, 1), (255, 255), (255, 256), (1_000_003, 1_000_003), (1_000_000, 1_000_000),
         (N_TWO_SWEEPS, N_TWO_SWEEPS)]
ALPHA = float(np.float32(0.37))  # exact in fp32: the kernel takes alpha as a float

_H = {}


def _rows(nrows, n, ld):
    """``nrows`` random history rows of length ``n`` with row stride ``ld`` (made once)."""
    key = (nrows, n, ld)
    if key not in _H:
        _H.clear()  # one large buffer at a time
        g = torch.Generator(device=DEV).manual_seed(nrows * 7919 + n)
        _H[key] = torch.randn((nrows, ld), generator=g, device=DEV)[:, :n]
    return _H[key]


def _vec(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV)


# Bound for lincomb_cols.  Per element the kernel computes t0 = fl(alpha x) and then
# t_{i+1} = fl(c_i h_i + t_i) for rows i = 0..nrows-1, one rounding each (fmaf), so
#   y = alpha x (1+d_0)...(1+d_nrows) + sum_i c_i h_i (1+d_{i+1})...(1+d_nrows),  |d| <= u,
# i.e. at most nrows + 1 roundings on any term:
#   |y - exact| <= ((1+u)^(nrows+1) - 1) (|alpha x| + sum_i |c_i h_i|)
#               <= (nrows + 2) u (|alpha x| + sum_i |c_i h_i|)      for nrows <= 256.
# `pre` multiplies the first term once more and `post` the whole sum once more: one more
# rounding each, (nrows + 4) u against |post| (|alpha x pre| + sum_i |c_i h_i|).
@pytest.mark.parametrize("n,ld", SIZES)
@pytest.mark.parametrize("nrows", [2, 20, 34, 240])
def test_lincomb_cols_bound_and_determinism(nrows, n, ld):
    H = _rows(nrows, n, ld)
    H64 = H.double()
    for nc in (1, 2, 3, 4):
        coef = _vec((nrows, nc), 10 + nc)
        # [nc, n] blocks whose row stride follows ld (odd stride: the scalar path)
        x = _vec((nc, ld), 20 + nc)[:, :n]
        pre, post = _vec(ld, 30 + nc)[:n].contiguous(), _vec(ld, 40 + nc)[:n].contiguous()
        rowsum = coef.double().T @ H64                       # [nc, n]
        rowmag = coef.double().abs().T @ H64.abs()
        for use_x, use_pp in ((True, False), (True, True), (False, False), (False, True)):
            y = torch.full((nc, ld), float("nan"), device=DEV)[:, :n]
            lincomb_cols_(H, nrows, coef, ALPHA, x if use_x else None, y,
                          pre=pre if use_pp else None, post=post if use_pp else None)
            ref, mag = rowsum.clone(), rowmag.clone()
            if use_x:
                t = ALPHA * x.double() * (pre.double() if use_pp else 1.0)
                ref, mag = ref + t, mag + t.abs()
            if use_pp:
                ref, mag = ref * post.double(), mag * post.double().abs()
            bound = (nrows + (4 if use_pp else 2)) * U * mag
            err = (y.double() - ref).abs()
            worst = float((err / bound.clamp_min(1e-300)).max())
            print(f"lincomb_cols nrows={nrows} n={n} ld={ld} nc={nc} x={use_x} pp={use_pp}: "
                  f"max err/bound = {worst:.3f}")
            assert bool((err <= bound).all()), (nc, use_x, use_pp, worst)
            y2 = torch.empty_like(y)
            lincomb_cols_(H, nrows, coef, ALPHA, x if use_x else None, y2,
                          pre=pre if use_pp else None, post=post if use_pp else None)
            assert torch.equal(y, y2)
            if nc == 1 and use_x and not use_pp:
                # the same order as the one-column `lincomb`: bitwise equal
                y1 = torch.empty(n, device=DEV)
                lincomb_(H, nrows, coef[:, 0].contiguous(), ALPHA, x[0], y1)
                assert torch.equal(y[0], y1)


def test_lincomb_cols_rejects_bad_shapes():
    H = _rows(2, 255, 255)
    y = torch.empty((5, 255), device=DEV)
    with pytest.raises(ValueError):
        lincomb_cols_(H, 2, torch.zeros((2, 5), device=DEV), 1.0, None, y)
    with pytest.raises(ValueError):
        lincomb_cols_(H, 2, torch.zeros((2, 3), device=DEV), 1.0, None, y[:4])


def _compact_q(SY, YY, h0):
    k = SY.shape[0]
    Rinv = scipy.linalg.solve_triangular(np.triu(SY), np.eye(k), lower=False)
    A = Rinv.T @ (np.diag(np.diag(SY)) + h0 * YY) @ Rinv
    Q = np.block([[A, -Rinv.T], [-Rinv, np.zeros((k, k))]])
    return 0.5 * (Q + Q.T)


# Bound for compact_diag.  With w_a = fl(fac_a h_a) (one rounding per factor, two factors
# per term) the kernels evaluate out = h0 + sum_{a <= b} m_ab Q_ab w_a w_b (m = 1 on the
# diagonal, 2 off it: exact) as nested fmaf chains.  With k2 <= 40 term (a, b) passes through
# the chain of row a and then the outer chain, at most 2 k2 roundings; beyond that (tiles of
# 8 rows) through at most 8 + (k2 / 8 + 1) k2.  Neither exceeds what the flat chain over all
# T = k2 (k2 + 1) / 2 + 1 terms would give (T - 1 fused steps and the final one: the T + 1 of
# the lincomb_cols bound with nrows + 1 = T terms), for any k2 >= 2; add the 2 of the w factors:
#   |out - exact| <= (T + 3) u (|h0| + sum_{a <= b} m_ab |Q_ab w_a w_b|),
# and 2 more for `scale` (fl(s s), then the product): (T + 5) u.
@pytest.mark.parametrize("n,ld", SIZES)
# k = 21: 2k = 42 rows, the tiled kernel with a partial strip (32 + 10) and a partial tile (8 + 2)
@pytest.mark.parametrize("k", [1, 10, 17, 21, 120])
def test_compact_diag_bound(k, n, ld):
    R = k + 1  # a ring with a spare slot, the accepted slots rotated (oldest first)
    order = np.roll(np.arange(R), -2)[:k]
    g = torch.Generator(device=DEV).manual_seed(k * 104729 + n)
    H = torch.zeros((2 * R, ld), device=DEV)[:, :n]
    H[:R] = torch.randn((R, n), generator=g, device=DEV)
    H[R:] = H[:R] + 0.3 * torch.randn((R, n), generator=g, device=DEV)
    idx = torch.as_tensor(order, device=DEV)
    S64, Y64 = H[idx].double(), H[R + idx].double()
    if n >= 4 * k:
        SY, YY = (S64 @ Y64.T).cpu().numpy(), (Y64 @ Y64.T).cpu().numpy()
    else:  # fewer elements than independent pairs need: Q from pairs of their own
        Sa = torch.randn((k, 4 * k + 8), generator=g, device=DEV, dtype=torch.float64)
        Ya = Sa + 0.3 * torch.randn((k, 4 * k + 8), generator=g, device=DEV, dtype=torch.float64)
        SY, YY = (Sa @ Ya.T).cpu().numpy(), (Ya @ Ya.T).cpu().numpy()
    h0 = float(np.float32(SY[-1, -1] / YY[-1, -1]))
    Q = torch.from_numpy(_compact_q(SY, YY, h0).astype(np.float32)).to(DEV)
    rows = torch.from_numpy(np.concatenate([order, R + order]).astype(np.int32)).to(DEV)
    fac = torch.cat([torch.ones(k), torch.full((k,), h0)]).to(DEV)
    scale = _vec(ld, 50 + k)[:n].contiguous()
    W = torch.cat([S64, Y64]) * fac.double()[:, None]
    quad = ((Q.double() @ W) * W).sum(0)
    qmag = ((Q.double().abs() @ W.abs()) * W.abs()).sum(0)
    T = (2 * k) * (2 * k + 1) // 2 + 1
    for use_scale in (False, True):
        out = torch.full((n,), float("nan"), device=DEV)
        compact_diag_(H, rows, fac, Q, h0, out, scale=scale if use_scale else None)
        ref, mag = h0 + quad, abs(h0) + qmag
        if use_scale:
            s2 = scale.double() ** 2
            ref, mag = ref * s2, mag * s2
        bound = (T + (5 if use_scale else 3)) * U * mag
        err = (out.double() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"compact_diag k={k} n={n} ld={ld} scale={use_scale}: max err/bound = {worst:.4f}")
        assert bool((err <= bound).all()), (use_scale, worst)
        out2 = torch.empty_like(out)
        compact_diag_(H, rows, fac, Q, h0, out2, scale=scale if use_scale else None)
        assert torch.equal(out, out2)


# ---------------------------------------------------------------------------- end to end
# The inner products of both paths are fp32 lane sums (MultiDot), so this tolerance is
# measured, not derived: the new path may err twice as much as the same product composed from
# MultiDot + lincomb_ on the gathered pairs (another summation order, the same precision).
# Measured on an MI355X, max |error| / max |reference| of H v against scipy's fp64 operator on
# the same pairs, one random v:
#   free (L-BFGS,   k = 4): composed 1.745e-07, operator 2.941e-07
#   box  (L-BFGS-B, k = 2): composed 1.295e-07, operator 1.659e-07
E2E_COMPOSED = {"free": 1.745e-07, "box": 1.295e-07}


def _composed(sk, yk, v):
    """``H v`` (h0 = 1) from one MultiDot and one lincomb_ over the gathered pairs."""
    k, P = sk.shape
    A = torch.from_numpy(np.concatenate([sk, yk])).float().to(DEV).contiguous()
    vt = torch.from_numpy(v).float().to(DEV)
    dots = MultiDot(2 * k, P, DEV)(A, 2 * k, [vt])[:, 0].cpu().numpy()
    SY, YY = sk @ yk.T, yk @ yk.T
    z = _compact_q(SY, YY, 1.0) @ dots
    y = torch.empty(P, device=DEV)
    lincomb_(A, 2 * k, torch.from_numpy(z.astype(np.float32)).to(DEV), 1.0, vt, y)
    return y.double().cpu().numpy()


@pytest.mark.parametrize("case", ["free", "box"])
def test_population_engine_hess_inv(case):
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    data = make_population_data(num_params=2000, num_halos=200_000, seed=9, device=DEV)
    model = PopulationSMFModel(aux_data=data)
    model.set_target_from_truth()
    bounds = None
    if case == "box":
        bounds = [(float(v) - 0.05, float(v) + 0.2) for v in data["guess"].cpu().numpy()]
    res = model.run_bfgs(data["guess"], maxsteps=15, method="device", param_bounds=bounds)
    op = res.hess_inv
    P, k = 2000, op.n_corrs
    assert op.shape == (P, P) and 1 <= k <= 10
    sk, yk = op.pairs()
    v = np.random.default_rng(11).normal(size=P)
    want = scipy.optimize.LbfgsInvHessProduct(sk, yk) @ v
    scale = np.abs(want).max()
    err_new = np.abs(op.with_h0(1.0) @ v - want).max() / scale
    err_old = np.abs(_composed(sk, yk, v) - want).max() / scale
    print(f"hess_inv e2e {case}: k={k} new {err_new:.3e} composed {err_old:.3e} (relative to max|Hv|)")
    # the composed error of this run counts too: a changed lane-sum order moves both paths
    assert err_new <= 2 * max(err_old, E2E_COMPOSED[case])
    # diagonal() against the diagonal of the 2000 unit-vector products.  For e_j the inner
    # products are exact (one non-zero term), so column j errs by the fp32 rounding of its
    # 2 R coefficients and the fmaf chain: (2 R + 3) u mag_j; compact_diag errs by
    # (T + 3) u mag_j (above) plus the fp32 roundings of Q (1) and of the two h0 factors (2):
    D = op.todense()
    h0 = op.h0
    W = np.concatenate([sk, h0 * yk])
    mag = h0 + ((np.abs(op._Q()) @ np.abs(W)) * np.abs(W)).sum(0)
    T = (2 * k) * (2 * k + 1) // 2 + 1
    bound = (T + 6 + 2 * op.R + 3) * U * mag
    derr = np.abs(op.diagonal().double().cpu().numpy() - np.diag(D))
    print(f"hess_inv e2e {case}: diagonal max err/bound = {(derr / bound).max():.4f}")
    assert (derr <= bound).all()
