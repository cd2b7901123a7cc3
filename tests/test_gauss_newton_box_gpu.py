"""The box_dual_pass kernel and the box-constrained Gauss-Newton fit on the MI355X.

Kernel bounds.  The oracle evaluates the same formulas in float64 numpy on the same float32
inputs, so both sides round; every bound below is the sum of the two.  With ``u = 2^-53``,
``gamma_m = m u / (1 - m u)`` (Higham, Accuracy and Stability, 3.1) and ``e`` the unit
roundoff of the per-column arithmetic (``u`` for the kernel and for the float64 torch path
that ``K > 10`` takes; ``2^-24`` for the composition of the ops, which keeps ``t``, ``sigma``
and ``delta`` as float32 vectors):

* ``t_p = sum_k a_k J_kp`` is a chain of ``K`` fused multiply-adds (numpy: ``K`` products
  and ``K - 1`` adds): ``|t - t_ref| <= et_p = 2 gamma_{K+2}(e) T_p``, ``T_p = sum_k |a_k J_kp|``.
* ``sigma = -t / (lam d)`` takes three more roundings on either side (``lam d``, the
  reciprocal, the product): ``|sigma - sigma_ref| <= es_p = et_p / (lam d_p) + 8 e |sigma_p|``.
* ``delta = sigma`` on a free column (error ``es_p``) and ``lo`` or ``hi`` exactly on a clipped
  one, provided both sides agree on ``free``: the inputs are built so that every column has
  ``min(|sigma - lo|, |sigma - hi|) >= max(1e-6 max(1, |sigma|), 4 es_p)`` (asserted), apart
  from the exact ties (a zero column of ``J`` with a zero side; ``lo = hi = 0``).
* ``delta_out`` is ``delta`` rounded to float32: ``<= 2^-24 |delta| + 2 es_p``.
* Each sum has at most ``n`` terms per thread chain and 30 more through the wave, LDS and
  slab reductions; ``m = n + 64`` covers it and the few roundings inside a term.  On either
  side ``|sum - exact| <= gamma_m sum |terms|``, so the sums differ by at most
  ``2 gamma_m sum |terms|`` plus what the error of ``delta`` and ``t`` carries into the terms:
  ``sum_p |J_kp| es_p`` (free columns) for ``v`` (and, for the composition, the float32 lane
  chains of ``MultiDot``, bounded as in tests/test_lbfgs_kernels.py), nothing for ``W`` (its weight ``1 / (lam d)``
  has three roundings, inside ``m``; ``4 e`` per term for the float32 weight of the
  composition) and ``sum_p es_p (|t_p| + lam d_p |delta_p|) + |delta_p| et_p`` for ``s``
  (plus ``4 e`` per term for the float32 ``lam d`` of the composition).
* The free count is exact.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64
U = 2.0 ** -53
LAM = 0.3
# above 1024 workgroups x 256 threads x 4 columns, the most the kernel launches: the
# grid-stride loop makes a second trip whatever the number of resident workgroups
N_SECOND_TRIP = 1024 * 256 * 4 + 1027


def _gamma(m, e):
    return m * e / (1.0 - m * e)


def _misaligned(t):
    """A contiguous device copy of ``t`` 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@functools.lru_cache(maxsize=2)
def _case(K, n, float32_columns=False):
    """Inputs (float32 numpy, ``a`` float64), the float64 oracle and the bounds, once per
    shape; ``float32_columns`` for the composition of the ops."""
    e = 2.0 ** -24 if float32_columns else U
    rng = np.random.default_rng(1000 * K + n % 997)
    J = rng.normal(size=(K, n)).astype(np.float32)
    a = rng.normal(size=K)
    d = (rng.random(n) + 0.1).astype(np.float32)
    zero = rng.random(n) < 0.05                    # exact tie: t = 0 against a zero side
    J[:, zero] = 0.0
    J64, ld = J.astype(np.float64), LAM * d.astype(np.float64)
    t = a @ J64
    T = np.abs(a) @ np.abs(J64)
    sigma = -t / ld
    et = 2.0 * _gamma(K + 2, e) * T
    es = et / ld + 8.0 * e * np.abs(sigma)
    scale = np.sqrt(K) / LAM
    lo = (-scale * rng.random(n)).astype(np.float32)
    hi = (scale * rng.random(n)).astype(np.float32)
    lo[rng.random(n) < 0.2] = -np.inf
    hi[rng.random(n) < 0.2] = np.inf
    side = rng.random(n)
    lo[zero & (side < 0.5)] = 0.0
    hi[zero & (side >= 0.5)] = 0.0
    fixed = rng.random(n) < 0.05
    lo[fixed], hi[fixed] = 0.0, 0.0
    # open a side that sigma comes too close to: a last-bit difference cannot flip `free`
    need = np.maximum(1e-6 * np.maximum(1.0, np.abs(sigma)), 4.0 * es)
    tie = (zero & ((lo == 0) | (hi == 0))) | fixed
    lo[(np.abs(sigma - lo) < need) & ~tie] = -np.inf
    hi[(np.abs(sigma - hi) < need) & ~tie] = np.inf
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    gap = np.minimum(np.abs(sigma - lo64), np.abs(sigma - hi64))
    assert (gap[~tie] >= need[~tie]).all()
    free = (sigma > lo64) & (sigma < hi64)
    assert not free[tie].any()
    delta = np.clip(sigma, lo64, hi64)
    w = free / ld
    ref = dict(v=J64 @ delta, W=(J64 * w) @ J64.T,
               s=float(np.sum(t * delta + 0.5 * ld * delta * delta)), nfree=int(free.sum()),
               delta=delta, free=free)
    g = 2.0 * _gamma(n + 64, U)
    es_free = np.where(free, es, 0.0)
    dot32 = 0.0
    if e > U:   # MultiDot forms each lane sum as a float32 fmaf chain (tests/test_lbfgs_kernels.py)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        chunks = max(n >> 2, 1)
        L = 4 * -(-chunks // (min(-(-chunks // 64), cus) * 64)) + 1
        dot32 = _gamma(L, 2.0 ** -24) + 2.0 ** -40
    bound = dict(
        v=(g + dot32) * (np.abs(J64) @ np.abs(delta)) + np.abs(J64) @ es_free,
        W=(g + (4.0 * e if e > U else 0.0)) * ((np.abs(J64) * w) @ np.abs(J64).T),
        s=g * float(np.sum(np.abs(t * delta) + 0.5 * ld * delta * delta))
        + float(np.sum(es_free * (np.abs(t) + ld * np.abs(delta)) + np.abs(delta) * et))
        + (4.0 * e * float(np.sum(0.5 * ld * delta * delta)) if e > U else 0.0),
        delta=2.0 ** -24 * np.abs(delta) + 2.0 * es_free)
    return J, a, d, lo, hi, ref, bound


def _padded(t):
    """A device copy of the ``[K, n]`` tensor ``t`` as a view into a wider buffer: 16-byte
    aligned, rows a multiple of 4 floats apart whatever ``n`` (the 16-byte-load layout)."""
    K, n = t.shape
    buf = torch.full((K, (n + 3) // 4 * 4 + 4), float("nan"), dtype=t.dtype, device=DEV)
    view = buf[:, :n]
    view.copy_(t)
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0 and view.stride(1) == 1
    return view


def _compare(out, delta_out, K, n, ref, bound, what):
    blk = out.cpu().numpy()
    v, W, s, nfree = blk[:K], blk[K:K + K * K].reshape(K, K), blk[-2], blk[-1]
    ratios = [np.max(np.abs(v - ref["v"]) / np.maximum(bound["v"], 1e-300)),
              np.max(np.abs(W - ref["W"]) / np.maximum(bound["W"], 1e-300)),
              abs(s - ref["s"]) / max(bound["s"], 1e-300)]
    print(f"K={K} n={n} {what}: err / bound: v {ratios[0]:.3f} W {ratios[1]:.3f} s {ratios[2]:.3f}")
    assert nfree == ref["nfree"]
    assert (np.abs(v - ref["v"]) <= bound["v"]).all()
    assert (np.abs(W - ref["W"]) <= bound["W"]).all() and np.array_equal(W, W.T)
    assert abs(s - ref["s"]) <= bound["s"]
    dl = delta_out.cpu().numpy().astype(np.float64)
    assert not np.isnan(dl).any()
    assert (np.abs(dl - ref["delta"]) <= bound["delta"]).all()
    clipped = ~ref["free"]
    assert np.array_equal(dl[clipped], ref["delta"][clipped])   # lo or hi exactly


@pytest.mark.parametrize("misaligned", [False, True], ids=["float4", "offset-one-float"])
@pytest.mark.parametrize("n", [1, 3, 4, 1027, N_SECOND_TRIP])
@pytest.mark.parametrize("K", [1, 2, 3, 10, 16, 20])
def test_box_dual_pass_kernel(K, n, misaligned):
    """K <= 10: the kernel.  ``float4`` is a 16-byte-aligned ``J`` with a padded row stride,
    so that the 16-byte-load kernel runs at every ``n >= 4`` (with a scalar tail at 1027 and
    on the second grid-stride trip); ``offset-one-float`` starts 4 bytes later and runs the
    scalar-load kernel.  Which of the two ran is asked of the extension and asserted.
    K = 16, 20: the float64 torch path, under the same bounds."""
    from multigrad_amd.ops.box_dual import MAX_FUSED_ROWS, box_dual_pass, vector_loads
    J, a, d, lo, hi, ref, bound = _case(K, n)
    Jd = _misaligned(torch.from_numpy(J)) if misaligned else _padded(torch.from_numpy(J))
    ad = torch.from_numpy(a).to(DEV)
    dd, lod, hid = (torch.from_numpy(x).to(DEV) for x in (d, lo, hi))
    fused = K <= MAX_FUSED_ROWS
    delta_out = torch.full((n,), float("nan"), device=DEV)
    vec = vector_loads(Jd, dd, lod, hid, delta_out)
    assert vec == vector_loads(Jd, dd, lod, hid)
    assert vec == (fused and not misaligned and n >= 4)
    big = n == N_SECOND_TRIP
    if big and fused:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
    out = box_dual_pass(Jd, ad, dd, LAM, lod, hid)
    if big and fused:   # the slab and the block only: nothing of size P
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - before < 4 * n
    assert out.dtype == F64 and out.shape == (K + K * K + 2,) and out.device == DEV
    again = box_dual_pass(Jd, ad, dd, LAM, lod, hid, delta_out)
    if fused:
        assert torch.equal(again, out)        # the same bits, with and without the write
        assert torch.equal(box_dual_pass(Jd, ad, dd, LAM, lod, hid, delta_out), out)
    path = ("16-byte loads" if vec else "scalar loads") if fused else "float64 torch path"
    _compare(again, delta_out, K, n, ref, bound, path)
    _compare(out, delta_out, K, n, ref, bound, path)


@pytest.mark.parametrize("n", [1027, N_SECOND_TRIP])
@pytest.mark.parametrize("K", [10, 16])
def test_composition_of_the_ops(K, n):
    """``box_dual_pass_composed``, the benchmark's baseline, under the bounds of float32
    per-column arithmetic (module docstring); the same bits from a second call."""
    from multigrad_amd.ops.box_dual import box_dual_pass_composed
    J, a, d, lo, hi, ref, bound = _case(K, n, True)
    Jd, ad = torch.from_numpy(J).to(DEV), torch.from_numpy(a).to(DEV)
    dd, lod, hid = (torch.from_numpy(x).to(DEV) for x in (d, lo, hi))
    delta_out = torch.full((n,), float("nan"), device=DEV)
    out = box_dual_pass_composed(Jd, ad, dd, LAM, lod, hid, delta_out)
    assert torch.equal(box_dual_pass_composed(Jd, ad, dd, LAM, lod, hid), out)
    _compare(out, delta_out, K, n, ref, bound, "composition")


def test_box_dual_pass_refuses_bad_arguments():
    from multigrad_amd.ops.box_dual import box_dual_pass
    J = torch.zeros(3, 8, device=DEV)
    a = torch.zeros(3, dtype=F64, device=DEV)
    vec = torch.ones(8, device=DEV)
    box_dual_pass(J, a, vec, 1.0, -vec, vec)
    bad = [
        (torch.zeros(0, 8, device=DEV), torch.zeros(0, dtype=F64, device=DEV), vec, -vec, vec, None),
        (torch.zeros(8, 3, device=DEV).T, a, vec, -vec, vec, None),       # column stride
        (J, a.float(), vec, -vec, vec, None),                             # a not float64
        (J, a[:2], vec, -vec, vec, None),
        (J, a, vec[:7], -vec, vec, None),
        (J, a, vec, -vec.cpu(), vec, None),                               # another device
        (J, a, vec, -vec, torch.ones(16, device=DEV)[::2], None),         # not contiguous
        (J, a, vec, -vec, vec, torch.zeros(7, device=DEV)),
        (J, a, vec, -vec, vec, torch.zeros(8, dtype=torch.int32, device=DEV)),
    ]
    for Jb, ab, db, lob, hib, out in bad:
        with pytest.raises(ValueError):
            box_dual_pass(Jb, ab, db, 1.0, lob, hib, out)
    with pytest.raises(RuntimeError):     # the extension itself takes float32 and K <= 10
        from multigrad_amd.ops import ext
        ext().box_dual_pass(torch.zeros(11, 8, device=DEV), torch.zeros(11, dtype=F64, device=DEV),
                            vec, 1.0, -vec, vec, None)


# ---------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _population():
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    data = make_population_data(2000, 54_000, seed=3, device=DEV)
    model = PopulationSMFModel(aux_data=data)
    model.set_target_from_truth()
    return model, data


def _box(data, a_range, s_range):
    """Bounds ``(ndim, 2)``: the ``a`` (even) and ``log10 sigma`` (odd) parameters."""
    b = torch.empty(data["guess"].numel(), 2, dtype=F64)
    b[0::2, 0], b[0::2, 1] = a_range
    b[1::2, 0], b[1::2, 1] = s_range
    return b


def test_population_fit_in_wide_bounds_beats_adam():
    """2 000 parameters, 54 000 halos, a box far outside the truth and a cap of 0.5 per step:
    the fit succeeds, stays inside, and ends at or below 200 Adam steps from the same guess
    (the yardstick of test_gauss_newton_dual_gpu.py)."""
    model, data = _population()
    guess = data["guess"]
    bounds = _box(data, (-6.0, 2.0), (-3.0, 1.0))
    res = model.run_gauss_newton_box(guess, param_bounds=bounds, max_step=0.5)
    traj = model.run_adam(guess, nsteps=200, learning_rate=0.01)
    adam = float(model.calc_loss_from_params(traj[-1]))
    print(f"box: fun={res.fun:.3e} nit={res.nit} njev={res.njev} nfev={res.nfev} "
          f"passes={res.inner_passes} unconverged={res.inner_unconverged} ({res.message}); "
          f"adam 200 steps: {adam:.3e}")
    assert res.success, res.message
    assert res.solver == "dual-box" and res.jac_mode == "native"
    lo, hi = bounds[:, 0].to(DEV, res.x.dtype), bounds[:, 1].to(DEV, res.x.dtype)
    assert bool(((res.x >= lo) & (res.x <= hi)).all())
    assert res.fun <= adam
    assert res.x.is_cuda and res.active.is_cuda and res.active.dtype == torch.int8
    K = data["bins"].nb
    assert max(res.host_copy_sizes) == K * K + K + 2 < guess.numel()


def test_population_fit_with_active_bounds_matches_lbfgsb():
    """Bounds that cut off some of the true values: some parameters end on a bound, the fit
    stops on the projected gradient or on ftol, and its loss is not above the device
    L-BFGS-B's on the same box by more than MARGIN."""
    model, data = _population()
    guess, truth = data["guess"], data["truth"]
    ftol, gtol = 2.2e-9, 1e-8
    a_med, s_med = float(truth[0::2].median()), float(truth[1::2].median())
    bounds = _box(data, (a_med - 1.0, a_med), (s_med, s_med + 1.0))
    res = model.run_gauss_newton_box(guess, param_bounds=bounds, max_step=0.5, ftol=ftol, gtol=gtol)
    ref = model.run_bfgs(guess, method="device", param_bounds=bounds)
    lo, hi = bounds[:, 0].to(DEV, res.x.dtype), bounds[:, 1].to(DEV, res.x.dtype)
    pg = float(torch.clamp(-res.jac, min=lo - res.x, max=hi - res.x).abs().max())
    margin = max(MARGIN, ftol * max(res.fun, 1.0))
    print(f"box: fun={res.fun:.6e} nit={res.nit} njev={res.njev} nfev={res.nfev} "
          f"passes={res.inner_passes} unconverged={res.inner_unconverged} "
          f"active={int((res.active != 0).sum())} pg={pg:.2e} ({res.message}); "
          f"L-BFGS-B: fun={float(ref.fun):.6e} nit={ref.nit}; difference "
          f"{res.fun - float(ref.fun):.3e}, margin {margin:.3e}")
    assert bool(((res.x >= lo) & (res.x <= hi)).all())
    assert int((res.active != 0).sum()) > 0
    assert res.success and (pg <= gtol or "ftol" in res.message), res.message
    assert res.fun <= float(ref.fun) + margin


def test_population_fit_above_the_fused_limit():
    """12 bins: K = 12 takes the float64 torch path, and the inner solve has to meet its
    1e-9 stop rule there as well.  The same yardstick as at 10 bins."""
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.ops.box_dual import MAX_FUSED_ROWS
    data = make_population_data(2000, 54_000, seed=3, device=DEV, nbins=12)
    assert data["bins"].nb == 12 > MAX_FUSED_ROWS
    model = PopulationSMFModel(aux_data=data)
    model.set_target_from_truth()
    guess = data["guess"]
    bounds = _box(data, (-6.0, 2.0), (-3.0, 1.0))
    res = model.run_gauss_newton_box(guess, param_bounds=bounds, max_step=0.5)
    traj = model.run_adam(guess, nsteps=200, learning_rate=0.01)
    adam = float(model.calc_loss_from_params(traj[-1]))
    converged = sum(1 for t in res.trials if t[2])
    print(f"K=12 box: fun={res.fun:.3e} nit={res.nit} njev={res.njev} nfev={res.nfev} "
          f"passes={res.inner_passes} unconverged={res.inner_unconverged} of {len(res.trials)} "
          f"({res.message}); adam 200 steps: {adam:.3e}")
    assert res.success, res.message
    assert converged > res.inner_unconverged       # the solves converge as a rule
    assert res.fun <= adam


# Three times the difference observed on the MI355X, box minus L-BFGS-B.  Observed: -5.9e-6 (the
# box fit ended at 1.9e-8, the device L-BFGS-B at 5.9e-6 when it stopped), so nothing is added
# and the floor ftol * max(loss, 1) = 2.2e-9 alone applies.
MARGIN = 0.0
