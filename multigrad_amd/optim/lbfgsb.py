"""Device L-BFGS-B: box-constrained L-BFGS on (optionally sharded) device vectors.

The reference hands its bounds to scipy's L-BFGS-B (``multigrad/bfgs.py:83-86``).  At
1e6-1e8 parameters that optimizer has to live on the GPUs, so this is L-BFGS-B itself
(Byrd, Lu, Nocedal & Zhu 1995, with the projected subspace step of Morales & Nocedal
2011, as in scipy's L-BFGS-B 3.0) in an SPMD form:

* **Generalized Cauchy point.**  The first local minimiser of the quadratic model
  ``m(x) = f + g'(x-x_k) + (x-x_k)'B(x-x_k)/2`` (compact form ``B = theta I - W M W'``,
  ``W = [Y, theta S]``) along the projected gradient path ``P(x - t g)``.  The path
  has one breakpoint per coordinate; each rank sends the ``K`` smallest of its own (with
  the gradient entry and the ``2m`` row of ``W``), so every rank holds the ``K`` globally
  smallest, sorted, and runs the same sequential segment scan on the host -- identical
  decisions everywhere without broadcasts.  The Cauchy point is then ``P(x - t* g)``, one
  elementwise pass on the device.  (If the minimiser lies beyond the ``K``-th breakpoint,
  ``K`` grows and the scan repeats.)
* **Subspace minimisation** over the free variables by the direct primal method.  The
  ``2m x 2m`` Gram matrix of ``W`` over the free rows is the full Gram matrix (kept from
  the history inner products) minus the rows of the active set, which are gathered; the
  step is projected onto the box and falls back to the feasible truncation if the
  projected step is not a descent direction.
* **Line search** along ``d = xbar - x`` (strong Wolfe, cubic interpolation, step <= 1 so
  the iterate stays feasible), on loss values and directional derivatives that are
  all-reduced, i.e. bitwise identical on every rank.
* **Host traffic.**  Two device->host copies per iteration besides the function
  evaluations: (A) the new pair's inner products with the history together with every
  Cauchy-point input, (B) the subspace inner products; the first evaluation of the line
  search also carries the directional derivative at the start point.

One iteration is these phases, a function each: copy A with the projected gradient
(``_measure``), the Cauchy point (``_generalized_cauchy`` around ``_cauchy_point``), copy B
with the subspace step (``_subspace_step``), the search (``_search``), its retry along the
truncated step (``_truncated``) and the update (``_update``).  The pair ring, the search
itself and the frame of the driver are shared with the unbounded L-BFGS
(:mod:`multigrad_amd.optim._quasi_newton`).

Termination as scipy: ``max|P(x-g)-x| <= pgtol`` or ``(f_k-f_{k+1})/max(|f_k|,|f_{k+1}|,1)
<= factr * eps`` or ``maxiter``.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import scipy.linalg
import scipy.optimize
import torch

from ..ops.lbfgs import MultiDot
from ._quasi_newton import HostCollectives, PairRing, Run, best_decrease, driver, strong_wolfe
from ._reduce import DeviceReducer
from .lbfgs import GenericObjective

__all__ = ["lbfgsb_minimize", "run_lbfgsb_device", "BoxObjective"]

_EPS = np.finfo(np.float64).eps
_B_CAP_MULTI = 1 << 16  # breakpoints per rank and Cauchy-point batch on several ranks


class BoxObjective(GenericObjective):
    """Replicated objective ``loss_and_grad_fn(x) -> (loss, grad)`` in the parameters
    themselves (no transform), for :func:`lbfgsb_minimize`."""

    def __init__(self, loss_and_grad_fn, x0: torch.Tensor, comm=None, **fn_kwargs):
        if "bounds" in fn_kwargs:
            raise TypeError("BoxObjective takes no bounds=: the box is lbfgsb_minimize's lo, hi")
        super().__init__(loss_and_grad_fn, x0, comm=comm, **fn_kwargs)


def _box(lo, hi, n, device):
    lo = torch.full((n,), -math.inf, device=device) if lo is None else \
        torch.as_tensor(lo, dtype=torch.float32, device=device).reshape(-1).clone()
    hi = torch.full((n,), math.inf, device=device) if hi is None else \
        torch.as_tensor(hi, dtype=torch.float32, device=device).reshape(-1).clone()
    return lo.contiguous(), hi.contiguous()


def _clip(v, lo, hi):
    return torch.minimum(torch.maximum(v, lo), hi)


def _compact(ring: PairRing):
    """``(idx, M, WWt)`` for the accepted pairs: ``M`` (2k x 2k) and the full Gram
    matrix ``W W'`` of ``W = [Y, theta S]`` (rows in ``idx`` order)."""
    idx = np.asarray(ring.order, dtype=np.int64)
    k = idx.size
    if k == 0:
        return idx, np.zeros((0, 0)), np.zeros((0, 0))
    th = ring.theta
    sy = ring.SY[np.ix_(idx, idx)]
    D = np.diag(np.diag(sy))
    Lm = np.tril(sy, -1)
    ss = ring.SS[np.ix_(idx, idx)]
    K = np.block([[-D, Lm.T], [Lm, th * ss]])
    M = np.linalg.inv(K)
    yy = ring.YY[np.ix_(idx, idx)]
    ys = sy.T  # y_i . s_j
    WWt = np.block([[yy, th * ys], [th * ys.T, th * th * ss]])
    return idx, M, WWt


def _rows(ring: PairRing, idx):
    """Row indices of ``W = [Y_idx, S_idx]`` in HS and the theta factor per row."""
    rows = np.concatenate([ring.R + idx, idx]).astype(np.int64)
    fac = np.concatenate([np.ones(idx.size), np.full(idx.size, ring.theta)])
    return rows, fac


class _Run(Run):
    """A run of L-BFGS-B: the box, the slot of the pair that waits to be measured and the
    start slope of the line search under way."""

    def __init__(self, obj, red, lo, hi, m: int, K: Optional[int]):
        n, dev = obj.n_local, obj.device
        super().__init__(obj, red, PairRing(m, n, dev), "L-BFGS-B")
        self.lo, self.hi = _box(lo, hi, n, dev)
        self.lo64, self.hi64 = self.lo.double(), self.hi.double()
        self.x = _clip(obj.x0().contiguous(), self.lo, self.hi)
        self.f, self.g = self.trial.initial(self.x)
        self.dot = MultiDot(2 * self.ring.R, n, dev)
        self.K = K
        self.pending = None  # slot of a written, not yet measured pair
        self.d0 = None       # slope at step 0 of the latest line search

    def accept_pending(self, dots: np.ndarray) -> None:
        self.ring.accept(self.pending, dots)
        self.pending = None


class _Model(NamedTuple):
    """The quadratic model at the Cauchy point: the compact matrices, the rows of W in the
    ring, ``c = W'(x^cp - x)`` and the Cauchy point."""
    M: np.ndarray
    WWt: np.ndarray
    rows: np.ndarray
    fac: np.ndarray
    cvec: np.ndarray
    xcp: torch.Tensor


def _measure(st: _Run):
    """Copy A: the pending pair's inner products with the history (the pair is accepted or
    dropped here), the projected-gradient norm and every Cauchy-point input, in one
    reduction and one device->host copy.  Returns ``(d.d, HS.d, max|P(x-g)-x|, breakpoints,
    number of finite local breakpoints)`` for the projected steepest-descent direction d."""
    x, g, lo, hi, ring = st.x, st.g, st.lo, st.hi, st.ring
    R = ring.R
    t = torch.where(g < 0, (x - hi) / g, torch.where(g > 0, (x - lo) / g,
                                                      torch.full_like(g, math.inf)))
    t = torch.where(torch.isnan(t), torch.full_like(t, math.inf), t)
    free_path = t > 0
    d = torch.where(free_path, -g, torch.zeros_like(g))
    xd = x.double()
    pg = (_clip(xd - g.double(), st.lo64, st.hi64) - xd).abs()
    vecs = [d] if st.pending is None else [ring.s(st.pending), ring.y(st.pending), d]
    dots_dev = st.dot(ring.HS, 2 * R, vecs)
    tc = torch.where(free_path & torch.isfinite(t), t, torch.full_like(t, math.inf))
    pg_l = pg.max().double() if g.numel() else torch.zeros((), dtype=torch.float64,
                                                           device=g.device)
    # one reduction and one copy: [d.d, HS.vecs (summed), max|pg| (max), #finite (local)]
    packA = st.red.reduce(sums=[(d.double() * d.double()).sum(), dots_dev],
                          maxes=[pg_l], local=[torch.isfinite(tc).sum()])
    dots_np = packA[1:1 + 2 * R * len(vecs)].reshape(2 * R, len(vecs))
    if st.pending is not None:
        st.accept_pending(dots_np[:, :2])
    return packA[0], dots_np[:, -1], float(packA[-2]), tc, int(packA[-1])


def _generalized_cauchy(st: _Run, dd, Wd, tc, nfin) -> _Model:
    """The Cauchy point ``P(x - t* g)`` of the compact model over the accepted pairs."""
    ring = st.ring
    idx, M, WWt = _compact(ring)
    rows, fac = _rows(ring, idx)
    tstar, cvec = _cauchy_point(dd, Wd[rows] * fac, M, ring.theta, tc, nfin, st.g, ring.HS,
                                rows, fac, st.red, st.K)
    return _Model(M, WWt, rows, fac, cvec, _clip(st.x - tstar * st.g, st.lo, st.hi))


def _subspace_step(st: _Run, mdl: _Model) -> torch.Tensor:
    """Copy B: the minimiser of the model over the variables free at the Cauchy point
    (direct primal method), as a step ``du`` from the Cauchy point; its inner products come
    back in one reduction and one device->host copy."""
    x, g, ring, red = st.x, st.g, st.ring, st.red
    M, WWt, rows, fac, cvec, xcp = mdl
    R, th, dev = ring.R, ring.theta, x.device
    free = (xcp > st.lo) & (xcp < st.hi)
    kk2 = rows.size // 2
    if kk2:
        coef = np.zeros(2 * R)
        coef[rows] = (M @ cvec) * fac
        r = g + th * (xcp - x) - ring.lincomb(coef, 0.0, None, torch.empty_like(x))
    else:
        r = g + th * (xcp - x)
    rF = torch.where(free, r, torch.zeros_like(r))
    WtZr = st.dot(ring.HS, 2 * R, [rF])[:, 0]
    if kk2:
        act = torch.nonzero(~free).reshape(-1)  # a host sync: only where it is used
        rows_d = torch.as_tensor(rows, device=dev)
        GA = _gram(ring.HS[rows_d[:, None], act[None, :]].double())
    else:
        GA = torch.zeros((0, 0), dtype=torch.float64, device=dev)
    redB = red.reduce(sums=[WtZr, GA])
    if kk2:
        GA_np = redB[2 * R:].reshape(kk2 * 2, kk2 * 2)
        fw = fac[:, None] * fac[None, :]
        GF = WWt - GA_np * fw               # Gram of W over the free rows
        v = M @ (redB[:2 * R][rows] * fac)
        N = np.eye(2 * kk2) - (M @ GF) / th
        v = scipy.linalg.solve(N, v)
        coef = np.zeros(2 * R)
        coef[rows] = v * fac
        zwv = ring.lincomb(coef, 0.0, None, torch.empty_like(x))
        du = -(rF / th) - (zwv / (th * th))
    else:
        du = -(rF / th)
    return torch.where(free, du, torch.zeros_like(du))


def _search(st: _Run, dirn: torch.Tensor, a1: float, c1: float, c2: float, maxls: int):
    """Strong-Wolfe step on (0, 1] along ``dirn`` (the iterate stays feasible), or None.  The
    directional derivatives are summed over the ranks with the (global) loss: one copy per
    trial point, and the first one also carries the slope at the start point (``st.d0``)."""
    g = st.g

    def sums(ga, first):
        parts = [(ga.double() * dirn.double()).sum()]
        if first:
            parts.append((g.double() * dirn.double()).sum())
        return parts

    def start_slope():
        st.d0 = float(st.trial.last[1])
        return st.d0

    st.trial.start(st.x, dirn, sums)
    return strong_wolfe(st.trial, st.f, start_slope, a1, c1, c2, maxls, amax=1.0)


def _truncated(st: _Run, xcp: torch.Tensor, du: torch.Tensor) -> torch.Tensor:
    """The direction to the feasible truncation of the subspace step (for when the
    projected step is not a descent direction)."""
    ratio = torch.where(du > 0, (st.hi - xcp) / du, torch.where(du < 0, (st.lo - xcp) / du,
                                                               torch.full_like(du, math.inf)))
    rmin_l = -ratio.min().double() if ratio.numel() else \
        torch.full((), -math.inf, dtype=torch.float64, device=du.device)
    rmin = -float(st.red.reduce(maxes=[rmin_l])[0])
    return xcp + min(1.0, rmin) * du - st.x


def _update(st: _Run, dirn: torch.Tensor, best: float) -> None:
    """Move to the accepted trial point; the new pair goes into the spare slot and waits
    there for copy A of the next iteration."""
    ring = st.ring
    f_new, g_new, _ = st.trial.cache[best]
    q = ring.spare()
    torch.mul(dirn, best, out=ring.s(q))
    torch.sub(g_new, st.g, out=ring.y(q))
    st.x.add_(ring.s(q))
    st.x.copy_(_clip(st.x, st.lo, st.hi))
    st.pending = q
    st.f, st.g = f_new, g_new


@driver(single_thread_blas=True)
def lbfgsb_minimize(obj, lo=None, hi=None, maxiter: int = 100, m: int = 10,
                    factr: float = 1e7, pgtol: float = 1e-5, maxls: int = 20,
                    c1: float = 1e-4, c2: float = 0.9, K: Optional[int] = None,
                    callback=None, gtol: Optional[float] = None,
                    ftol: Optional[float] = None,
                    hess_inv: bool = True) -> scipy.optimize.OptimizeResult:
    """Minimise ``obj`` subject to ``lo <= x <= hi`` (local slices of the optimizer's
    vector, +-inf allowed).  ``obj`` as for :func:`multigrad_amd.optim.lbfgs.lbfgs_minimize`
    (``x0()``, ``__call__(x) -> (f, g)``, optional ``device_call``, ``full(x)``, ``comm``,
    ``sharded``).  ``gtol`` / ``ftol`` are accepted as aliases of ``pgtol`` /
    ``factr * eps`` (the unbounded driver's names).

    ``hess_inv=True`` adds ``hess_inv``, a
    :class:`~multigrad_amd.optim.invhess.DeviceLbfgsInvHessProduct` over every pair accepted
    when the run returns (a pair still waiting to be measured goes through the acceptance
    rule first: one more collective dot block); as in scipy the bounds do not enter it.  It
    keeps the history ring alive (a reference, no copy: ``2 (m + 1)`` fp32 vectors, 0.9 GB at
    1e7 parameters and ``m = 10``); ``hess_inv=False`` frees it on return."""
    if gtol is not None:
        pgtol = gtol
    if ftol is not None:
        factr = ftol / _EPS
    ftol = factr * _EPS
    if hess_inv:
        from .invhess import check_hess_inv_objective
        check_hess_inv_objective(obj)
    red = DeviceReducer(obj.comm, obj.sharded, obj.device)  # collective (may connect peer memory)
    st = _Run(obj, red, lo, hi, m, K)
    ring = st.ring
    # the first Cauchy-point batch all-gathers (1 + B0) x (2 + 2m) fp64 records per rank:
    # connect that context now; the geometric growth to larger batches (rare: the Cauchy
    # point usually lies among the first few thousand breakpoints) connects its larger
    # context on demand, collectively (every rank reaches the same batch together) -- about
    # 1.2 MB per rank at m = 10 instead of 11.5 MB reserved for a 2^16 batch up front
    b0 = int(K) if K is not None else min(1 << 14, _B_CAP_MULTI)
    red.reserve_gather((1 + b0) * (2 + 2 * m) * 8)
    host = HostCollectives(obj.comm)
    for k in range(maxiter + 1):
        dd, Wd, pgmax, tc, nfin = _measure(st)
        if k > 0 and callback is not None:
            host.callback(callback, obj, st.x)
        if pgmax <= pgtol:
            st.converged_gradient()
            break
        if k == maxiter:
            break
        mdl = _generalized_cauchy(st, dd, Wd, tc, nfin)
        du = _subspace_step(st, mdl)
        dirn = _clip(mdl.xcp + du, st.lo, st.hi) - st.x
        a1 = 1.0
        if k == 0 or not ring.order:
            dnorm2 = float(red.reduce(sums=[(dirn.double() ** 2).sum()])[0])
            a1 = min(1.0, 1.0 / math.sqrt(max(dnorm2, 1e-300)))
        best = _search(st, dirn, a1, c1, c2, maxls)
        if st.d0 >= 0:
            # the projected subspace step is not a descent direction: truncate instead
            dirn = _truncated(st, mdl.xcp, du)
            best = _search(st, dirn, a1, c1, c2, maxls)
        best = best_decrease(best, st.trial.cache, st.f)
        if best is None:
            st.no_step()
            break
        f_old = st.f
        _update(st, dirn, best)
        st.nit = k + 1
        if st.hooks.active:
            st.hooks(k, st.f, None, (lambda: st.x) if not obj.sharded else None,
                     nfev=st.trial.nfev)
        if st.converged_decrease(f_old, ftol):
            if callback is not None:
                host.callback(callback, obj, st.x)
            break
    host_calls = host.count
    if hess_inv and st.pending is not None:
        # the last pair is measured at the top of the next iteration, which never came
        pk = red.reduce(sums=[st.dot(ring.HS, 2 * ring.R, [ring.s(st.pending), ring.y(st.pending)])])
        st.accept_pending(pk.reshape(2 * ring.R, 2))
    return st.result(host_calls, hess_inv, st.dot)


def _cauchy_point(dd, p0, M, theta, tc, nfin, g, HS, rows, fac, red, K):
    """Generalized Cauchy point ``t*`` and ``c = W'(x^cp - x)`` (Byrd et al. 1995,
    algorithm CP), over the breakpoints in increasing order, in batches.

    ``tc``: this rank's breakpoints (+inf where none), ``nfin`` of them finite.  Each batch
    takes the next ``K`` of every rank (sorted on the device); across ranks the union is
    exact up to the smallest "largest gathered" breakpoint of the ranks that have more,
    and only that prefix is scanned (the rest waits for the next batch).  The scan of a
    batch is vectorised: the running ``p``, ``c``, ``f'`` and ``f''`` of the sequential
    algorithm are prefix sums over the sorted breakpoints (``_scan_batch``)."""
    dev = tc.device
    k2 = p0.size
    Mt = torch.as_tensor(M, dtype=torch.float64, device=dev)
    st = {"p": torch.as_tensor(p0, dtype=torch.float64, device=dev),
          "c": torch.zeros(k2, dtype=torch.float64, device=dev),
          "fp": -dd, "fpp": theta * dd - (float(p0 @ M @ p0) if k2 else 0.0), "told": 0.0}
    order = torch.argsort(tc)
    rows_t = torch.as_tensor(rows, dtype=torch.int64, device=dev)
    fac_t = torch.as_tensor(fac, dtype=torch.float64, device=dev)
    comm = None if red is None else red.comm
    multi = comm is not None and comm.size > 1
    # batch sizes: K if given, else geometric from 2^14 (the Cauchy point usually lies among
    # the first few thousand breakpoints, and a scan costs O(2k x batch) in fp64) up to
    # 2^16 per rank (several ranks: one all-gather per batch) or 2^20 (one rank)
    B_cap = int(K) if K is not None else (_B_CAP_MULTI if multi else 1 << 20)
    B = int(K) if K is not None else min(1 << 14, B_cap)
    ptr = 0
    while True:
        sel = order[ptr:ptr + B]
        tb = tc[sel].double()
        gb = g[sel].double()
        Wb = (HS[rows_t[:, None], sel[None, :]].double() * fac_t[:, None]) if k2 else \
            torch.zeros((0, sel.numel()), dtype=torch.float64, device=dev)
        left = nfin - ptr  # this rank's finite breakpoints not yet scanned
        if multi:
            rec = torch.full((B, 2 + k2), math.inf, dtype=torch.float64, device=dev)
            nb = sel.numel()
            rec[:nb, 0], rec[:nb, 1], rec[:nb, 2:] = tb, gb, Wb.T
            rec[nb:, 1:] = 0.0
            hdr = torch.tensor([[float(left)] + [0.0] * (1 + k2)], dtype=torch.float64, device=dev)
            mine = torch.cat([hdr, rec]).contiguous()
            allr = red.all_gather(mine)   # peer memory / RCCL: [W, 1 + B, 2 + k2]
            # one copy: every rank's count of unscanned breakpoints and its B-th breakpoint
            hdr = torch.stack([allr[:, 0, 0], allr[:, B, 0]], 1).cpu().numpy()
            lefts = hdr[:, 0]
            t_cut = math.inf
            for r in range(comm.size):
                if lefts[r] > B:
                    t_cut = min(t_cut, float(hdr[r, 1]))
            recs = allr[:, 1:].reshape(-1, 2 + k2)
            keep = recs[:, 0] <= t_cut
            recs = recs[keep & torch.isfinite(recs[:, 0])]
            recs = recs[torch.argsort(recs[:, 0], stable=True)]
            tb, gb, Wb = recs[:, 0], recs[:, 1], recs[:, 2:].T.contiguous()
            mine_used = int(((rec[:, 0] <= t_cut) & torch.isfinite(rec[:, 0])).sum().item())
            more = bool((lefts > B).any())
        else:
            fin = torch.isfinite(tb)
            tb, gb, Wb = tb[fin], gb[fin], Wb[:, fin]
            mine_used = sel.numel()
            more = left > B
        found, tstar, c = _scan_batch(st, tb, gb, Wb, Mt, theta)
        if found:
            return tstar, c
        ptr += mine_used
        B = min(B * 8, B_cap)
        if not more:
            dtmin = -st["fp"] / st["fpp"] if st["fpp"] > 0 else 0.0
            dtmin = max(dtmin, 0.0)
            c = st["c"] + dtmin * st["p"]
            return st["told"] + dtmin, c.cpu().numpy()


def _rowcumsum(X: torch.Tensor) -> torch.Tensor:
    """Inclusive cumulative sum along the last dim of a (R x N) tensor as ONE device-wide
    scan of the flattened data minus each row's start offset.  torch's per-row scan runs
    one block per row, so with R = 2k ~ 20 rows it used ~20 blocks of the GPU (565 us per
    call at N = 2^20, against ~0.1 ms here); fp64, so the offsets cost no accuracy."""
    if X.dim() == 1 or X.shape[0] == 1:
        return torch.cumsum(X, -1)
    c = torch.cumsum(X.reshape(-1), 0).reshape(X.shape)
    off = torch.cat([torch.zeros(1, dtype=c.dtype, device=c.device), c[:-1, -1]])
    return c - off[:, None]


def _gram(A: torch.Tensor, chunk: int = 8192) -> torch.Tensor:
    """``A @ A.T`` for a short, very wide fp64 ``A`` (2k x K): a batched product over column
    chunks, summed.  A single GEMM with M = N = 2k and K ~ 1e6-1e7 runs a 128x128 tile
    with no split of K (5.4 ms measured at K ~ 5e6)."""
    R, K = A.shape
    if K <= 4 * chunk:
        return A @ A.T
    nc = -(-K // chunk)
    Ap = torch.zeros((R, nc * chunk), dtype=A.dtype, device=A.device)
    Ap[:, :K] = A
    X = Ap.view(R, nc, chunk).permute(1, 0, 2)          # (nc, R, chunk), strided view
    return torch.bmm(X, X.transpose(1, 2)).sum(0)


def _scan_batch(st, t, g, W, M, theta):
    """One batch of the Cauchy-point scan (sorted breakpoints ``t``, gradient entries
    ``g``, columns ``W`` (2k x N) = rows of ``[Y, theta S]`` at the breakpoints).  Returns
    ``(True, t*, c)`` when the minimiser lies in a segment of this batch, else advances
    ``st`` past it and returns ``(False, None, None)``.  The 2k-vectors are kept as
    (2k x N) so every prefix sum runs along the contiguous dimension."""
    N = t.numel()
    if N == 0:
        return False, None, None
    told0 = st["told"]
    prev = torch.cat([torch.full((1,), told0, dtype=torch.float64, device=t.device), t[:-1]])
    dt = t - prev
    gw = W * g[None, :]
    P = st["p"][:, None] + _rowcumsum(gw) - gw               # p before breakpoint i
    Mw = M @ W                                               # M w_i (M symmetric)
    wMp = (Mw * P).sum(0)
    wMw = (Mw * W).sum(0)
    dfpp = -theta * g * g - 2 * g * wMp - g * g * wMw
    fpp_b = st["fpp"] + torch.cumsum(dfpp, 0) - dfpp          # f'' at the start of segment i
    Cp = st["c"][:, None] + _rowcumsum(P * dt[None, :])     # c after breakpoint i
    wMc = (Mw * Cp).sum(0)
    dfp = dt * fpp_b + g * g - theta * t * g * g - g * wMc
    fp_b = st["fp"] + torch.cumsum(dfp, 0) - dfp              # f' at the start of segment i
    dtmin = torch.where(fpp_b > 0, -fp_b / fpp_b, torch.full_like(fp_b, math.inf))
    stop = dtmin < dt
    # ONE host copy: the first stop index (or -1), the end-of-batch state, and -- formed on
    # the device at that index, used only when it is >= 0 -- t* and c (three copies fewer
    # per Cauchy point than reading t[j-1], dtmin[j] and c back one by one)
    jt = torch.argmax(stop.to(torch.int8))
    first = torch.where(stop.any(), jt.to(torch.float64),
                        torch.full((), -1.0, dtype=torch.float64, device=t.device))
    told_t = torch.where(jt > 0, t[(jt - 1).clamp(min=0)],
                         torch.full((), told0, dtype=torch.float64, device=t.device))
    dtm_t = dtmin[jt].clamp(min=0.0)
    c_prev = torch.where(jt > 0, Cp[:, (jt - 1).clamp(min=0)], st["c"])
    c_t = c_prev + dtm_t * P[:, jt]
    tail = torch.cat([torch.stack([first, fp_b[-1] + dfp[-1], fpp_b[-1] + dfpp[-1], t[-1],
                                   told_t + dtm_t]), c_t]).cpu().numpy()
    j = int(tail[0])
    if j >= 0:
        return True, float(tail[4]), tail[5:]
    st["p"] = P[:, -1] + gw[:, -1]
    st["c"] = Cp[:, -1]
    st["fp"], st["fpp"], st["told"] = float(tail[1]), float(tail[2]), float(tail[3])
    return False, None, None


def run_lbfgsb_device(loss_and_grad_fn, params, maxsteps: int = 100, param_bounds=None,
                      randkey=None, comm=None, history: int = 10, prior=None,
                      prior_weight: float = 1.0, **kw):
    """Device L-BFGS-B for a generic ``loss_and_grad_fn(params[, randkey])`` (replicated).
    ``hess_inv=True`` (default) returns the inverse-Hessian operator as ``res.hess_inv``
    (it holds the history ring, see :func:`lbfgsb_minimize`).  ``prior`` and ``prior_weight``
    as for :func:`~multigrad_amd.optim.lbfgs.run_lbfgs_device`: the box-constrained minimum of
    ``loss + prior_weight * prior.penalty(x)``."""
    from ..utils.random import init_randkey
    from ..utils.tensors import as_param_tensor
    from .prior import PriorObjective, check_prior, with_penalty
    x0 = as_param_tensor(params)
    check_prior(prior, x0.numel())
    lo, hi = bounds_arrays(param_bounds, x0.numel())
    fkw = {} if randkey is None else {"randkey": init_randkey(randkey)}
    obj = BoxObjective(loss_and_grad_fn, x0, comm=comm, **fkw)
    if prior is not None:
        obj = PriorObjective(obj, prior, prior_weight)
    return with_penalty(lbfgsb_minimize(obj, lo, hi, maxiter=maxsteps, m=history, **kw), prior)


def bounds_arrays(param_bounds, n: int):
    """``(lo, hi)`` float arrays (+-inf for open sides) from a reference-style spec
    ``(ndim, 2)`` with ``None`` entries, or ``(None, None)``."""
    if param_bounds is None:
        return None, None
    if isinstance(param_bounds, (np.ndarray, torch.Tensor)):
        b = np.asarray(param_bounds.detach().cpu() if isinstance(param_bounds, torch.Tensor)
                       else param_bounds, dtype=np.float64).reshape(n, 2)
        b = np.where(np.isnan(b), np.array([-np.inf, np.inf]), b)
        return b[:, 0].astype(np.float32), b[:, 1].astype(np.float32)
    lo = np.full(n, -np.inf)
    hi = np.full(n, np.inf)
    for i, b in enumerate(param_bounds):
        if b is None:
            continue
        a, c = b
        if a is not None:
            lo[i] = float(a)
        if c is not None:
            hi[i] = float(c)
    return lo.astype(np.float32), hi.astype(np.float32)
