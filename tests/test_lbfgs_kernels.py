"""``multi_dot`` and ``lincomb`` (csrc/lbfgs.hip behind ops/lbfgs.py) against plain float64 /
int64 references with derived bounds, and the unbounded device L-BFGS run to its gradient
tolerance.  The ``check_*`` bodies take a ``device``: here they run on the torch fallbacks of
ops/lbfgs.py, test_lbfgs_kernels_gpu.py runs them again on the HIP kernels.

Inputs.  ``A`` (and ``H``) is a view ``big[1:, c_off:c_off + cols]`` of a larger float32
buffer with ``cols >= n``; every right-hand vector, ``x`` and ``y`` is a slice of a longer
vector.  Everything an op must not read is NaN: the row before and the rows from ``nrows``
on, the columns outside ``[0, n)``, vector elements from ``n`` on, the coefficients from
``nrows`` on, the workspace and ``out`` (refilled before every call).  Results must be
finite and ``out`` past ``nrows * nc`` must stay NaN.  Layouts of ``multi_dot``:

  a  all bases 16-byte aligned, ``lda % 4 == 0``, ``n % 4 == 0``: float4 only
  b  as a with ``n % 4 == 3`` and ``lda = n + 5`` rounded up to 4: float4 body, scalar tail
  c  ``lda == n`` odd: scalar
  d  as b for any n, but the last right-hand vector starts one float late: scalar
  e  ``A`` starts one float late in an ``lda % 4 == 0`` buffer: scalar

Exact checks.  With integers of {-3..3} every product and every float32 lane sum is exact
(the longest lane chain here has under 100 terms: |sum| < 900 << 2^24) and so are the
float64 reductions: the result equals the int64 product bit for bit at any size.

Bound of ``multi_dot``.  A lane forms its sum as one float32 ``fmaf`` chain t <- fl(a b + t),
one rounding per term, so a chain of L terms errs by at most gamma_L sum |a_j b_j| with
gamma_L = L u / (1 - L u), u = 2^-24 (Higham, Accuracy and Stability, 3.1); the lane sums are
then added in float64 (wave shuffles, LDS, the reduce kernel: a few dozen roundings of
2^-53), for which 2^-40 sum |a_j b_j| is ample:

    |out - ref| <= (gamma_L + 2^-40) sum_j |a_j b_j|.

L is the longest chain of any lane.  A launch has ``bx = min(ceil(chunks / tpb), cap)``
column blocks of ``tpb`` lanes, a lane takes every ``bx * tpb``-th chunk of ``VW`` elements
(float4: VW = 4, chunks = n >> 2, and the lanes of the first block take one tail element
more; scalar: VW = 1, chunks = n; tpb = 64 lanes from 4 rows on, where a wave owns its rows,
else 256).  The cap is the number of resident workgroups, which a test cannot see, but it is
at least the CU count, so with ``bx_min = min(ceil(chunks / tpb), CUs)``

    L <= VW ceil(chunks / (bx_min tpb)) + (1 if VW == 4 and n % 4 else 0).

The CPU fallback multiplies in float64: L = 0, the 2^-40 term alone.  The reference takes the
float64 products (exact: 48 bits) and sums them pairwise (numpy), error about 2^-48.

Bound of ``lincomb``.  Per element t_0 = fl(alpha x), t_{i+1} = fl(c_i h_i + t_i): one
rounding for alpha x, one per ``fmaf``, at most nrows + 1 on any term.  The bound takes
gamma_{nrows + 2}; the spare rounding leaves room for the compiler contracting the alpha x
product into the first step or not:

    |y - ref| <= gamma_{nrows + 2} (|alpha x_j| + sum_i |c_i H_ij|).

The sizes that exist only for the kernels' grid-stride loops (n = 600 003, 1 049 603,
4 195 331) run here at one row count each, enough to debug the check bodies without a GPU.
"""
import math

import numpy as np
import pytest
import torch

from multigrad_amd.ops.lbfgs import MultiDot, lincomb_, lincomb_cols_
from multigrad_amd.optim.lbfgs import run_lbfgs_device

CPU = torch.device("cpu")
U = 2.0 ** -24
NAN = float("nan")

# every dot_rpw branch and boundary (1-3 rows per thread; 2/4/6/8 rows per wave), 1/2/3/8 row
# groups, last groups with one real row (9, 17, 25, 33, 65) and 243 = 2 * 121 + 1 (m = 120)
ROWS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 23, 24, 25, 32, 33, 63, 64, 65, 243)
NCS = (1, 2, 3, 4)
EXACT_N = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1027, 1028)
BOUND_N = (1027, 1028, 65_539)
# a second trip of the grid-stride loop needs n > 4 * 2048 * 64 (>= 4 rows) or 4 * 2048 * 256
TWO_TRIPS = ((1_049_603, (4, 8, 23, 40)), (4_195_331, (1, 3)))
TWO_TRIPS_NCS = (1, 3, 4)
PATH = {"a": "float4", "b": "float4 + tail", "c": "scalar", "d": "scalar", "e": "scalar"}

LINCOMB_ROWS = (0, 1, 2, 22, 23, 242, 256)
LINCOMB_N = (1, 3, 4, 5, 255, 257, 1027, 1028, 600_003)  # 600 003 > 2048 * 256: second trip
LINCOMB_LAYOUTS = ("pad", "odd")


def _ru4(k):
    return (k + 3) // 4 * 4


def layout_fits(layout, n):
    return {"a": n % 4 == 0, "b": n % 4 == 3, "c": n % 2 == 1}.get(layout, True)


def _geometry(layout, n):
    """(row stride, first column, columns) of the view ``big[1:, c0:c0 + cols]``."""
    if layout == "a":
        return n + 8, 4, n + 4
    if layout in ("b", "d", "pad"):
        return _ru4(n + 5), 4, _ru4(n + 5) - 4
    if layout == "c":
        return n, 0, n
    if layout == "odd":
        return n | 1, 0, n | 1
    assert layout == "e"
    return _ru4(n + 5), 1, _ru4(n + 5) - 1


def _draw(t, kind, gen):
    return t.random_(-3, 4, generator=gen) if kind == "int" else t.normal_(generator=gen)


class Inputs:
    """``nrows`` rows of ``n`` values in a NaN-surrounded view (see the module docstring) and
    ``nvec`` vectors, each both 16-byte aligned and one float late.  The values depend on
    (kind, n, nrows) only, so every layout of a size shares one reference."""

    def __init__(self, device, layout, n, nrows, kind, nvec=4):
        self.key = (kind, n, nrows, nvec)
        self.n, self.nrows, self.kind = n, nrows, kind
        gen = torch.Generator().manual_seed(7919 * n + 31 * nrows + (kind == "int"))
        ld, c0, cols = _geometry(layout, n)
        big = torch.full((nrows + 2, ld), NAN, dtype=torch.float32)
        # drawn contiguous (the order of the draws must not follow the layout), kept on the host
        self.clean = _draw(torch.empty((nrows, n), dtype=torch.float32), kind, gen)
        big[1:1 + nrows, c0:c0 + n] = self.clean
        self.vecs = _draw(torch.empty((nvec, n), dtype=torch.float32), kind, gen)
        self.big = big.to(device) if device.type != "cpu" else big.clone()
        self.A = self.big[1:, c0:c0 + cols]
        self.live = nrows
        self.aligned = [self._vector(v, 4, device) for v in self.vecs]
        self.late = [self._vector(v, 1, device) for v in self.vecs]
        self.misalign_last = layout == "d"

    def _vector(self, v, off, device):
        buf = torch.full((off + self.n + 3,), NAN, dtype=torch.float32)
        buf[off:off + self.n] = v
        return buf.to(device)[off:]

    def keep_rows(self, r):
        """Rows from ``r`` on become NaN (call with decreasing ``r``)."""
        assert r <= self.live
        self.A[r:self.live] = NAN
        self.live = r

    def rhs(self, nc):
        B = list(self.aligned[:nc])
        if self.misalign_last:
            B[nc - 1] = self.late[nc - 1]
        return B


_DOT_REF = {}


def dot_reference(inp):
    """(A B^T, |A| |B|^T) of the clean values, float64 ``[nrows, nvec]`` on the host: the int64
    product for integers (exact), else exact float64 products summed pairwise."""
    if inp.key not in _DOT_REF:
        if inp.kind == "int":
            ref = (inp.clean.long() @ inp.vecs.long().T).double()
            mag = (inp.clean.long().abs() @ inp.vecs.long().abs().T).double()
        else:
            a = inp.clean.numpy().astype(np.float64)
            ref = np.empty((inp.nrows, len(inp.vecs)))
            mag = np.empty_like(ref)
            for c, b in enumerate(inp.vecs.numpy().astype(np.float64)):
                p = a * b
                ref[:, c] = p.sum(axis=1)
                mag[:, c] = np.abs(p).sum(axis=1)
            ref, mag = torch.from_numpy(ref), torch.from_numpy(mag)
        _DOT_REF[inp.key] = (ref, mag)
    return _DOT_REF[inp.key]


def _multidot(nrows_max, n, device):
    md = MultiDot(nrows_max, n, device)
    md.out = torch.full((nrows_max * 4 + 8,), NAN, dtype=torch.float64, device=device)
    return md


def _call_dot(md, A, r, B):
    """One call on a NaN workspace and a NaN ``out``: the finite ``[r, nc]`` result (host)."""
    md.out.fill_(NAN)
    if hasattr(md, "ws"):
        md.ws.fill_(NAN)
    md(A, r, B)
    host = md.out.cpu()
    used = r * len(B)
    assert bool(torch.isfinite(host[:used]).all()), "a result is not finite"
    assert bool(torch.isnan(host[used:]).all()), "out was written past nrows * nc"
    return host[:used].view(r, len(B))


def check_multi_dot_exact(device, layout, n, rows=ROWS, ncs=NCS):
    """Integer data: bitwise the int64 product, twice, for every row and vector count."""
    rows = sorted(rows, reverse=True)
    inp = Inputs(device, layout, n, rows[0], "int")
    ref = dot_reference(inp)[0]
    md = _multidot(rows[0], n, device)  # one workspace serves every row count below it
    for r in rows:
        inp.keep_rows(r)
        for nc in ncs:
            B = inp.rhs(nc)
            got = _call_dot(md, inp.A, r, B)
            assert torch.equal(got, ref[:r, :nc]), (layout, n, r, nc)
            assert torch.equal(_call_dot(md, inp.A, r, B), got), (layout, n, r, nc)


def lane_chain(cus, layout, n, nrows):
    """Upper bound of the longest float32 lane chain on a device of ``cus`` CUs (module
    docstring)."""
    tpb = 64 if nrows >= 4 else 256
    vw, chunks = (4, n >> 2) if layout in ("a", "b") else (1, n)
    bx_min = max(1, min(-(-chunks // tpb), cus))
    return vw * -(-chunks // (bx_min * tpb)) + (1 if vw == 4 and n % 4 else 0)


def chain_length(device, layout, n, nrows):
    """``lane_chain`` for the kernels on ``device``; 0 for the float64 fallback on the CPU."""
    if device.type == "cpu":
        return 0
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return lane_chain(cus, layout, n, nrows)


def assert_within(got, ref, bound, what):
    """``|got - ref| <= bound`` element by element; returns the worst ``err / bound``."""
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert bool((err <= bound).all()), f"{what}: max err / bound = {worst:.4g}"
    return worst


def dot_bound(L, mag):
    return (L * U / (1.0 - L * U) + 2.0 ** -40) * mag


def check_multi_dot_bound(device, layout, n, rows=ROWS, ncs=NCS):
    """Normal data against the derived bound; prints the worst err / bound per path."""
    rows = sorted(rows, reverse=True)
    inp = Inputs(device, layout, n, rows[0], "normal")
    ref, mag = dot_reference(inp)
    md = _multidot(rows[0], n, device)
    worst = {}
    for r in rows:
        inp.keep_rows(r)
        bound = dot_bound(chain_length(device, layout, n, r), mag)
        for nc in ncs:
            got = _call_dot(md, inp.A, r, inp.rhs(nc))
            w = assert_within(got, ref[:r, :nc], bound[:r, :nc], f"multi_dot {layout} n={n} r={r} nc={nc}")
            split = "split" if r >= 4 else "not split"
            worst[split] = max(worst.get(split, 0.0), w)
    for split, w in sorted(worst.items()):
        print(f"multi_dot [{device.type}] {PATH[layout]}, {split}, n={n}: max err / bound = {w:.4f}")
    return worst


def check_bound_has_teeth(device):
    """The bound check passes on the true reference and rejects one with a single product
    removed from one row (n = 1027): a dropped element cannot hide inside the bound."""
    n, r, nc = 1027, 5, 2
    inp = Inputs(device, "b", n, r, "normal")
    ref, mag = dot_reference(inp)
    got = _call_dot(_multidot(r, n, device), inp.A, r, inp.rhs(nc))
    bound = dot_bound(chain_length(device, "b", n, r), mag)[:r, :nc]
    assert_within(got, ref[:r, :nc], bound, "true reference")
    prod = inp.clean[2].double() * inp.vecs[1].double()
    bad = ref[:r, :nc].clone()
    bad[2, 1] -= prod[int(prod.abs().argmax())]
    with pytest.raises(AssertionError):
        assert_within(got, bad, bound, "perturbed reference")


# ------------------------------------------------------------------------------- lincomb
def _lincomb_references(inp, coef, rows):
    """{nrows: (sum_i c_i H_i, sum_i |c_i H_i|)} in float64, rows added in order (exact for
    integers; else nrows roundings of 2^-53, nothing against the float32 bound)."""
    acc = torch.zeros(inp.n, dtype=torch.float64)
    mag = torch.zeros(inp.n, dtype=torch.float64)
    out = {}
    for i in range(max(rows) + 1):
        if i in rows:
            out[i] = (acc.clone(), mag.clone())
        if i < inp.nrows:
            t = inp.clean[i].double() * float(coef[i])
            acc += t
            mag += t.abs()
    return out


def _nan_slice(n, off, device):
    buf = torch.full((off + n + 4,), NAN, dtype=torch.float32, device=device)
    return buf, buf[off:off + n]


def check_lincomb(device, kind, layout, n, rows=LINCOMB_ROWS):
    """``lincomb_`` against float64: bitwise for integers (alpha = -2), within the derived
    bound for normal data (alpha 0 and -0.5); with and without ``x``; and bitwise equal to
    ``lincomb_cols_`` with one column (for normal data on the kernels only: the two
    fallbacks go through different float64 products)."""
    rows = sorted(rows, reverse=True)
    R = rows[0]
    inp = Inputs(device, layout, n, R, kind, nvec=1)
    gen = torch.Generator().manual_seed(104729 * n + R)
    coef = _draw(torch.empty(max(R, 1), dtype=torch.float32), kind, gen)
    refs = _lincomb_references(inp, coef, rows)
    x64 = inp.vecs[0].double()
    # aligned x and y with the padded H (lincomb_cols then takes float4), one float late else
    off = 4 if layout == "pad" else 1
    x = inp.aligned[0] if layout == "pad" else inp.late[0]
    worst = 0.0
    for r in rows:
        inp.keep_rows(r)
        cbuf = torch.full((R + 3,), NAN, dtype=torch.float32)
        cbuf[:r] = coef[:r]
        cdev = cbuf.to(device)
        rowsum, rowmag = refs[r]
        for alpha in ((-2.0,) if kind == "int" else (0.0, -0.5)):
            for use_x in (True, False):
                ybuf, y = _nan_slice(n, off, device)
                lincomb_(inp.A, r, cdev, alpha, x if use_x else None, y)
                host = ybuf.cpu()
                got = host[off:off + n].double()
                assert bool(torch.isnan(host[:off]).all() and torch.isnan(host[off + n:]).all())
                assert bool(torch.isfinite(got).all()), (kind, layout, n, r, alpha, use_x)
                ref = rowsum + (alpha * x64 if use_x else 0.0)
                what = f"lincomb {kind} {layout} n={n} nrows={r} alpha={alpha} x={use_x}"
                if kind == "int":
                    assert torch.equal(got, ref), what
                else:
                    k = r + 2
                    bound = k * U / (1.0 - k * U) * (rowmag + ((alpha * x64).abs() if use_x else 0.0))
                    worst = max(worst, assert_within(got, ref, bound, what))
                if r == 0 and not use_x:
                    assert not bool(got.any()), what  # exact zeros
                y2buf, y2 = _nan_slice(n, off, device)
                lincomb_cols_(inp.A, r, cdev[:r].view(r, 1), alpha, x[None] if use_x else None, y2[None])
                if kind == "int" or device.type != "cpu":
                    assert torch.equal(y2buf.cpu()[off:off + n].double(), got), what + " (one column)"
    if kind != "int":
        print(f"lincomb [{device.type}] {layout} n={n}: max err / bound = {worst:.4f}")
    return worst


def check_lincomb_refuses_257_rows(device):
    H = torch.zeros((257, 8), dtype=torch.float32, device=device)
    coef = torch.zeros(257, dtype=torch.float32, device=device)
    y = torch.zeros(8, dtype=torch.float32, device=device)
    lincomb_(H, 256, coef, 0.0, None, y)
    with pytest.raises(ValueError):
        lincomb_(H, 257, coef, 0.0, None, y)


def check_refuses_bad_arguments(device):
    """The extension raises instead of computing (device tensors only: it has no CPU path)."""
    from multigrad_amd.ops._ext import ext
    E = ext()
    n = 64
    f32 = dict(dtype=torch.float32, device=device)
    f64 = dict(dtype=torch.float64, device=device)
    H, coef = torch.ones((4, n), **f32), torch.ones(8, **f32)
    x, y = torch.ones(2 * n, **f32), torch.empty(2 * n, **f32)
    E.lincomb(H, 2, coef, 0.5, x[:n], n, y[:n])  # the well-formed call
    for bad in (lambda: E.lincomb(H, 2, coef, 0.5, x[::2], n, y[:n]),       # strided x
                lambda: E.lincomb(H, 2, coef, 0.5, x[:n], n, y[::2]),       # strided y
                lambda: E.lincomb(H, 2, coef[::2], 0.5, x[:n], n, y[:n]),   # strided coef
                lambda: E.lincomb(H, 2, coef, 0.5, x[:n], -1, y[:n]),
                lambda: E.lincomb(H, -1, coef, 0.5, x[:n], n, y[:n])):
        with pytest.raises(RuntimeError):
            bad()
    A = torch.ones((243, n), **f32)
    B = [torch.ones(n, **f32) for _ in range(5)]
    out = torch.zeros(243 * 4, **f64)
    ws = torch.zeros(E.multi_dot_workspace(243, n), **f64)
    small = torch.zeros(E.multi_dot_workspace(4, n), **f64)
    E.multi_dot(A, 243, B[:4], n, out, ws)  # the well-formed call
    for bad in (lambda: E.multi_dot(A, 243, B[:4], -1, out, ws),
                lambda: E.multi_dot(A, -1, B[:4], n, out, ws),
                lambda: E.multi_dot(A.double(), 243, B[:4], n, out, ws),    # float64 A
                lambda: E.multi_dot(A, 243, B[:4], n, out.float(), ws),     # float32 out
                lambda: E.multi_dot(A, 243, B[:4], n, out, small),          # workspace of 4 rows
                lambda: E.multi_dot(A, 243, B[:4], n + 1, out, ws),         # n > A.size(1)
                lambda: E.multi_dot(A, 243, B, n, out, ws),                 # five vectors
                lambda: E.multi_dot(A, 243, [B[0], B[1][:n - 1]], n, out, ws)):  # a short B
        with pytest.raises(RuntimeError):
            bad()


# ------------------------------------------------------------------- L-BFGS to its tolerance
GTOL = 1e-5
_CPU_NIT = {}


def _quadratic(n):
    """f(x) = 1/2 (x - c)^T (diag(D) + v v^T) (x - c), condition number about 1e3."""
    rng = np.random.default_rng(n)
    D = np.logspace(-3, 0, n)
    rng.shuffle(D)
    v = rng.normal(size=n) / np.sqrt(n)
    c = rng.uniform(-1.0, 1.0, size=n)

    def f_and_g(x):
        r = x - c
        vr = float(v @ r)
        return 0.5 * (float(r @ (D * r)) + vr * vr), D * r + v * vr

    return f_and_g


def run_quadratic(device, n, m):
    """The objective is float64 on the host and hands back a float32 gradient, so the vector
    ops are the only float32 arithmetic of the run.  Returns the result and the float64
    max|g| at ``res.x``."""
    f_and_g = _quadratic(n)

    def lg(x):
        f, g = f_and_g(x.detach().double().cpu().numpy())
        return torch.tensor(f, dtype=torch.float64), torch.from_numpy(g).float().to(device)

    res = run_lbfgs_device(lg, torch.zeros(n, dtype=torch.float32, device=device), maxsteps=3000,
                           history=m, ftol=0.0, gtol=GTOL, hess_inv=False)
    gmax = float(np.abs(f_and_g(res.x.detach().double().cpu().numpy())[1]).max())
    return res, gmax


def check_lbfgs_reaches_gtol(device, n, m):
    """Converged by the gradient test, in at most twice the iterations of the same call on
    CPU tensors (float64 dot products: the reference; the factor allows for the discrete
    branches of the line search).  The 1 % covers rounding the gradient to float32."""
    if (n, m) not in _CPU_NIT:
        _CPU_NIT[(n, m)] = run_quadratic(CPU, n, m)[0].nit
    res, gmax = run_quadratic(device, n, m)
    print(f"lbfgs [{device.type}] n={n} m={m}: nit={res.nit} (CPU tensors {_CPU_NIT[(n, m)]}) "
          f"max|g|={gmax:.3e} status={res.status}")
    assert res.status == 0, res.message
    assert gmax <= 1.01 * GTOL
    assert res.nit <= 2 * _CPU_NIT[(n, m)]
    return res


# ------------------------------------------------------------------------------ the CPU runs
EXACT_CASES = [(lay, n) for n in EXACT_N for lay in "abcde" if layout_fits(lay, n)]
BOUND_CASES = [(lay, n) for n in BOUND_N for lay in "abc" if layout_fits(lay, n)]


@pytest.mark.parametrize("layout,n", EXACT_CASES)
def test_multi_dot_exact(layout, n):
    check_multi_dot_exact(CPU, layout, n)


def test_multi_dot_exact_at_a_two_trip_size():
    check_multi_dot_exact(CPU, "b", TWO_TRIPS[0][0], rows=(4,), ncs=(3,))


@pytest.mark.parametrize("layout,n", BOUND_CASES)
def test_multi_dot_bound(layout, n):
    check_multi_dot_bound(CPU, layout, n)


def test_bound_has_teeth():
    check_bound_has_teeth(CPU)


def test_chain_length_formula():
    """The bound's L on a device of 256 CUs, by hand: n = 65 539 on the float4 path has 16 384
    chunks; 4+ rows: 256 blocks of 64 lanes, one chunk each (+ the tail element) = 5; 1-3 rows:
    64 blocks of 256 lanes = 5; scalar: 65 539 / (256 * 64) -> 5 and 65 539 / (256 * 256) -> 2."""
    assert lane_chain(256, "b", 65_539, 4) == 5 and lane_chain(256, "b", 65_539, 3) == 5
    assert lane_chain(256, "c", 65_539, 4) == 5 and lane_chain(256, "c", 65_539, 3) == 2
    assert lane_chain(256, "a", 1028, 243) == 4 and lane_chain(256, "b", 3, 1) == 1
    assert lane_chain(256, "c", 4_195_331, 1) == 65 and lane_chain(256, "a", 0, 1) == 0
    assert chain_length(CPU, "b", 65_539, 4) == 0


@pytest.mark.parametrize("layout", LINCOMB_LAYOUTS)
@pytest.mark.parametrize("n", LINCOMB_N[:-1])
@pytest.mark.parametrize("kind", ["int", "normal"])
def test_lincomb(kind, n, layout):
    check_lincomb(CPU, kind, layout, n)


@pytest.mark.parametrize("kind", ["int", "normal"])
def test_lincomb_at_the_two_trip_size(kind):
    check_lincomb(CPU, kind, "odd", LINCOMB_N[-1], rows=(2, 0))


def test_lincomb_refuses_257_rows():
    check_lincomb_refuses_257_rows(CPU)


@pytest.mark.parametrize("m", [1, 10, 120])
@pytest.mark.parametrize("n", [1027, 1028])
def test_lbfgs_reaches_gtol(n, m):
    res = check_lbfgs_reaches_gtol(CPU, n, m)
    assert math.isfinite(res.fun)
