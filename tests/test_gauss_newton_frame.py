"""The one damped-loop frame of the three Gauss-Newton drivers (``optim/_damped.py``) against
a recording of the three hand-kept loops it replaced: the order of the Jacobian and loss
calls, the counters, the messages, the damping trail and the iterates of small float64 CPU
problems that between them leave every driver through every exit."""
import json
import os

import pytest
import torch

from multigrad_amd.optim.gauss_newton import run_gauss_newton, run_gauss_newton_dual
from multigrad_amd.optim.gauss_newton_box import run_gauss_newton_box

F64 = torch.float64
DRIVERS = {"dense": run_gauss_newton, "dual": run_gauss_newton_dual, "box": run_gauss_newton_box}

# sumstats S_k = sum_p A_kp x_p (1 + b x_p), loss = 1/2 sum_k w_k (S_k - t_k)^2: closed forms
# in + - * / only, so the recording depends on no libm
A = [[1.0, 0.5, -0.3, 0.2, 0.1, -0.4],
     [0.2, -1.0, 0.4, 0.3, -0.2, 0.1],
     [-0.1, 0.3, 1.0, -0.5, 0.2, 0.3],
     [0.4, 0.1, -0.2, 1.0, 0.5, -0.1]]
W = [1.0, 2.0, 0.5, 1.5]
T = [1.0, -0.5, 0.7, 0.2]

WIDE = dict(K=2, P=3, b=0.0, x0=[0.0, 0.0, 0.0])       # linear, more parameters than sumstats
TALL = dict(K=3, P=2, b=0.1, x0=[0.0, 0.0])            # a residual stays at the optimum
SIX = dict(K=4, P=6, b=0.05, x0=[0.2, -0.1, 0.0, 0.1, -0.2, 0.3])
TIGHT = [(-1.0, 1.0), (-1.0, 0.1), (-0.05, None)]      # the free optimum of WIDE lies outside


def _case(name, drivers, problem, **kw):
    extra = {k: kw.pop(k) for k in ("at_target", "hsign", "poison", "nan_loss") if k in kw}
    return [dict(name=f"{name}-{d}", driver=d, problem=dict(problem, **extra),
                 kwargs={k: v for k, v in kw.items() if d == "box" or k not in BOX_ONLY})
            for d in drivers]


BOX_ONLY = ("param_bounds", "max_step", "min_damping", "inner_passes")
ALL, DUALS = ("dense", "dual", "box"), ("dual", "box")
CASES = sum([
    _case("gtol_start", ALL, dict(WIDE, x0=[0.5, -0.25, 1.0]), at_target=True),
    _case("gtol_later", ALL, WIDE, ftol=0.0),
    _case("ftol", ALL, TALL, gtol=0.0),
    _case("ftol_six", ALL, SIX, gtol=0.0, ftol=1e-4),
    _case("maxsteps", ALL, TALL, gtol=0.0, ftol=0.0, maxsteps=2),
    _case("low_damping", ("dense", "dual"), TALL, gtol=0.0, ftol=0.0, maxsteps=3, damping=1e-11),
    _case("nan_loss", ALL, TALL, nan_loss=True),
    _case("zero_gn", ALL, WIDE, hsign=0.0),
    _case("nonfinite_start", DUALS, dict(WIDE, x0=[1.0, 0.0, 0.0]), poison=True),
    _case("nonfinite_reeval", DUALS, WIDE, poison=True, ftol=1.0),
    _case("nonfinite_next", DUALS, WIDE, poison=True, ftol=0.0),
    _case("floor", ("box",), TALL, gtol=0.0, ftol=0.0, maxsteps=3),
    _case("floor_above_start", ("box",), TALL, gtol=0.0, damping=1e-6, min_damping=1e-2),
    _case("active", ("box",), WIDE, param_bounds=TIGHT),
    _case("one_pass", ("box",), WIDE, param_bounds=TIGHT, inner_passes=1, maxsteps=8),
    _case("outside", ("box",), dict(WIDE, x0=[2.0, -3.0, 0.0]), param_bounds=TIGHT),
    _case("capped", ("box",), SIX, max_step=0.05, gtol=0.0, ftol=1e-4),
    _case("capped_bounded", ("box",), SIX, max_step=[0.05, 0.1, 0.2, 0.05, 0.1, 0.2],
          param_bounds=[(-0.3, 0.3)] * 6, gtol=0.0, inner_passes=3),
], [])


def _callables(problem, driver, log):
    K, P, b = problem["K"], problem["P"], problem["b"]
    a = torch.tensor([row[:P] for row in A[:K]], dtype=F64)
    w = torch.tensor(W[:K], dtype=F64)

    def sumstats(x):
        return (a * (x * (1.0 + b * x))).sum(1)

    x0 = torch.tensor(problem["x0"], dtype=F64)
    t = sumstats(x0) if problem.get("at_target") else torch.tensor(T[:K], dtype=F64)
    hw = problem.get("hsign", 1.0) * w

    def parts(x):
        x = torch.as_tensor(x, dtype=F64).reshape(-1)
        r = sumstats(x) - t
        J = a * (1.0 + 2.0 * b * x)
        if problem.get("poison"):   # finite only at x_0 = 0; the loss does not know of it
            J[0, 0] = J[0, 0] + (1e200 * x[0]) * (1e200 * x[0])
        return 0.5 * (w * r * r).sum(), w * r, J

    def loss_fn(x):
        log.append("L")
        loss = parts(x)[0]
        return (loss - loss) / 0.0 if problem.get("nan_loss") else loss

    def dense_fn(x):
        log.append("J")
        loss, c, J = parts(x)
        G = (J[:, :, None] * (hw[:, None, None] * J[:, None, :])).sum(0)
        return loss, (c[:, None] * J).sum(0), G, "forward"

    def factors_fn(x):
        log.append("J")
        loss, c, J = parts(x)
        return loss, c, J, torch.diag(hw), "forward"

    return (dense_fn if driver == "dense" else factors_fn), loss_fn, x0


def run_case(case):
    """What the fixture records of one run, as JSON types."""
    log = []
    jac_fn, loss_fn, x0 = _callables(case["problem"], case["driver"], log)
    res = DRIVERS[case["driver"]](jac_fn, loss_fn, x0, **case["kwargs"])
    rec = dict(calls="".join(log), nit=res.nit, nfev=res.nfev, njev=res.njev,
               success=res.success, message=res.message, jac_mode=res.jac_mode,
               x=torch.as_tensor(res.x).reshape(-1).tolist(), fun=float(res.fun))
    for key in ("solver", "host_copy_sizes", "damping", "damping_floor", "inner_passes",
                "inner_unconverged"):
        if key in res:
            rec[key] = res[key]
    if "trials" in res:
        rec["trials"] = [[float(lam), int(n), bool(ok), bool(acc)] for lam, n, ok, acc in res.trials]
        rec["active"] = res.active.reshape(-1).tolist()
    return rec


with open(os.path.join(os.path.dirname(__file__), "golden", "gauss_newton_traces.json")) as _fh:
    GOLDEN = json.load(_fh)

NOT_FINITE = "the Jacobian or the loss derivatives are not finite at the current point"


def _exits(case, rec):
    """The exits and branches of the loop that a recorded run went through."""
    out, msg, kw = set(), rec["message"], case["kwargs"]
    if msg.endswith("<= gtol"):
        out.add("gtol_start" if rec["njev"] == 1 else "gtol_later")
    if msg.endswith("<= ftol"):
        out.add("ftol")
    if msg.startswith("maximum number") and rec["nit"] == kw.get("maxsteps"):
        out.add("maxsteps")
    if "damping above 1e12" in msg:
        out.add("zero_gn" if case["problem"].get("hsign") == 0.0 else "damping_ceiling")
    if msg == NOT_FINITE:
        # with ftol = 1 every accepted step passes the ftol rule, so the last J is its re-evaluation
        out.add("nonfinite_first" if rec["calls"] == "J" else
                "nonfinite_reeval" if kw.get("ftol") == 1.0 else "nonfinite_later")
    floor = kw.get("min_damping", 1e-4) if case["driver"] == "box" else 1e-12
    if rec.get("damping", None) == floor or (kw.get("damping") == 1e-11 and rec["nit"] >= 2):
        out.add("floor")
    if rec.get("inner_unconverged", 0) > 0 and kw.get("inner_passes") == 1:
        # the same problem with the default passes ends on its bounds (the "active" case)
        assert kw["param_bounds"] is TIGHT and case["problem"] == dict(WIDE)
        out.add("inner_out_of_passes")
    if "param_bounds" in kw and any(
            not (lo is None or lo <= v) or not (hi is None or v <= hi)
            for v, (lo, hi) in zip(case["problem"]["x0"], kw["param_bounds"])):
        out.add("start_outside")
    return out


def test_golden_cases_reach_every_exit():
    """Every driver leaves through every exit it has, on a recorded case."""
    assert [c["name"] for c in CASES] == list(GOLDEN["cases"])
    reached = {d: set() for d in DRIVERS}
    for case in CASES:
        reached[case["driver"]] |= _exits(case, GOLDEN["cases"][case["name"]])
    common = {"gtol_start", "gtol_later", "ftol", "maxsteps", "damping_ceiling", "floor"}
    assert reached["dense"] >= common
    duals = common | {"zero_gn", "nonfinite_first", "nonfinite_reeval", "nonfinite_later"}
    assert reached["dual"] >= duals
    assert reached["box"] >= duals | {"inner_out_of_passes", "start_outside"}
    # a rejected trial that cost a loss evaluation, and one that did not
    box = [GOLDEN["cases"][c["name"]] for c in CASES if c["driver"] == "box"]
    assert any(ok and not acc for r in box for _, _, ok, acc in r["trials"])
    assert any(not ok for r in box for _, _, ok, _ in r["trials"])
    assert any(r["damping_floor"] > 1e-4 for r in box)
    assert any(GOLDEN["cases"]["active-box"]["active"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_drivers_repeat_the_recorded_runs(case):
    """Everything discrete exactly; ``x`` and ``fun`` to the tolerance in the fixture's header:
    100 times the spread of the recording itself between 1 and 16 threads, at least 1e-13,
    relative to ``max |x|`` and to ``max(|fun|, 1)``, the scale of the ftol rule."""
    want = dict(GOLDEN["cases"][case["name"]])
    got = run_case(case)
    tol = GOLDEN["tolerance"]
    assert tol == max(100.0 * GOLDEN["thread_spread"], 1e-13)
    for key in ("x", "fun"):
        g, w = got.pop(key), want.pop(key)
        g, w = (g, w) if key == "x" else ([g], [w])
        scale = max([abs(v) for v in w] + ([1.0] if key == "fun" else []))
        assert len(g) == len(w)
        assert all(abs(gv - wv) <= tol * scale for gv, wv in zip(g, w)), (key, g, w)
    assert got == want
