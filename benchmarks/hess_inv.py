"""Cost of the device inverse-Hessian operator (optim/invhess.py) at P = 1e7, k = 10, one GPU.

In one process, alternating, 5 rounds each:

* ``apply`` with 1 and with 4 columns against the same products composed from the ops the
  optimizers already had (per column one ``MultiDot`` and one ``lincomb_``);
* ``diagonal()`` against a float4 copy that moves the same number of bytes.

Prints a markdown table (time per call: best and spread over the rounds, bytes moved, rate)
and one JSON line; ``--out`` also writes the table to a file.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MULTIGRAD_PROGRESS", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from multigrad_amd.ops.lbfgs import MultiDot, lincomb_  # noqa: E402
from multigrad_amd.optim._reduce import DeviceReducer  # noqa: E402
from multigrad_amd.optim.invhess import DeviceLbfgsInvHessProduct, IdentityLayout  # noqa: E402


def make_operator(P, k, dev, seed=0):
    """An operator over k synthetic accepted pairs in a ring of k + 1 slots."""
    R = k + 1
    g = torch.Generator(device=dev).manual_seed(seed)
    HS = torch.zeros((2 * R, P), device=dev)
    for q in range(k):
        HS[q] = torch.randn(P, generator=g, device=dev)
        HS[R + q] = HS[q] + 0.3 * torch.randn(P, generator=g, device=dev)
    SY, YY = np.zeros((R, R)), np.zeros((R, R))
    dot = MultiDot(2 * R, P, dev)
    for q in range(k):  # the optimizers' own inner products (fp64 results)
        d = dot(HS, 2 * R, [HS[q], HS[R + q]]).cpu().numpy()
        SY[:, q] = d[:R, 1]   # s_i . y_q
        YY[:, q] = d[R:, 1]   # y_i . y_q
    red = DeviceReducer(None, False, dev)
    return DeviceLbfgsInvHessProduct(HS, R, list(range(k)), SY, YY, red, IdentityLayout(P), dot=dot)


def composed_apply(op, V, out, coef, dot):
    """H V column by column from one MultiDot and one lincomb_ per column."""
    R, k, h0 = op.R, op.n_corrs, op.h0
    idx = np.asarray(op.order)
    Q = op._Q()
    for c in range(V.shape[0]):
        d = dot(op.HS, 2 * R, [V[c]])[:, 0].cpu().numpy()
        z = Q @ np.concatenate([d[idx], h0 * d[R + idx]])
        cm = np.zeros(2 * R)
        cm[idx] = z[:k]
        cm[R + idx] = h0 * z[k:]
        coef.copy_(torch.from_numpy(cm.astype(np.float32)))
        lincomb_(op.HS, 2 * R, coef, h0, V[c], out[c])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--P", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device(a.device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("benchmarks/hess_inv.py needs a GPU")
    P, k = a.P, a.k
    op = make_operator(P, k, dev)
    R = op.R
    g = torch.Generator(device=dev).manual_seed(1)
    V4 = torch.randn((4, P), generator=g, device=dev)       # rows = columns of the block
    V4u = V4.T   # [P, 4] as apply() takes it; column-major, so apply() uses it without a copy
    out4 = torch.empty_like(V4)
    coef = torch.zeros(2 * R, device=dev)
    dot1 = MultiDot(2 * R, P, dev)
    nbytes_diag = (2 * k + 1) * 4 * P
    src = torch.empty(nbytes_diag // 8, device=dev)          # a copy reads and writes
    dst = torch.empty_like(src)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    # bytes each variant moves (history rows + vectors read, results written)
    def b_new(c):
        return ((2 * R + c) + (2 * R + 2 * c)) * 4 * P

    def b_old(c):
        return c * ((2 * R + 1) + (2 * R + 2)) * 4 * P

    variants = [
        ("apply, 1 column", lambda: op.apply(V4[0]), b_new(1)),
        ("composed, 1 column", lambda: composed_apply(op, V4[:1], out4, coef, dot1), b_old(1)),
        ("apply, 4 columns", lambda: op.apply(V4u), b_new(4)),
        ("composed, 4 columns", lambda: composed_apply(op, V4, out4, coef, dot1), b_old(4)),
        ("diagonal()", lambda: op.diagonal(), nbytes_diag),
        ("float4 copy, same bytes", lambda: dst.copy_(src), nbytes_diag),
    ]
    # outputs agree before anything is timed
    ref = composed_apply(op, V4, out4, coef, dot1).clone()
    got = op.apply(V4u).T
    agree = float((got - ref).abs().max() / ref.abs().max())
    for _, fn, _ in variants:  # warm-up: code objects, workspaces
        fn()
    sync()
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, fn, _ in variants:
            sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            sync()
            times[name].append((time.perf_counter() - t0) / a.calls)
    lines = [f"P = {P}, k = {k} (ring of {2 * R} rows), {a.rounds} rounds of {a.calls} calls, "
             f"alternating; device {dev}; max |apply - composed| / max |composed| = {agree:.2e}",
             "",
             "| variant | best ms | median ms | worst ms | MB moved | TB/s at best |",
             "|---|---|---|---|---|---|"]
    rec = {}
    for name, _, nb in variants:
        t = sorted(times[name])
        best, med, worst = t[0], t[len(t) // 2], t[-1]
        rec[name] = {"best_ms": best * 1e3, "median_ms": med * 1e3, "worst_ms": worst * 1e3,
                     "bytes": nb}
        lines.append(f"| {name} | {best * 1e3:.3f} | {med * 1e3:.3f} | {worst * 1e3:.3f} | "
                     f"{nb / 1e6:.0f} | {nb / best / 1e12:.2f} |")
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table + "\n")
    print(json.dumps({"metric": "hess_inv operator cost", "P": P, "k": k, "device": str(dev),
                      "agreement": agree, "variants": rec}))


if __name__ == "__main__":
    main()
