"""The driver's bench.py contract on CPU: one JSON line with the required keys, at 1 rank
and at 2 gloo ranks launched by torch.distributed.run (owner and hashed placements)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
        "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"}
ARGS = ["--params", "2000", "--halos", "20000", "--steps", "3", "--warmup", "1"]


def _env():
    env = dict(os.environ, MULTIGRAD_PROGRESS="0", OMP_NUM_THREADS="1",
               MULTIGRAD_DEVICE_COMM="0", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    return env


def _json_lines(out: str):
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def test_bench_single_rank_json():
    r = subprocess.run([sys.executable, "bench.py"] + ARGS + ["--profile-phases"], cwd=ROOT,
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1
    rec = lines[0]
    assert KEYS <= set(rec)
    assert rec["n_gpus"] == 1 and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["value"] > 0 and rec["higher_is_better"] is True
    assert {"model", "global_batch", "seq_len", "parallelism"} <= set(rec["config"])
    assert set(rec["phases_ms"]) >= {"forward", "loss", "vjp", "adam"}


def _dump_run(tmp_path, name, extra=(), env=None):
    import numpy as np
    out = tmp_path / name
    r = subprocess.run([sys.executable, "bench.py"] + ARGS + ["--dump-outputs", str(out)]
                       + list(extra), cwd=ROOT, env=env or _env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    (rec,) = _json_lines(r.stdout)
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    return rec, arrays


def _check_dump(rec, arrays):
    import numpy as np
    assert set(arrays) == {"params", "loss"}
    assert arrays["params"].dtype == np.float32 and arrays["params"].shape == (2000,)
    assert arrays["loss"].dtype == np.float64 and arrays["loss"].shape == (1,)
    assert np.isfinite(arrays["params"]).all()
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    # the dump is the state after exactly warmup + steps steps: its loss is the record's
    assert arrays["loss"][0] == rec["loss_last"]
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert rec["ms_per_step"] == pytest.approx(1e3 / rec["value"], rel=1e-3)


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's parameters and loss as .npy; the inputs
    are seeded, so a second run (here with --full) writes the same arrays."""
    import numpy as np
    rec_a, a = _dump_run(tmp_path, "a")
    rec_b, b = _dump_run(tmp_path, "b", ["--full"])
    _check_dump(rec_a, a)
    _check_dump(rec_b, b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    # the parameters moved from the start (the steps ran) and differ between elements
    assert np.unique(a["params"]).size > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_bench_plain_and_full_gpu(tmp_path, full):
    """On the GPU a plain run skips the device-operation count (a profiler run of its own);
    --full reports it.  Both dump the same kind of outputs."""
    env = dict(os.environ, MULTIGRAD_PROGRESS="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    rec, arrays = _dump_run(tmp_path, "out", ["--full"] if full else [], env=env)
    _check_dump(rec, arrays)
    ops = rec["config"]["device_ops_per_step"]
    assert (ops is not None and len(ops) > 0) if full else ops is None


def test_dump_samples_large_outputs(tmp_path):
    """A parameter vector above the per-array limit is written as a fixed sample."""
    import numpy as np
    import torch
    import bench

    class Eng:
        def params(self):
            return torch.arange(1000, dtype=torch.float32)

        def last_loss(self):
            return 0.5

    class Comm:
        rank = 0

    old = bench.DUMP_MAX_BYTES
    bench.DUMP_MAX_BYTES = 400
    try:
        bench.dump_outputs(str(tmp_path / "a"), Eng(), Comm())
        bench.dump_outputs(str(tmp_path / "b"), Eng(), Comm())
    finally:
        bench.DUMP_MAX_BYTES = old
    a, b = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "b" / "params.npy")
    assert a.shape == (100,) and a.dtype == np.float32 and np.all(np.diff(a) > 0)
    np.testing.assert_array_equal(a, b)
    assert np.load(tmp_path / "a" / "loss.npy")[0] == 0.5


@pytest.mark.parametrize("placement", ["owner", "hashed"])
def test_bench_two_ranks_json(placement):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(29400 + os.getpid() % 500),
           "bench.py", "--gpus", "2", "--placement", placement] + ARGS
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout  # rank 0 only
    rec = lines[0]
    assert KEYS <= set(rec) and rec["n_gpus"] == 2
    assert rec["config"]["placement"] == placement
    assert rec["config"]["optimizer_sharding"] == ("owner" if placement == "owner" else "zero1")


def test_extra_placement_failure_keeps_the_headline():
    """A failure of the extra (owner) placement is reported in the record's errors; a
    failure of the headline placement still ends the run."""
    import bench

    def timed(p):
        if p == "owner":
            raise MemoryError("out of device memory")
        return {"steps_per_s": 1.0}

    released = []
    res, errors = bench.run_placements(["hashed", "owner"], timed,
                                       on_error=lambda: released.append(True))
    assert res == {"hashed": {"steps_per_s": 1.0}}
    assert errors["owner"].startswith("MemoryError: out of device memory")
    assert released == [True]

    def broken(p):
        raise RuntimeError("headline failed")

    with pytest.raises(RuntimeError):
        bench.run_placements(["hashed", "owner"], broken)
