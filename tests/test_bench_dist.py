"""Dry-run of bench.py's multi-rank orchestration under the EXACT torchrun
invocation the driver uses at round end (one rank per GPU) — on CPU via
MODELX_BENCH_CPU=1 (gloo, fake transfer client). Validates rank/port/store
layout, barrier flow, MAX-reduce and the one-line JSON contract for
world_size 2 without needing 8 GPUs."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


import pytest


def _run(tmp_path, world, extra, port):
    env = dict(os.environ, MODELX_BENCH_CPU="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(REPO, "bench.py"),
           "--gpus", str(world), "--steps", "2", "--warmup", "1",
           "--blob-gib", "0.002", "--store", str(tmp_path / "store")] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=REPO, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line expected, got {lines}"
    return json.loads(lines[0])


@pytest.mark.parametrize("world", [2, 4])
def test_torchrun_cpu_dry_run_fanout_default(tmp_path, world):
    """The driver's exact multi-rank invocation lands in fan-out mode:
    shared store, per-rank shard push, every shard broadcast from its owner
    (config-4 semantics — what SCALE measures on an 8-GPU node)."""
    out = _run(tmp_path, world, [], 29671 + world * 40)
    assert out["n_gpus"] == world
    assert out["steps"] == 2
    assert out["scaling"] == "weak"
    assert out["value"] > 0
    assert out["metric"].startswith("push+pull GiB/s")
    assert out["config"]["parallelism"] == f"fanout{world}-rccl-xgmi-broadcast-pipelined"
    assert out["config"]["model"].startswith("config4-")


def _payload(seed, nbytes, draws):
    """Replay bench.py's payload stream: the draws-th random_ fill after
    torch.manual_seed(seed) — the bytes step (draws - 1 - warmup) pushed."""
    import torch

    torch.manual_seed(seed)
    t = torch.empty(nbytes, dtype=torch.uint8)
    for _ in range(draws):
        t.random_(0, 256)
    return t.numpy()


def _expect_dump(payload, world, n_tensors):
    import numpy as np

    import bench

    k = bench.dump_sample_len(world, n_tensors)
    if payload.size > k:
        payload = payload[bench.dump_sample_indices(payload.size, k)]
    return payload.astype(np.float32)


def _digest_str(arr):
    import numpy as np

    return bytes(arr.astype(np.uint8)).decode()


def _load_dir(d):
    import numpy as np

    return {p.name: np.load(p) for p in sorted(d.iterdir())}


@pytest.mark.parametrize("steps", [2, 1])  # pipelined loop / plain one_step loop
def test_dump_outputs_single_rank(tmp_path, steps):
    """--dump-outputs writes the LAST timed step's pulled bytes and the
    digest of that step's push as float32 .npy: both are checked against an
    independent replay of the seeded payload stream (warm-up draw, then one
    draw per step). Same arguments -> identical files from run to run.
    --steps sets the timed step count; --full adds the stage report."""
    import hashlib

    import numpy as np

    env = dict(os.environ, MODELX_BENCH_CPU="1", MASTER_PORT=str(29931 + steps))
    nbytes = (6 << 20) + 5  # above bench.DUMP_SAMPLE: the sampled path
    runs = []
    for tag, extra in (("a", ["--full"]), ("b", [])):
        d = tmp_path / tag
        r = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
             "--steps", str(steps), "--warmup", "1",
             "--blob-gib", repr(nbytes / (1 << 30)),
             "--store", str(tmp_path / "store"), "--dump-outputs", str(d)] + extra,
            capture_output=True, text=True, timeout=300, cwd=REPO, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, lines
        res = json.loads(lines[0])
        assert res["steps"] == steps and res["ms_per_step"] > 0
        assert ("# step 0:" in r.stderr) == bool(extra)
        runs.append(_load_dir(d))
    a, b = runs
    assert sorted(a) == ["blob.bin.digest.npy", "blob.bin.npy"]
    payload = _payload(0, nbytes, 1 + steps)
    assert a["blob.bin.npy"].dtype == np.float32
    assert a["blob.bin.npy"].shape == (4 << 20,)
    assert np.array_equal(a["blob.bin.npy"], _expect_dump(payload, 1, 1))
    assert _digest_str(a["blob.bin.digest.npy"]) == \
        "sha256:" + hashlib.sha256(payload.tobytes()).hexdigest()
    for name in a:
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("steps", [2, 1])  # pipelined fan-out / one_step fan-out arm
def test_dump_outputs_fanout_world2(tmp_path, steps):
    """Fan-out at world 2: every rank dumps every owner's shard as landed in
    its own memory plus the digest of its own push; all files of all ranks
    together stay within 64 MB, each tensor cut to its share of the budget."""
    import hashlib

    import numpy as np

    nbytes = (8 << 20) + 3  # shards 4194305 / 4194306: unequal, both sampled
    shard = [nbytes // 2, nbytes - nbytes // 2]
    d = tmp_path / "dump"
    out = _run(tmp_path, 2, ["--steps", str(steps), "--blob-gib", repr(nbytes / (1 << 30)),
                             "--dump-outputs", str(d)], 30011 + steps * 40)
    assert out["steps"] == steps
    files = _load_dir(d)
    assert sorted(files) == sorted(
        [f"rank{q}.src{r}.shard.bin.npy" for q in (0, 1) for r in (0, 1)]
        + [f"rank{q}.shard.bin.digest.npy" for q in (0, 1)])
    assert sum(p.stat().st_size for p in d.iterdir()) <= 64_000_000
    for r in (0, 1):
        payload = _payload(r, shard[r], 1 + steps)
        want = _expect_dump(payload, 2, 2)
        assert want.size < payload.size  # the budget, not the tensor, set the length
        for q in (0, 1):
            got = files[f"rank{q}.src{r}.shard.bin.npy"]
            assert got.dtype == np.float32 and np.array_equal(got, want), (q, r)
        assert _digest_str(files[f"rank{r}.shard.bin.digest.npy"]) == \
            "sha256:" + hashlib.sha256(payload.tobytes()).hexdigest()


def test_dump_budget_holds_at_every_world():
    """The per-tensor share keeps world x tensors x 4 bytes under the 64 MB
    limit for both step shapes: fan-out lands world tensors per rank,
    independent mode one."""
    import bench

    for world in (1, 2, 3, 4, 8, 16):
        for n_tensors in (1, world):
            k = bench.dump_sample_len(world, n_tensors)
            assert 0 < k <= bench.DUMP_SAMPLE
            # + one digest file per rank: 128-byte header, < 100 characters
            total = world * (n_tensors * (4 * k + 128) + 128 + 4 * 100)
            assert total <= 64_000_000, (world, n_tensors, total)


def test_torchrun_cpu_dry_run_independent_mode(tmp_path):
    """--mode independent keeps the per-rank-stack shape (no collectives in
    the step; A/B comparator for the fan-out)."""
    out = _run(tmp_path, 2, ["--mode", "independent"], 29891)
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2-presigned-s3"
