#!/usr/bin/env python3
"""GPU micro-benchmark of content-defined chunk dedup, in one process.

Part 1 — kernels on --mib MiB (default 1 GiB) of random bytes, each an engine
call timed by a host clock around a device synchronise (so set-up, the list
copy and the host selection are included; take kernel time alone from a
``rocprofv3 --kernel-trace --stats`` run with --kernel-only):
``Tensor.copy_`` (D2D), ``sha256_chunk_leaves`` at 128 KiB, ``cdc_candidates``
at 16 bits, ``cdc_chunks`` at the defaults, ``sha256_multibuf`` over those
chunks, then ``dedup_pull_ranges`` of the CDC chunks into a destination one
byte off the source's phase beside ``dedup_pull`` of the 128 KiB grid chunks.
Before any timing ``cdc_chunks`` is checked against ``_core.cdc_chunks_host``.

Part 2 — end to end at the default parameters: tensor A and B = A with 37 bytes
inserted at offset 5000, pushed with ``cdc=True``; a fresh client pulls A then
B with ``cdc`` off and on. Reported per mode: fetched bytes and wall time of
B's pull.

    python tools/cdc_micro.py [--mib 1024] [--reps 5] [--warmup 1] [--kernel-only]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from modelx_amd import _core  # noqa: E402

CS = 128 << 10


def kernel_part(args, src, result):
    size = src.numel()
    eng = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=1)
    ptr = src.data_ptr()
    back = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    chunks = eng.cdc_chunks(ptr, size)
    assert chunks == _core.cdc_chunks_host(src.cpu().numpy().tobytes()), "chunks differ from host"
    where = [(ptr + o, ln) for o, ln in chunks]
    eng.dedup_reset(1 << 20)
    eng.dedup_register_ranges(eng.sha256_multibuf(where), ptr, chunks)
    leaves = eng.sha256_chunk_leaves(ptr, size, CS)
    eng.dedup_register(leaves, ptr, CS, size)
    digests = eng.sha256_multibuf(where)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    work = {"copy_": lambda: back[:size].copy_(src),
            "sha256_chunk_leaves_128k": lambda: eng.sha256_chunk_leaves(ptr, size, CS),
            "cdc_candidates_16": lambda: eng.cdc_candidates(ptr, size, 16),
            "cdc_chunks_defaults": lambda: eng.cdc_chunks(ptr, size),
            "sha256_multibuf_cdc_chunks": lambda: eng.sha256_multibuf(where),
            "gather_ranges_mixed_phase": lambda: eng.dedup_pull_ranges(
                digests, chunks, back.data_ptr() + 1),
            "gather_grid": lambda: eng.dedup_pull(leaves, back.data_ptr(), CS, size)}
    for _ in range(args.warmup):
        for fn in work.values():
            timed(fn)
    times = {k: [] for k in work}
    for _ in range(args.reps):
        for k, fn in work.items():
            times[k].append(timed(fn))
    missing, got = eng.dedup_pull_ranges(digests, chunks, back.data_ptr() + 1)
    assert got == size and not missing and torch.equal(back[1:size + 1], src)
    gib = size / (1 << 30)
    result["chunks"] = len(chunks)
    result["kernels"] = {k: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v),
                             "gib_per_s_median": gib / statistics.median(v)}
                         for k, v in times.items()}


def e2e_part(args, src, result):
    from util_servers import start_modelxd_s3, start_s3d

    from modelx_amd.client.gpu import GpuClient

    root = tempfile.mkdtemp(prefix="cdc-micro-", dir="/dev/shm" if os.path.isdir("/dev/shm")
                            else None)
    s3d = start_s3d(os.path.join(root, "s3"))
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    try:
        extra = torch.randint(0, 256, (37,), dtype=torch.uint8, device="cuda")
        b = torch.cat([src[:5000], extra, src[5000:]])
        g = GpuClient(mdx.url, device=0)
        g.push_from_gpu("micro/cdc", "a", {"w.bin": src}, cdc=True)
        g.push_from_gpu("micro/cdc", "b", {"w.bin": b}, cdc=True)
        result["push_cdc"] = [s for s in g.last_stats if s["phase"] == "push-cdc"]
        del g
        out = {}
        for mode, options in (("grid_only", {}), ("cdc", {"cdc": True})):
            c = GpuClient(mdx.url, device=0, dedup=True, **options)
            c.pull_to_gpu("micro/cdc", "a")
            c.last_stats.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = c.pull_to_gpu("micro/cdc", "b")["w.bin"]
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert torch.equal(got, b)
            stats = {s["phase"]: s for s in c.last_stats}
            fetched = sum(s.get("bytes", 0) for p, s in stats.items()
                          if p in ("pull-cdc", "pull-dedup", "pull-transfer",
                                   "pull-transfer-hashed", "pull-chunk-refetch"))
            out[mode] = {"wall_s": wall, "fetched_bytes": fetched, "size": b.numel(),
                         "phases": sorted(stats)}
            del c, got
        result["e2e"] = out
    finally:
        mdx.stop()
        s3d.stop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    src = torch.randint(0, 256, (args.mib << 20,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    result = {"mib": args.mib, "reps": args.reps}
    kernel_part(args, src, result)
    if not args.kernel_only:
        e2e_part(args, src, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
