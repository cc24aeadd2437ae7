#!/usr/bin/env python3
"""GPU micro-benchmark of the tar pack kernel (core/hip/tar.hip) against a
device-to-device ``Tensor.copy_`` of the same bytes, in one process.

Workloads (default 16 members of 64 MiB = 1 GiB of payload):
  pack phase 0   members are 16-byte aligned tensors
  pack phase 1   members are views base[1:], one byte off the 16-byte grid
  copy_          torch D2D copy of the same 1 GiB

Every repetition runs the three back to back, so drift on a shared machine
hits them alike. Times are host clocks around calls that end in a device
synchronise; ``engine.tar_pack`` includes its per-call set-up (two small
allocations, the header/segment upload, the launch and the stream sync), so
the kernel alone is faster than the call — take kernel time from a
``rocprofv3 --kernel-trace --stats`` run of this same tool.

    python tools/tar_pack_micro.py [--members 16] [--member-mib 64] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from modelx_amd import _core  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--member-mib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not _core.hip_available():
        raise SystemExit("tar_pack_micro needs a GPU")

    n, size = args.members, args.member_mib << 20
    eng = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=1)
    bases = [torch.randint(0, 256, (size + 16,), dtype=torch.uint8, device="cuda:0")
             for _ in range(n)]
    names = [f"bench/member{i:02d}.bin" for i in range(n)]
    total = _core.tar_pack_layout([(nm, size) for nm in names])["total"]
    archive = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    flat_src = torch.randint(0, 256, (n * size,), dtype=torch.uint8, device="cuda:0")
    flat_dst = torch.empty_like(flat_src)
    payload = n * size

    def members(phase):
        views = [b[phase:phase + size] for b in bases]
        assert all(v.data_ptr() % 16 == phase for v in views)
        return [(nm, v.data_ptr(), size) for nm, v in zip(names, views)]

    def run_pack(mem):
        t0 = time.perf_counter()
        eng.tar_pack(archive.data_ptr(), total, mem)  # returns after its stream sync
        return time.perf_counter() - t0

    def run_copy():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flat_dst.copy_(flat_src)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    work = {"pack_phase0": lambda m=members(0): run_pack(m),
            "pack_phase1": lambda m=members(1): run_pack(m),
            "copy_": run_copy}
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        for fn in work.values():
            fn()
    times = {k: [] for k in work}
    for _ in range(args.reps):
        for k, fn in work.items():
            times[k].append(fn())

    # the packed archive must be the one the layout describes (phase 1 ran last)
    first = archive[512:512 + 4096].cpu()
    assert torch.equal(first, bases[0][1:1 + 4096].cpu())

    gib = payload / (1 << 30)
    result = {"payload_bytes": payload, "archive_bytes": total, "members": n,
              "reps": args.reps, "warmup": args.warmup}
    for k, ts in times.items():
        rates = sorted(gib / t for t in ts)
        result[k] = {"median_ms": statistics.median(ts) * 1e3,
                     "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
                     "median_gib_s": statistics.median(rates),
                     "min_gib_s": rates[0], "max_gib_s": rates[-1]}
        r = result[k]
        print(f"{k:12s} median {r['median_ms']:.3f} ms  {r['median_gib_s']:.0f} GiB/s of payload "
              f"(min {r['min_gib_s']:.0f}, max {r['max_gib_s']:.0f}) over {args.reps} reps")
    for k in ("pack_phase0", "pack_phase1"):
        result[k + "_over_copy"] = result[k]["median_gib_s"] / result["copy_"]["median_gib_s"]
        print(f"{k}/copy_ = {result[k + '_over_copy']:.2f}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
