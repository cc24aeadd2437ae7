#!/usr/bin/env python3
"""GPU micro-benchmark of the byte-plane path, in one process.

Part 1 — kernels (core/hip/byteplane.hip) against a device-to-device copy of
the same bytes: ``engine.byte_planes`` split and merge for E = 2 and 4 at
G = E * 128 KiB on --mib MiB (default 1 GiB), and ``Tensor.copy_`` of the same
buffer (a D2D hipMemcpyAsync). A permutation can do no better than a copy.

Part 2 — codec on the same number of bf16 N(0, 0.02) bytes: ratio, compress
and decode rate of ``engine.zstd_compress_device`` / ``zstd_decompress_device``
- plain       the interleaved bytes, default encoder (what compress="zstd"
              does without planes)
- planes      split + literals-only compress; decode + merge
with the split and merge inside the planes timings, since a push and a pull
pay for them.

Every repetition runs all workloads back to back, so drift on a shared
machine hits them alike. Times are host clocks around calls that end in a
device synchronise, so they include each call's set-up; take kernel time
alone from a ``rocprofv3 --kernel-trace --stats`` run of this tool.

    python tools/byte_planes_micro.py [--mib 1024] [--reps 10] [--warmup 2]
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

FRAME = 128 << 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not _core.hip_available():
        raise SystemExit("byte_planes_micro needs a GPU")

    size = args.mib << 20
    dev = "cuda:0"
    eng = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=1)
    g = torch.Generator(device=dev).manual_seed(0)
    src = (torch.randn(size // 2, device=dev, generator=g) * 0.02).to(torch.bfloat16) \
        .view(torch.uint8)
    planar = torch.empty_like(src)
    back = torch.empty_like(src)
    bound = _core.zstd_compress_bound(size)
    comp_plain = torch.empty(bound, dtype=torch.uint8, device=dev)
    comp_planes = torch.empty(bound, dtype=torch.uint8, device=dev)
    sizes = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def planes(elem, merge):
        a, b = (planar, back) if merge else (src, planar)
        return lambda: eng.byte_planes(
            [(a.data_ptr(), b.data_ptr(), size, elem, elem * FRAME)], merge)

    def compress_plain():
        sizes["plain"] = eng.zstd_compress_device(src.data_ptr(), size, FRAME,
                                                  comp_plain.data_ptr(), bound)

    def compress_planes():
        eng.byte_planes([(src.data_ptr(), planar.data_ptr(), size, 2, 2 * FRAME)], False)
        sizes["planes"] = eng.zstd_compress_device(planar.data_ptr(), size, FRAME,
                                                   comp_planes.data_ptr(), bound,
                                                   literals_only=True)

    def decode_plain():
        eng.zstd_decompress_device(comp_plain.data_ptr(), sizes["plain"], back.data_ptr(), size)

    def decode_planes():
        eng.zstd_decompress_device(comp_planes.data_ptr(), sizes["planes"],
                                   planar.data_ptr(), size)
        eng.byte_planes([(planar.data_ptr(), back.data_ptr(), size, 2, 2 * FRAME)], True)

    # order matters only in that each merge follows the split of its E and
    # each decode follows its compress
    work = {
        "copy_": lambda: back.copy_(src),
        "split_e2": planes(2, False), "merge_e2": planes(2, True),
        "split_e4": planes(4, False), "merge_e4": planes(4, True),
        "compress_plain": compress_plain, "decode_plain": decode_plain,
        "compress_planes": compress_planes, "decode_planes": decode_planes,
    }
    checks = {"merge_e2", "merge_e4", "decode_plain", "decode_planes"}
    for _ in range(args.warmup):
        for k, fn in work.items():
            timed(fn)
            if k in checks:  # results must not change: every round trip is exact
                assert torch.equal(back, src), k
                back.zero_()
    times = {k: [] for k in work}
    for _ in range(args.reps):
        for k, fn in work.items():
            times[k].append(timed(fn))
    assert torch.equal(back, src)

    gib = size / (1 << 30)
    result = {"bytes": size, "reps": args.reps, "warmup": args.warmup,
              "ratio_plain": sizes["plain"] / size, "ratio_planes": sizes["planes"] / size}
    for k, ts in times.items():
        rates = sorted(gib / t for t in ts)
        result[k] = {"median_ms": statistics.median(ts) * 1e3,
                     "median_gib_s": statistics.median(rates),
                     "min_gib_s": rates[0], "max_gib_s": rates[-1]}
        r = result[k]
        print(f"{k:16s} median {r['median_ms']:9.3f} ms  {r['median_gib_s']:8.1f} GiB/s of raw "
              f"bytes (min {r['min_gib_s']:.1f}, max {r['max_gib_s']:.1f}) over {args.reps} reps")
    for k in ("split_e2", "merge_e2", "split_e4", "merge_e4"):
        result[k + "_over_copy"] = result[k]["median_gib_s"] / result["copy_"]["median_gib_s"]
        print(f"{k}/copy_ = {result[k + '_over_copy']:.2f}")
    print(f"ratio plain {result['ratio_plain']:.4f}  planes {result['ratio_planes']:.4f}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
