#!/usr/bin/env python3
"""GPU micro-benchmark of the CRC-32C part-checksum path, in one process.

Part 1 — kernel (core/hip/crc32c.hip) against a device-to-device copy of the
same bytes: ``engine.crc32c_ranges`` over --mib MiB (default 1 GiB) as ONE
range and as 16 equal ranges, and ``Tensor.copy_`` of the same buffer (a D2D
hipMemcpyAsync, which reads every byte once and also writes it). Before any
timing the 16 values are checked against ``_core.crc32c_host`` of the same
bytes, and their ``crc32c_combine`` against the one-range value.

Part 2 — end to end: ``push_from_gpu`` of the same tensor with
``part_checksum`` off and on, alternating, against modelx-s3d + modelxd with
the store on tmpfs. Every push gets fresh content (the first bytes are
rewritten) so nothing is deduplicated, and its objects are removed afterwards.
Reported per mode: the push's wall time, and for "on" the
``push-part-checksum`` phase of ``last_stats`` (the kernel call); the rest of
the difference is the store reading bodies through user space and
checksumming them instead of splicing.

Times are host clocks around calls that end in a device synchronise, so they
include each call's set-up; take kernel time alone from a ``rocprofv3
--kernel-trace --stats`` run of this tool.

    python tools/crc32c_micro.py [--mib 1024] [--reps 10] [--warmup 2] [--e2e-reps 3]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from modelx_amd import _core  # noqa: E402


def kernel_part(args, src, result):
    size = src.numel()
    eng = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=1)
    back = torch.empty_like(src)
    ptr = src.data_ptr()
    one = [(ptr, size)]
    part = size // 16
    many = [(ptr + i * part, part) for i in range(16)]

    # results first: the kernel at the size that is timed, against the host
    got = eng.crc32c_ranges(many)
    host = src.cpu().numpy()
    want = [_core.crc32c_host(host[i * part:(i + 1) * part].tobytes()) for i in range(16)]
    assert got == want, "16-range values differ from the host's"
    whole = got[0]
    for c in got[1:]:
        whole = _core.crc32c_combine(whole, c, part)
    assert eng.crc32c_ranges(one) == [whole], "one-range value differs from the combined parts"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    work = {"copy_": lambda: back.copy_(src),
            "crc32c_1_range": lambda: eng.crc32c_ranges(one),
            "crc32c_16_ranges": lambda: eng.crc32c_ranges(many)}
    for _ in range(args.warmup):
        for fn in work.values():
            timed(fn)
    times = {k: [] for k in work}
    for _ in range(args.reps):
        for k, fn in work.items():
            times[k].append(timed(fn))
    gib = size / (1 << 30)
    for k, ts in times.items():
        rates = sorted(gib / t for t in ts)
        r = result[k] = {"median_ms": statistics.median(ts) * 1e3,
                         "median_gib_s": statistics.median(rates),
                         "min_gib_s": rates[0], "max_gib_s": rates[-1]}
        print(f"{k:18s} median {r['median_ms']:9.3f} ms  {r['median_gib_s']:8.1f} GiB/s read "
              f"(min {r['min_gib_s']:.1f}, max {r['max_gib_s']:.1f}) over {args.reps} reps",
              flush=True)
    for k in ("crc32c_1_range", "crc32c_16_ranges"):
        result[k + "_over_copy"] = result[k]["median_gib_s"] / result["copy_"]["median_gib_s"]
        print(f"{k}/copy_ = {result[k + '_over_copy']:.2f}", flush=True)


def push_part(args, src, result):
    from util_servers import start_modelxd_s3, start_s3d

    from modelx_amd.client.gpu import GpuClient

    size = src.numel()
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    root = tempfile.mkdtemp(prefix="modelx-crc-", dir=shm)
    if shutil.disk_usage(root).free < 3 * size:
        shutil.rmtree(root)
        raise SystemExit(f"crc32c_micro: {root} has less than {3 * size} bytes free")
    s3d = start_s3d(root)
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    walls = {"": [], "crc32c": []}
    kernel = []
    try:
        g = GpuClient(mdx.url, device=0)
        stamp = torch.zeros(8, dtype=torch.uint8, device=src.device)
        n = 0
        for rep in range(1 + args.e2e_reps):  # the first pair is the warm-up
            for mode in ("", "crc32c"):
                n += 1
                stamp[:] = torch.tensor(list(n.to_bytes(8, "little")), dtype=torch.uint8)
                src[:8] = stamp  # fresh digest: nothing is deduplicated
                g.last_stats.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g.push_from_gpu(f"bench/r{n}", "v1", {"w.bin": src}, part_checksum=mode)
                wall = time.perf_counter() - t0
                shutil.rmtree(os.path.join(root, "modelx", "registry", "bench"),
                              ignore_errors=True)
                if rep == 0:
                    continue
                walls[mode].append(wall)
                if mode:
                    kernel.append(sum(s["seconds"] for s in g.last_stats
                                      if s["phase"] == "push-part-checksum"))
    finally:
        mdx.stop()
        s3d.stop()
        shutil.rmtree(root, ignore_errors=True)
    off, on = statistics.median(walls[""]), statistics.median(walls["crc32c"])
    ker = statistics.median(kernel)
    result["push"] = {"bytes": size, "reps": args.e2e_reps, "off_s": off, "on_s": on,
                      "off_all_s": walls[""], "on_all_s": walls["crc32c"],
                      "part_checksum_phase_s": ker,
                      "kernel_share_of_push": ker / on,
                      "store_and_rest_s": on - off - ker}
    gib = size / (1 << 30)
    print(f"push off {off:.3f} s ({gib / off:.1f} GiB/s)  on {on:.3f} s ({gib / on:.1f} GiB/s)  "
          f"push-part-checksum {ker * 1e3:.3f} ms = {100 * ker / on:.2f}% of the push; "
          f"rest of the difference {on - off - ker:.3f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e-reps", type=int, default=3)
    args = ap.parse_args()
    if not _core.hip_available():
        raise SystemExit("crc32c_micro needs a GPU")
    size = (args.mib << 20) // 256 * 256
    g = torch.Generator(device="cuda:0").manual_seed(0)
    src = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda:0", generator=g)
    result = {"bytes": size, "reps": args.reps, "warmup": args.warmup}
    kernel_part(args, src, result)
    if args.e2e_reps:
        push_part(args, src, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
