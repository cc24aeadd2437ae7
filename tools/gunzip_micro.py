#!/usr/bin/env python3
"""GPU micro-benchmark of the inflate kernels (core/hip/inflate.hip), in one
process.

Three archives of ``--mib`` MiB each are gzipped in HBM by
``engine.gzip_compress_device`` (this project's own format): ``words`` (Huffman
chunks), ``bf16_tar`` (bf16 weights behind a tar header block) and ``random``
(incompressible: every chunk stored, so the member is ONE span that a single
wave hops and copies). Each member is then planned and emitted; before any
timing the output is compared with the source.

Times are host clocks around ``gunzip_plan_device`` (scan, measure, span table
D2H, chain walk) and ``gunzip_emit_device`` (emit, CRC-32), each of which ends
in a device synchronise; take kernel time alone from a ``rocprofv3
--kernel-trace --stats`` run of this tool. ``--cpu`` adds what the pull does
without the kernels: ``zlib.decompressobj`` over the same member on one core,
fed 1 MiB at a time as ``_stream_targz_to_device`` feeds it (no network, no
staging copy).

``--stock`` takes the members from ``zlib`` instead (one unflushed stream per
payload and level, what stock clients write) and plans them with
``search=True``: block search, symbolic windows, window chain.

    python tools/gunzip_micro.py [--mib 64] [--reps 5] [--warmup 1] [--cpu]
                                 [--stock [--levels 1 6 9]]
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from modelx_amd import _core  # noqa: E402
from tools.gzip_micro import payloads as gzip_payloads  # noqa: E402


def payloads(n, device):
    out = gzip_payloads(n, device)
    g = torch.Generator(device="cpu").manual_seed(1)
    out["random"] = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g).to(device)
    return out


def timed(fn, warmup, reps):
    ts = []
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t = time.perf_counter() - t0
        if rep >= warmup:
            ts.append(t)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, nargs="+", default=[64])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--stock", action="store_true")
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 6, 9])
    args = ap.parse_args()
    if not _core.hip_available():
        raise SystemExit("gunzip_micro needs a GPU")
    eng = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=1)
    result = {"reps": args.reps, "warmup": args.warmup, "runs": []}
    search = {"search": True} if args.stock else {}
    for mib in args.mib:
        n = mib << 20
        cases = [(name, src, level) for name, src in payloads(n, "cuda:0").items()
                 for level in (args.levels if args.stock else [None])]
        for name, src, level in cases:
            torch.cuda.synchronize()  # the engine's stream does not order against torch's
            if args.stock:
                co = zlib.compressobj(level, zlib.DEFLATED, 31)
                member = co.compress(src.cpu().numpy().tobytes()) + co.flush()
                stored = len(member)
                gz = torch.frombuffer(bytearray(member + bytes(16)), dtype=torch.uint8).to("cuda:0")
            else:
                bound = _core.gzip_compress_bound(n)
                gz = torch.empty(bound, dtype=torch.uint8, device="cuda:0")
                stored = eng.gzip_compress_device(src.data_ptr(), n, gz.data_ptr(), bound)
            plan = eng.gunzip_plan_device(gz.data_ptr(), stored, **search)
            assert plan["status"] == "ok" and plan["out_bytes"] == n, plan["status"]
            out = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            eng.gunzip_emit_device(gz.data_ptr(), stored, plan["plan"], out.data_ptr(), n)
            assert torch.equal(out, src), "the output is not the source"
            t_plan = timed(lambda: eng.gunzip_plan_device(gz.data_ptr(), stored, **search),
                           args.warmup, args.reps)
            if args.stock:  # the timed plan calls made the emit's plan stale
                plan = eng.gunzip_plan_device(gz.data_ptr(), stored, **search)
            t_emit = timed(lambda: eng.gunzip_emit_device(gz.data_ptr(), stored, plan["plan"],
                                                          out.data_ptr(), n),
                           args.warmup, args.reps)
            gib = n / (1 << 30)
            both = statistics.median(t_plan) + statistics.median(t_emit)
            run = {"mib": mib, "payload": name, "ratio": stored / n, "spans": plan["spans"],
                   "plan_median_ms": statistics.median(t_plan) * 1e3,
                   "emit_median_ms": statistics.median(t_emit) * 1e3,
                   "emit_min_ms": min(t_emit) * 1e3, "emit_max_ms": max(t_emit) * 1e3,
                   "gib_s": gib / both}
            if args.stock:
                run["level"] = level
            if args.cpu:
                member = gz[:stored].cpu().numpy().tobytes()
                inflater = zlib.decompressobj(16 + zlib.MAX_WBITS)
                t0 = time.perf_counter()
                got = sum(len(inflater.decompress(member[i:i + (1 << 20)]))
                          for i in range(0, len(member), 1 << 20))
                run["cpu_zlib_ms"] = (time.perf_counter() - t0) * 1e3
                run["cpu_zlib_gib_s"] = gib / (run["cpu_zlib_ms"] / 1e3)
                assert got + len(inflater.flush()) == n
            print(run, flush=True)
            result["runs"].append(run)
            del src, gz, out
    print(json.dumps(result))


if __name__ == "__main__":
    main()
