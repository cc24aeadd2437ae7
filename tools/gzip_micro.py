#!/usr/bin/env python3
"""GPU micro-benchmark of the DEFLATE kernel (core/hip/deflate.hip), in one
process.

``engine.gzip_compress_device`` of 64 MiB and 1 GiB of two payloads: bf16
weights (seeded normal values) behind one 512 B tar header block, and ``words``
(a seeded join of a 200-word vocabulary). Before any timing, at each size, the
output is inflated by zlib and compared with the source, and the chunks of its
first 1 MiB are checked against ``_core.gzip_compress_host``, the host model.

Times are host clocks around a call that ends in a device synchronise, so they
include the call's size read-back and gather launch; take kernel time alone
from a ``rocprofv3 --kernel-trace --stats`` run of this tool. ``--cpu`` adds
the CPU path the kernel replaces, ``zlib.compress`` at level 9 (what
``helper.tgz`` runs) on the first ``--cpu-mib`` MiB of the same bytes on one core.
``--ratio`` needs no GPU: the host model's size next to zlib levels 1 and 6.

    python tools/gzip_micro.py [--mib 64 1024] [--reps 5] [--warmup 1] [--cpu] [--ratio]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from modelx_amd import _core  # noqa: E402


def words_mib():
    r = random.Random(7)
    vocab = [bytes(r.randrange(97, 123) for _ in range(r.randrange(2, 9))) for _ in range(200)]
    out = bytearray()
    while len(out) < 1 << 20:
        out += r.choice(vocab) + b" "
    return bytes(out[:1 << 20])


def payloads(n, device):
    """{name: uint8 tensor of n bytes}. `words` repeats 1 MiB of text, each
    repeat rotated by its index so that 32 KiB chunks differ."""
    g = torch.Generator(device="cpu").manual_seed(0)
    w = torch.randn((n - 512) // 2, generator=g).to(torch.bfloat16).view(torch.uint8)
    tar = torch.cat([torch.zeros(512, dtype=torch.uint8), w])
    base = torch.frombuffer(bytearray(words_mib()), dtype=torch.uint8)
    text = torch.cat([torch.roll(base, 997 * i) for i in range(n >> 20)])
    return {"bf16_tar": tar.to(device), "words": text.to(device)}


def ratio_table(mib):
    out = {}
    for name, t in payloads(mib << 20, "cpu").items():
        x = t.numpy().tobytes()
        out[name] = {"host_model": len(_core.gzip_compress_host(x)) / len(x),
                     "zlib_1": len(zlib.compress(x, 1)) / len(x),
                     "zlib_6": len(zlib.compress(x, 6)) / len(x)}
        print(name, {k: round(v, 4) for k, v in out[name].items()}, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-mib", type=int, default=64)
    ap.add_argument("--ratio", action="store_true")
    args = ap.parse_args()
    result = {"reps": args.reps, "warmup": args.warmup, "runs": []}
    if args.ratio:
        result["ratio_16mib"] = ratio_table(16)
        print(json.dumps(result))
        return
    if not _core.hip_available():
        raise SystemExit("gzip_micro needs a GPU")
    eng = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=1)
    for mib in args.mib:
        n = mib << 20
        for name, src in payloads(n, "cuda:0").items():
            torch.cuda.synchronize()  # the engine's stream does not order against torch's
            bound = _core.gzip_compress_bound(n)
            out = torch.empty(bound, dtype=torch.uint8, device="cuda:0")
            stored = eng.gzip_compress_device(src.data_ptr(), n, out.data_ptr(), bound)
            host = src.cpu().numpy().tobytes()
            got = out[:stored].cpu().numpy().tobytes()
            assert zlib.decompress(got, 31) == host, "zlib does not return the source"
            # one byte more, so that the chunks of the first MiB are not last;
            # the byte's own stored chunk and the trailer are the last 14 bytes
            head = _core.gzip_compress_host(host[:(1 << 20) + 1])
            assert got[:len(head) - 14] == head[:-14], "differs from the host model"
            ts = []
            for rep in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.gzip_compress_device(src.data_ptr(), n, out.data_ptr(), bound)
                t = time.perf_counter() - t0
                if rep >= args.warmup:
                    ts.append(t)
            gib = n / (1 << 30)
            rates = sorted(gib / t for t in ts)
            run = {"mib": mib, "payload": name, "ratio": stored / n,
                   "median_ms": statistics.median(ts) * 1e3,
                   "median_gib_s": statistics.median(rates),
                   "min_gib_s": rates[0], "max_gib_s": rates[-1]}
            if args.cpu:
                part = host[:args.cpu_mib << 20]
                t0 = time.perf_counter()
                zlib.compress(part, 9)
                run["cpu_zlib9_gib_s"] = len(part) / (1 << 30) / (time.perf_counter() - t0)
            print(run, flush=True)
            result["runs"].append(run)
            del src, out
    print(json.dumps(result))


if __name__ == "__main__":
    main()
