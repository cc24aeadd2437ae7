#!/usr/bin/env python3
"""GPU micro-benchmark of the ChaCha20-Poly1305 kernel (core/hip/aead.hip),
in one process.

``engine.aead_seal`` (source -> a second buffer) and ``engine.aead_open`` (in
place) of 64 MiB and 1 GiB of seeded random bytes at segment sizes of 64, 128
and 256 KiB, and in the same rounds ``Tensor.copy_`` of the same bytes: a D2D
hipMemcpyAsync, which like the kernel reads and writes every byte once and is
the yardstick. Before any timing, at each size and segment, the first two
segments of the sealed blob and their tags are checked against
``_core.aead_seal_host``, the host model, and an open must return -1 and the
source bytes.

Times are host clocks around calls that end in a device synchronise, so they
include each call's set-up; take kernel time alone from a ``rocprofv3
--kernel-trace --stats`` run of this tool. An open leaves plaintext behind, so
every timed open is preceded by an untimed seal of the same buffer.

    python tools/aead_micro.py [--mib 64 1024] [--seg-kib 64 128 256] [--reps 10] [--warmup 2]
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

KEY = bytes(range(32))


def check(eng, src, sealed, n, seg):
    """The kernel at the size that is timed, against the host model: a
    whole-blob host seal of 1 GiB would take a long time, so the check is the
    first two segments, which the host can seal alone because a segment
    depends only on its index and the last-segment flag. The tests cover the
    rest against the reference."""
    eng.aead_seal(KEY, src.data_ptr(), n, sealed.data_ptr(), seg)
    nseg = (n + seg - 1) // seg
    host = src[:2 * seg].cpu().numpy().tobytes()
    want = _core.aead_seal_host(KEY, host + b"\0", seg)  # a third segment keeps these non-last
    got = sealed[:2 * seg].cpu().numpy().tobytes()
    tags = sealed[n:n + 32].cpu().numpy().tobytes()
    assert got == want[:2 * seg], "first segments differ from the host model"
    assert tags == want[2 * seg + 1:2 * seg + 33], "first tags differ from the host model"
    assert eng.aead_open(KEY, sealed.data_ptr(), n + 16 * nseg, n, seg) == -1
    assert torch.equal(sealed[:n], src), "open does not return the source"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--seg-kib", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not _core.hip_available():
        raise SystemExit("aead_micro needs a GPU")
    eng = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=1)
    result = {"reps": args.reps, "warmup": args.warmup, "runs": []}
    for mib in args.mib:
        n = mib << 20
        g = torch.Generator(device="cuda:0").manual_seed(0)
        src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0", generator=g)
        torch.cuda.synchronize()  # the engine's stream does not order against torch's
        segs = [k << 10 for k in args.seg_kib]
        sealed = torch.empty(n + 16 * ((n + min(segs) - 1) // min(segs)), dtype=torch.uint8,
                             device="cuda:0")
        for seg in segs:
            check(eng, src, sealed, n, seg)
        stored = {seg: n + 16 * ((n + seg - 1) // seg) for seg in segs}
        work = {"copy_": (None, lambda: sealed[:n].copy_(src))}
        for seg in segs:
            seal = (lambda seg=seg: eng.aead_seal(KEY, src.data_ptr(), n, sealed.data_ptr(), seg))
            work[f"seal_{seg >> 10}k"] = (None, seal)
            work[f"open_{seg >> 10}k"] = (seal, lambda seg=seg: eng.aead_open(
                KEY, sealed.data_ptr(), stored[seg], n, seg))
        times = {k: [] for k in work}
        for rep in range(args.warmup + args.reps):
            for k, (before, fn) in work.items():
                if before:
                    before()
                t = timed(fn)
                if rep >= args.warmup:
                    times[k].append(t)
        gib = n / (1 << 30)
        run = {"mib": mib}
        for k, ts in times.items():
            rates = sorted(gib / t for t in ts)
            run[k] = {"median_ms": statistics.median(ts) * 1e3,
                      "median_gib_s": statistics.median(rates),
                      "min_gib_s": rates[0], "max_gib_s": rates[-1]}
            print(f"{mib:5d} MiB {k:10s} median {run[k]['median_ms']:9.3f} ms  "
                  f"{run[k]['median_gib_s']:8.1f} GiB/s (min {rates[0]:.1f}, max {rates[-1]:.1f}) "
                  f"= {run[k]['median_gib_s'] / run['copy_']['median_gib_s']:.2f} of copy_",
                  flush=True)
        result["runs"].append(run)
        del src, sealed
    print(json.dumps(result))


if __name__ == "__main__":
    main()
