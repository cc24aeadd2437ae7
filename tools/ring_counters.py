"""Pinned-ring slot-wait counters on the flagship benchmark's shape.

Runs bench.py's single-GPU pipelined step (push of step k on a side thread
while step k-1 is pulled, same client, same defaults) and reports
``slot_wait_seconds`` per direction: the time engine threads spent blocked
for a pinned slot, summed over the threads of every call (8 pull workers per
pull, up to 6 part uploads per push), next to the wall time of the timed
region. The engine returns the counter in the stats of ``pull_to_device*``
and ``push_part_from_device``; GpuClient drops the latter, so this tool
records it through a thin wrapper around the engine.

  python tools/ring_counters.py --steps 20 --warmup 5

Prints one JSON line (profiles/pinned_ring.md).
"""
import argparse
import json
import os
import shutil
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))


class RecordingEngine:
    """Forwards everything to the engine and keeps the stats dict of every
    part upload."""

    def __init__(self, engine):
        self._engine = engine
        self._lock = threading.Lock()
        self.push_stats = []

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def push_part_from_device(self, *args, **kwargs):
        stats = self._engine.push_part_from_device(*args, **kwargs)
        with self._lock:
            self.push_stats.append(stats)
        return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blob-gib", type=float, default=8.0)
    ap.add_argument("--conns", type=int, default=8)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--slot-mib", type=int, default=64)
    ap.add_argument("--part-mib", type=int, default=256)
    args = ap.parse_args()

    import torch

    from bench_shapes import start_stack
    from modelx_amd.client.gpu import GpuClient

    torch.cuda.set_device(0)
    store = ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp") + "/modelx-ring-counters"
    procs, url = start_stack(0, store)
    try:
        g = GpuClient(url, device=0, num_slots=args.slots, slot_bytes=args.slot_mib << 20,
                      num_conns=args.conns)
        g.engine = RecordingEngine(g.engine)
        repo = "bench/ring"
        src = torch.empty(int(args.blob_gib * (1 << 30)), dtype=torch.uint8, device="cuda:0")
        torch.manual_seed(0)

        def gen():
            src.random_(0, 256)
            torch.cuda.synchronize(0)

        def push(k):
            g.push_from_gpu(repo, f"s{k}", {"blob.bin": src}, part_bytes=args.part_mib << 20)

        def clean(k):
            g.remote.delete_manifest(repo, f"s{k}")
            g.remote.garbage_collect(repo)

        for w in range(args.warmup):
            gen()
            push(1000 + w)
            g.pull_to_gpu(repo, f"s{1000 + w}", verify=True)
            g.remote.delete_index(repo)
        g.last_stats.clear()
        g.engine.push_stats.clear()
        torch.cuda.synchronize(0)
        t0 = time.monotonic()
        gen()
        push(0)
        for k in range(1, args.steps):
            gen()
            th = threading.Thread(target=push, args=(k,))
            th.start()
            g.pull_to_gpu(repo, f"s{k - 1}", verify=True)
            th.join()
            clean(k - 1)
        g.pull_to_gpu(repo, f"s{args.steps - 1}", verify=True)
        clean(args.steps - 1)
        torch.cuda.synchronize(0)
        wall = time.monotonic() - t0

        pulls = [s for s in g.last_stats if str(s.get("phase", "")).startswith("pull-transfer")]
        parts = g.engine.push_stats
        print(json.dumps({
            "steps": args.steps,
            "wall_s": round(wall, 3),
            "gib_per_s": round(2 * args.blob_gib * args.steps / wall, 3),
            "pull": {"calls": len(pulls),
                     "seconds": round(sum(s["seconds"] for s in pulls), 3),
                     "slot_wait_seconds": round(sum(s["slot_wait_seconds"] for s in pulls), 3),
                     "threads_per_call": args.conns},
            "push": {"part_calls": len(parts),
                     "seconds": round(sum(s["seconds"] for s in parts), 3),
                     "slot_wait_seconds": round(sum(s["slot_wait_seconds"] for s in parts), 3)},
        }), flush=True)
    finally:
        for p in procs:
            p.stop()
        shutil.rmtree(store, ignore_errors=True)


if __name__ == "__main__":
    main()
