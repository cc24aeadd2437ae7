"""Multi-GPU fan-out: land a pulled index on all (or a subset of) the 8
MI355X of a node, RCCL over xGMI (torch.distributed backend "nccl" IS RCCL
on ROCm).

No reference counterpart (the reference is single-destination) — SURVEY.md
§2.2/§5 "distributed backend". Topology notes: each MI355X has 7
point-to-point xGMI links (~153 GB/s each). A ring broadcast serializes on
one link, so for full replication we use RCCL's tree/binomial broadcast via
``dist.broadcast`` per pipeline chunk, overlapped with the next chunk's S3
fetch (double-buffered). For sharded placement every rank range-GETs its own
1/N of the blobs (N× S3 concurrency) and replication, when requested, is a
per-blob broadcast from the owner rank.

Choreography (plan building, chunk schedule, owner assignment) is pure
Python and unit-tested on CPU with the gloo backend; only the transfer
callables touch HIP.
"""
from __future__ import annotations

import threading
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

from ..wire import types
from .gpu_rules import payload_descriptors

DEFAULT_PIPELINE_CHUNK = 256 << 20


@dataclass
class ShardPlan:
    """blob name -> owner rank, greedy size-balanced (largest first)."""

    owners: Dict[str, int] = field(default_factory=dict)
    rank_bytes: List[int] = field(default_factory=list)

    @classmethod
    def build(cls, descs: Sequence[types.Descriptor], world_size: int) -> "ShardPlan":
        plan = cls(owners={}, rank_bytes=[0] * world_size)
        for d in sorted(descs, key=lambda d: -d.size):
            owner = min(range(world_size), key=lambda r: plan.rank_bytes[r])
            plan.owners[d.name] = owner
            plan.rank_bytes[owner] += d.size
        return plan


def chunk_schedule(size: int, chunk: int = DEFAULT_PIPELINE_CHUNK) -> List[Tuple[int, int]]:
    """[(offset, length)] pipeline chunks for a blob."""
    out = []
    off = 0
    while off < size:
        ln = min(chunk, size - off)
        out.append((off, ln))
        off += ln
    return out or [(0, 0)]


def broadcast_blob_pipelined(dist, tensor, size: int, src_rank: int,
                             fetch_chunk: Optional[Callable[[int, int], None]],
                             chunk: int = DEFAULT_PIPELINE_CHUNK,
                             group=None) -> None:
    """Broadcast `tensor[:size]` from src_rank, chunk by chunk. On the source
    rank, ``fetch_chunk(offset, length)`` produces chunk bytes into the
    tensor before its broadcast; fetch of chunk k+1 overlaps the collective
    of chunk k (fetch releases the GIL inside the native engine)."""
    sched = chunk_schedule(size, chunk)
    is_src = dist.get_rank(group) == src_rank if group is not None else dist.get_rank() == src_rank

    fetch_threads: List[threading.Thread] = []
    if is_src and fetch_chunk is not None:
        # prefetch chunk 0 synchronously, then overlap
        fetch_chunk(*sched[0])
    for i, (off, ln) in enumerate(sched):
        if ln == 0:
            continue
        if is_src and fetch_chunk is not None and i + 1 < len(sched):
            t = threading.Thread(target=fetch_chunk, args=sched[i + 1])
            t.start()
            fetch_threads.append(t)
        view = tensor.narrow(0, off, ln)
        dist.broadcast(view, src=src_rank, group=group)
        if fetch_threads:
            fetch_threads[-1].join()


def fanout_pull_broadcast(dist, gpu_client, repository: str, version: str,
                          device: int, chunk: int = DEFAULT_PIPELINE_CHUNK,
                          src_rank: int = 0, verify: bool = True,
                          skip_sidecars: bool = True):
    """All-replicate pull: rank `src_rank` fetches from S3, every rank ends
    with all blobs in its HBM (BASELINE config 4 replicate mode). Every rank
    verifies its own copy on-GPU — corruption anywhere in S3, host ring,
    PCIe or xGMI is caught at the destination.

    Accepts any client with the GpuClient surface; a client without an
    ``engine`` (the bench's CPU dry-run stand-in) runs the SAME chunk
    schedule and collectives on CPU tensors over gloo — the choreography is
    identical, only the transfer/verify callables differ."""
    import torch

    is_gpu = hasattr(gpu_client, "engine")
    dev = f"cuda:{device}" if is_gpu else "cpu"
    rank = dist.get_rank()
    manifest = gpu_client.remote.get_manifest(repository, version)
    out = {}
    for desc in payload_descriptors(manifest, skip_sidecars):
        tensor = torch.empty(desc.size, dtype=torch.uint8, device=dev)
        fetch = None
        if rank == src_rank:
            if is_gpu:
                located = gpu_client._download_url(repository, desc)
                if located is None:
                    raise RuntimeError("fan-out needs a presigned location "
                                       "(registry without --enable-redirect)")
                url, headers = located

                def fetch(off, ln, _url=url, _h=headers, _t=tensor):
                    gpu_client.engine.pull_to_device(_url, _h, ln, _t.data_ptr() + off,
                                                     gpu_client.num_conns, off)
            else:
                # CPU dry-run: materialize the blob before the broadcasts
                buf = b"".join(gpu_client.remote.get_blob_content(repository, desc.digest))
                tensor.copy_(torch.frombuffer(bytearray(buf), dtype=torch.uint8))
        broadcast_blob_pipelined(dist, tensor, desc.size, src_rank, fetch, chunk)
        if verify:
            if is_gpu:
                # the collective is async on torch's stream; the verify
                # kernel runs on the engine's own stream with no implicit
                # ordering — sync or the digest reads torn bytes
                torch.cuda.synchronize(device)
                gpu_client._verify_device_digest(tensor.data_ptr(), desc.size, desc)
            else:
                from ..wire import digest as dg

                raw = tensor.numpy().tobytes()
                target = desc.digest or desc.annotations.get(
                    types.ANNOTATION_CHUNK_DIGEST, "")
                if target and not dg.verify_bytes(raw, target):
                    raise RuntimeError(f"fan-out digest mismatch for {desc.name}")
        out[desc.name] = tensor
    return out


def fanout_pull_sharded(dist, gpu_client, repository: str, version: str, device: int,
                        replicate: bool = False, verify: bool = True):
    """Sharded pull: rank r fetches the blobs ShardPlan assigns it (N× S3
    concurrency across the node). With replicate=True each blob is then
    broadcast from its owner so every rank holds the full set."""
    import torch

    rank = dist.get_rank()
    world = dist.get_world_size()
    manifest = gpu_client.remote.get_manifest(repository, version)
    descs = [d for d in manifest.blobs
             if d.size > 0 and d.media_type != types.MEDIA_TYPE_MODEL_LEAVES]
    plan = ShardPlan.build(descs, world)
    out = {}
    owned = [d for d in descs if plan.owners[d.name] == rank]
    if owned:
        # concurrent shard pulls (reentrant engine; per-blob latency would
        # otherwise stack across a rank's whole 1/N of the index)
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=min(len(owned), 6)) as ex:
            for name, t in ex.map(
                    lambda d: (d.name,
                               gpu_client.pull_blob_to_device(repository, d, verify=verify)),
                    owned):
                out[name] = t
    if replicate:
        for desc in descs:
            if plan.owners[desc.name] != rank:
                out[desc.name] = torch.empty(desc.size, dtype=torch.uint8,
                                             device=f"cuda:{device}")
    if replicate:
        # owners stream their blobs to everyone (binomial broadcast per blob;
        # different owners' broadcasts use disjoint xGMI links)
        for desc in descs:
            tensor = out[desc.name]
            broadcast_blob_pipelined(dist, tensor, desc.size, plan.owners[desc.name], None)
            if verify and plan.owners[desc.name] != rank:
                torch.cuda.synchronize(device)  # order collective before engine read
                gpu_client._verify_device_digest(tensor.data_ptr(), desc.size, desc)
    return out


def fanout_pull_single_process(ref, manifest: types.Manifest,
                               selection: Sequence[types.Descriptor],
                               devices: Sequence[int]):
    """modelxdl --gpus helper: one process, shard blobs across local devices
    (each device gets its own engine; no collectives needed)."""
    from .gpu import GpuClient

    plan = ShardPlan.build(selection, len(devices))
    clients = {d: GpuClient(ref.registry, ref.authorization, device=d) for d in devices}
    out: Dict[int, Dict[str, object]] = {d: {} for d in devices}
    for desc in selection:
        dev = devices[plan.owners[desc.name]]
        out[dev][desc.name] = clients[dev].pull_blob_to_device(ref.repository, desc)
    return out
