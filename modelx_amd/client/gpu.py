"""GPU data plane: S3 → HBM pulls and HBM → S3 pushes on MI355X.

Orchestrates the native pinned-ring engine (modelx_amd._core, built from
core/src/engine.cpp + core/hip/sha256.hip):

- ``pull_to_gpu``: manifest → presigned URL per blob → parallel ranged GETs
  into pinned slots → hipMemcpyAsync onto the device buffer → CDNA4 SHA-256
  chunk kernel verifies the chunked digest. Returns ``dict[name,
  torch.Tensor]`` (uint8) resident in HBM.
- ``push_from_gpu``: chunk-digest the device buffers on GPU, presigned
  (multi)part upload streamed D2H through the pinned ring, manifest PUT last.
- multi-GPU fan-out: rank 0 pulls, RCCL broadcast over xGMI per pipeline
  chunk via torch.distributed — see ``fanout.py`` (fanout_pull_broadcast /
  fanout_pull_sharded).

Layout: what a descriptor or a manifest means (which digest a blob is checked
against, at what chunk size, which blobs are payloads, how a push is cut into
parts) is decided in ``gpu_rules.py``, once each. ``pull_blob_to_device`` is
a dispatcher over one ``_land_*`` method per landing strategy;
``push_from_gpu`` digests (``_digest_batched`` / ``_digest_one``) and hands
every blob to ``_upload_blob``.

The native extension is REQUIRED on a GPU box: if HIP devices are visible and
the extension is missing, this module raises instead of silently falling back
to a CPU path.
"""
from __future__ import annotations

import base64
import os
import sys
import time
import zlib
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from datetime import datetime, timezone
from typing import Dict, List, NamedTuple, Optional, Tuple

from ..wire import digest as dg
from ..wire import errors as er
from ..wire import types
from . import gpu_rules as rules
from .gpu_rules import DEFAULT_GPU_CHUNK, leaves_usable
from .gpu_rules import annotated_chunk_size as _annotated_chunk_size
from .push import check_planes
from .registry import RegistryClient

DEFAULT_SLOT_BYTES = 64 << 20
DEFAULT_NUM_SLOTS = 16
DEFAULT_NUM_CONNS = 16  # measured: 16 conns/16 slots -> 17.3 vs 14.3 GiB/s at 8/10 (bench sweep)
DEFAULT_PART_BYTES = 256 << 20  # push part granularity (multipart)
DEFAULT_PUSH_PARALLEL = 6


def _core():
    try:
        from modelx_amd import _core as core
    except ImportError as e:  # pragma: no cover
        raise er.ModelxError(
            er.ErrCode.INTERNAL,
            "modelx_amd._core native extension not built "
            "(python setup_ext.py build_ext --inplace)",
        ) from e
    return core


def _tls_verify() -> bool:
    """requests verify flag for presigned-URL calls; MODELX_TLS_INSECURE=1
    (self-signed stores) matches the native engine's switch."""
    if os.environ.get("MODELX_TLS_INSECURE") == "1":
        import urllib3

        urllib3.disable_warnings()
        return False
    return True


def _signed_headers(part: dict) -> Dict[str, str]:
    return {k: ",".join(v) if isinstance(v, list) else str(v)
            for k, v in (part.get("signedHeader") or {}).items()}


def _map(fn, jobs, parallel: int) -> list:
    """``[fn(j) for j in jobs]``, on a thread pool when ``parallel`` > 1 and
    there is more than one job (the engine is reentrant)."""
    jobs = list(jobs)
    if parallel > 1 and len(jobs) > 1:
        with ThreadPoolExecutor(max_workers=parallel) as ex:
            return list(ex.map(fn, jobs))
    return [fn(j) for j in jobs]


class _PinnedStaging:
    """Bounded pinned staging between a host byte stream and HBM: bytes fed in
    reach ``emit`` as views of one pinned buffer, ``nbytes`` at a time and the
    rest on ``flush``. ``emit`` must be done with a view when it returns."""

    def __init__(self, nbytes: int, emit):
        import torch

        self._buf = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self._frombuffer = torch.frombuffer
        self._fill = 0
        self._emit = emit

    def feed(self, data) -> None:
        view = memoryview(data)
        while view:
            n = min(len(view), self._buf.numel() - self._fill)
            self._buf[self._fill:self._fill + n] = self._frombuffer(bytearray(view[:n]),
                                                                    dtype=self._buf.dtype)
            self._fill += n
            view = view[n:]
            if self._fill == self._buf.numel():
                self.flush()

    def flush(self) -> None:
        if self._fill:
            self._emit(self._buf[:self._fill])
            self._fill = 0


class _DeviceReader:
    """File-like view of device memory for a streamed PUT, read D2H in
    ``slot``-sized pieces. Carries a length so requests sends
    Content-Length (the registry, like S3, takes identity bodies, not
    chunked transfer encoding)."""

    def __init__(self, engine, ptr: int, size: int, slot: int):
        self._engine, self._ptr, self._slot = engine, ptr, slot
        self.len = size
        self._off = 0
        self._buf = b""

    def read(self, n=-1):
        size = self.len
        if n is None or n < 0:
            n = size - self._off + len(self._buf)
        while len(self._buf) < n and self._off < size:
            take = min(self._slot, size - self._off)
            self._buf += self._engine.read_device(self._ptr + self._off, take)
            self._off += take
        out, self._buf = self._buf[:n], self._buf[n:]
        return out


class _Landing(NamedTuple):
    """One located blob on its way into ``tensor``; ``cs`` is the chunk size
    of its leaves (``rules.leaf_chunk_size``)."""

    repository: str
    desc: types.Descriptor
    tensor: object
    url: str
    headers: Dict[str, str]
    cs: int
    verify: bool
    plan_entry: object

    @property
    def ptr(self) -> int:
        return self.tensor.data_ptr()


# One digested device blob ready for upload: `digest` is the main digest, `root`
# the chunked one, `notes` the annotations beyond the chunk ones. `keep` holds the
# compressed tensor alive until pushed (None: `ptr` is the source tensor's memory).
_PushBlob = namedtuple("_PushBlob", "name ptr size media_type digest root leaves notes keep")


class GpuClient:
    """Per-device transfer client. One GpuEngine (pinned ring + streams +
    hash stream) per instance."""

    PART_RETRIES = 3  # reference: pkg/client/extension_s3.go:133-148
    ZSTD_WAVE_CAP = 64 << 30  # raw bytes per batched-decode wave

    def __init__(self, registry: str, authorization: str = "", device: int = 0,
                 num_slots: int = DEFAULT_NUM_SLOTS, slot_bytes: int = DEFAULT_SLOT_BYTES,
                 num_conns: int = DEFAULT_NUM_CONNS, dedup: bool = False):
        core = _core()
        if not core.hip_available():
            raise er.ModelxError(er.ErrCode.INTERNAL, "no HIP device visible")
        self.remote = RegistryClient(registry, authorization)
        self.device = device
        self.num_conns = num_conns
        self.slot_bytes = slot_bytes
        self.engine = core.GpuEngine(device=device, num_slots=num_slots,
                                     slot_bytes=slot_bytes, num_streams=4)
        self.last_stats: List[dict] = []
        # cross-blob chunk dedup (SURVEY.md §2.2 chunk_verify_dedup): an
        # HBM-resident hash table (core/hip/dedup.hip) maps leaf digests to
        # resident chunk addresses; a pull probes it on-device and gathers
        # hits D2D at HBM bandwidth instead of re-fetching from S3. Opt-in:
        # registered tensors are kept alive in _dedup_tensors.
        self.dedup = dedup
        self._dedup_tensors: List[object] = []
        self._dedup_registered = False

    # ----------------------------------------------------------- helpers --

    def _sync_producers(self) -> None:
        """Synchronize torch's streams before the engine READS a
        user-provided tensor. The engine runs on its own non-blocking HIP
        streams, which never implicitly order against torch's default
        stream — without this, digesting/pushing a tensor whose producing
        kernel (randint/repeat/copy) is still in flight reads torn bytes
        and permanently stores content that matches no digest. (Observed
        on hardware with 2.4 GiB generated tensors; small tensors usually
        win the race, which is what made it look intermittent.)"""
        import torch

        torch.cuda.synchronize(self.device)

    def _device(self, nbytes: int) -> "torch.Tensor":
        """Uninitialised uint8 bytes in this client's HBM; never a null pointer."""
        import torch

        return torch.empty(max(nbytes, 1), dtype=torch.uint8,
                           device=f"cuda:{self.device}")[:nbytes]

    def _stat(self, phase: str, nbytes: int, t0: Optional[float] = None, **more) -> dict:
        """Append one ``last_stats`` entry; ``seconds`` since ``t0`` if given."""
        entry = {"phase": phase, "bytes": nbytes, **more}
        if t0 is not None:
            entry["seconds"] = time.monotonic() - t0
        self.last_stats.append(entry)
        return entry

    def _verify_device_digest(self, ptr: int, size: int, desc: types.Descriptor) -> None:
        """GPU chunk-digest the landed buffer and compare against the
        descriptor's chunked digest (or its chunk annotation)."""
        target = rules.chunked_target(desc)
        if target is None:
            # canonical sha256 only (no chunk annotation): one sequential
            # chain — D2H through the pinned ring + SHA-NI on CPU, the fast
            # path for a single chain (a GPU lane is ~4x slower)
            got = "sha256:" + self.engine.sha256_canonical_device(ptr, size).hex()
            if got != desc.digest:
                raise er.ModelxError(er.ErrCode.DIGEST_INVALID,
                                     f"GPU digest mismatch for {desc.name}: {got}")
            return
        expect, cs = target
        leaves = self.engine.sha256_chunk_leaves(ptr, size, cs)
        got = dg.root_from_leaf_bytes(leaves, cs, size)
        if got != expect:
            raise er.ModelxError(er.ErrCode.DIGEST_INVALID,
                                 f"GPU chunk digest mismatch for {desc.name}: {got} != {expect}")

    def _download_url(self, repository: str,
                      desc: types.Descriptor) -> Optional[Tuple[str, Dict[str, str]]]:
        """Presigned GET URL for a blob, or None when the registry runs
        without --enable-redirect (the caller degrades to streaming the
        bytes through the registry, pull.go:206-215 semantics)."""
        loc = self.remote.get_blob_location(repository, desc, "download")
        if loc is None:
            return None
        parts = loc.properties.get("parts") or []
        if not parts:
            raise er.ModelxError(er.ErrCode.UNKNOWN, "empty location parts")
        return parts[0]["url"], _signed_headers(parts[0])

    @staticmethod
    def _plan_url(entry) -> Optional[Tuple[str, Dict[str, str]]]:
        """(url, headers) from a pull-plan blob entry, if it has one."""
        loc = (entry or {}).get("location") or {}
        parts = (loc.get("properties") or {}).get("parts") or []
        if not parts:
            return None
        return parts[0]["url"], _signed_headers(parts[0])

    @staticmethod
    def _plan_leaves(entry, desc: types.Descriptor) -> Optional[bytes]:
        """Inlined leaves from a pull-plan entry, VERIFIED against the
        descriptor's leaves-blob digest (the plan is untrusted input)."""
        b64 = (entry or {}).get("leaves64")
        if not b64:
            return None
        try:
            data = base64.b64decode(b64)
        except Exception:
            return None
        ld = desc.annotations.get(types.ANNOTATION_LEAVES_BLOB, "")
        if not ld or dg.sha256_digest(data) != ld:
            return None
        return data

    def _expected_leaves(self, repository: str, desc: types.Descriptor) -> Optional[bytes]:
        """Fetch the leaves sidecar blob (per-chunk SHA-256 array) if the
        descriptor carries one."""
        ld = desc.annotations.get(types.ANNOTATION_LEAVES_BLOB, "")
        if not ld:
            return None
        try:
            data = b"".join(self.remote.get_blob_content(repository, ld))
        except er.ModelxError:
            return None
        if dg.sha256_digest(data) != ld:
            return None
        return data

    def _usable_leaves(self, job: _Landing) -> Optional[bytes]:
        """The blob's expected leaves from the plan or the sidecar. The
        sidecar's own digest says nothing about its length: leaves that do
        not fit (size, cs) count as no leaves at all, so the pull degrades
        to the full, digest-verified fetch."""
        lv = (self._plan_leaves(job.plan_entry, job.desc)
              or self._expected_leaves(job.repository, job.desc))
        return lv if lv is not None and leaves_usable(lv, job.desc.size, job.cs) else None

    @staticmethod
    def _bad_chunk_ranges(got: bytes, expect: bytes, chunk_size: int,
                          size: int) -> List[Tuple[int, int]]:
        """Contiguous (offset, length) ranges of mismatching chunks, all
        inside ``[0, size)``. Leaves that are not the array of a
        ``size``-byte blob at ``chunk_size`` say nothing about any chunk:
        the whole blob is then bad."""
        if not leaves_usable(expect, size, chunk_size) or len(got) != len(expect):
            return [(0, size)] if size > 0 else []
        if size == 0:
            return []  # the one leaf of an empty blob covers no bytes
        n = len(expect) // 32
        bad = [i for i in range(n) if got[i * 32 : (i + 1) * 32] != expect[i * 32 : (i + 1) * 32]]
        ranges: List[Tuple[int, int]] = []
        for i in bad:
            off = i * chunk_size
            ln = min(chunk_size, size - off)
            if ranges and ranges[-1][0] + ranges[-1][1] == off:
                ranges[-1] = (ranges[-1][0], ranges[-1][1] + ln)
            else:
                ranges.append((off, ln))
        return ranges

    def _fetch_ranges(self, url: str, headers: Dict[str, str], ptr: int,
                      ranges: List[Tuple[int, int]]) -> int:
        if not ranges:
            return 0
        self.engine.pull_ranges_to_device(url, headers, ranges, ptr, self.num_conns)
        return sum(ln for _, ln in ranges)

    # ------------------------------------------------------ chunk dedup --

    def register_chunks(self, tensor, leaves: bytes, chunk_size: int,
                        size: Optional[int] = None) -> None:
        """Add a blob's chunks to the HBM dedup table (dedup.hip insert
        kernel); keeps the tensor alive while registered. ``size`` is the
        blob's length when the tensor is larger than the blob it holds."""
        if not self.dedup:
            return
        nbytes = tensor.numel() * tensor.element_size()
        if size is None:
            size = nbytes
        if size > nbytes or not leaves_usable(leaves, size, chunk_size):
            return  # would index chunks the tensor does not have
        self._dedup_tensors.append(tensor)
        self.engine.dedup_register(leaves, tensor.data_ptr(), chunk_size, size)
        self._dedup_registered = True

    def clear_chunk_index(self) -> None:
        if self._dedup_registered:
            self.engine.dedup_reset(0)
        self._dedup_tensors.clear()
        self._dedup_registered = False

    # ---------------------------------------------------- landing a blob --

    def pull_blob_to_device(self, repository: str, desc: types.Descriptor,
                            tensor=None, verify: bool = True,
                            resume: bool = False, plan_entry=None) -> "torch.Tensor":
        """Land a blob in HBM. With ``resume=True`` and an existing tensor,
        only chunks whose GPU hash mismatches the expected leaves are fetched
        (chunk-level resume/dedup — the reference resumes at whole-blob
        granularity only, pull.go:115-124). On digest mismatch after a full
        pull, only the BAD chunks are refetched (SURVEY.md §5 fault-injection
        requirement: a flipped byte must re-fetch the chunk, not the blob).

        The strategies are tried in order; one that does not apply (no
        usable leaves, nothing resident) returns None and the next runs."""
        had_tensor = tensor is not None
        if tensor is None:
            tensor = self._device(desc.size)
        assert tensor.numel() >= desc.size
        located = self._plan_url(plan_entry) or self._download_url(repository, desc)
        if located is None:
            return self._land_via_registry(repository, desc, tensor, verify)
        job = _Landing(repository, desc, tensor, *located,
                       rules.leaf_chunk_size(desc), verify, plan_entry)
        out = None
        if resume and had_tensor:
            out = self._land_resume(job)
        if out is None and self.dedup and self._dedup_registered:
            out = self._land_dedup(job)
        if out is None:
            out = self._land_transfer(job)
        return out

    def _stream_via_registry(self, repository: str, desc: types.Descriptor, tensor) -> None:
        """Stream the blob through the registry API into HBM in bounded
        pinned pieces. Slow (single stream, extra hop)."""
        t0 = time.monotonic()
        off = 0

        def land(piece):
            nonlocal off
            tensor[off:off + piece.numel()].copy_(piece, non_blocking=False)
            off += piece.numel()

        staging = _PinnedStaging(self.slot_bytes, land)
        for chunk in self.remote.get_blob_content(repository, desc.digest):
            staging.feed(chunk)
        staging.flush()
        if off != desc.size:
            raise er.ModelxError(er.ErrCode.UNKNOWN,
                                 f"registry stream truncated: {off} != {desc.size}")
        self._stat("pull-registry-stream", off, t0)

    def _land_via_registry(self, repository: str, desc: types.Descriptor, tensor,
                           verify: bool) -> "torch.Tensor":
        """Landing for a redirect-less registry: degrades to the registry
        stream instead of failing. A digest mismatch is streamed once more."""
        self._stream_via_registry(repository, desc, tensor)
        if verify:
            try:
                self._verify_device_digest(tensor.data_ptr(), desc.size, desc)
            except er.ModelxError:
                self._stream_via_registry(repository, desc, tensor)
                self._verify_device_digest(tensor.data_ptr(), desc.size, desc)
        return tensor

    def _land_resume(self, job: _Landing) -> Optional["torch.Tensor"]:
        """Fetch only the chunks of the caller's tensor that differ from the
        expected leaves. None without usable leaves."""
        expect = self._usable_leaves(job)
        if expect is None:
            return None
        desc = job.desc
        got = self.engine.sha256_chunk_leaves(job.ptr, desc.size, job.cs)
        ranges = self._bad_chunk_ranges(got, expect, job.cs, desc.size)
        fetched = self._fetch_ranges(job.url, job.headers, job.ptr, ranges)
        self._stat("pull-resume", fetched, skipped=desc.size - fetched)
        if job.verify:
            self._verify_device_digest(job.ptr, desc.size, desc)
        return job.tensor

    def _land_dedup(self, job: _Landing) -> Optional["torch.Tensor"]:
        """Cross-blob dedup: probe the HBM table and gather resident chunks
        D2D, fetch only the rest (SURVEY.md §2.2 chunk_verify_dedup; the
        reference dedups at whole-blob granularity only, push.go:169-177).
        None without usable leaves or when no chunk is resident."""
        expect = self._usable_leaves(job)
        if expect is None:
            return None
        desc, cs = job.desc, job.cs
        t0 = time.monotonic()
        missing, dedup_bytes = self.engine.dedup_pull(expect, job.ptr, cs, desc.size)
        if not dedup_bytes:
            return None
        fetched = self._fetch_ranges(job.url, job.headers, job.ptr, missing)
        stats = self._stat("pull-dedup", fetched, t0, dedup_bytes=dedup_bytes)
        if job.verify:
            # verify against the leaves; refetch any bad chunk (a
            # stale/poisoned index entry must degrade to a fetch, never to
            # a failure)
            got = self.engine.sha256_chunk_leaves(job.ptr, desc.size, cs)
            bad = self._bad_chunk_ranges(got, expect, cs, desc.size)
            if bad:
                fetched_offs = {o for off, ln in missing for o in range(off, off + ln, cs)}
                bad_offs = [o for off, ln in bad for o in range(off, off + ln, cs)]
                refetched = sum(o in fetched_offs for o in bad_offs)
                kinds = {"gathered": len(bad_offs) - refetched, "fetched": refetched}
                print(f"modelx: dedup refetch {desc.name}: "
                      f"{len(bad)} ranges, chunks by origin {kinds}", file=sys.stderr)
                stats["refetched_bytes"] = self._fetch_ranges(job.url, job.headers,
                                                              job.ptr, bad)
                stats["refetched_ranges"] = len(bad)
                got = self.engine.sha256_chunk_leaves(job.ptr, desc.size, cs)
            root = dg.root_from_leaf_bytes(got, cs, desc.size)
            target = rules.chunked_target(desc)
            if target and root != target[0]:
                raise er.ModelxError(er.ErrCode.DIGEST_INVALID,
                                     f"GPU chunk digest mismatch for {desc.name}: {root}")
        self.register_chunks(job.tensor, expect, cs, desc.size)
        return job.tensor

    def _land_transfer(self, job: _Landing) -> "torch.Tensor":
        """Full transfer, then verify. Where the slots cover whole chunks the
        chunks are hashed on each slot's stream right behind its H2D copy,
        so verification overlaps the transfer; a streamed root that misses
        the digest goes on to the full verify and the chunk refetch."""
        desc, cs = job.desc, job.cs
        target = rules.chunked_target(desc)
        t0 = time.monotonic()
        if job.verify and target and self.slot_bytes % cs == 0 and desc.size > 0:
            stats, leaves = self.engine.pull_to_device_hashed(
                job.url, job.headers, desc.size, job.ptr, self.num_conns, cs)
            stats.update(name=desc.name, phase="pull-transfer-hashed")
            self.last_stats.append(stats)
            if dg.root_from_leaf_bytes(leaves, cs, desc.size) == target[0]:
                self.last_stats.append({"phase": "pull-verify", "bytes": desc.size,
                                        "seconds": time.monotonic() - t0 - stats["seconds"]})
                self.register_chunks(job.tensor, leaves, cs, desc.size)
                return job.tensor
        else:
            stats = self.engine.pull_to_device(job.url, job.headers, desc.size, job.ptr,
                                               self.num_conns)
            stats.update(name=desc.name, phase="pull-transfer")
            self.last_stats.append(stats)
            if not job.verify:
                return job.tensor
        t0 = time.monotonic()
        try:
            self._verify_device_digest(job.ptr, desc.size, desc)
        except er.ModelxError as first_err:
            self._refetch_bad_chunks(job, first_err)
        self._stat("pull-verify", desc.size, t0)
        return job.tensor

    def _refetch_bad_chunks(self, job: _Landing, first_err: er.ModelxError) -> None:
        """Chunk-level refetch before giving up on a landed blob whose
        digest check raised ``first_err``: fetch the chunks that differ from
        the leaves sidecar and verify again."""
        desc = job.desc

        def failed(err, path):
            return er.ModelxError(
                er.ErrCode.DIGEST_INVALID,
                f"{err.message} [size={desc.size} media={desc.media_type} path={path}]")

        expect = self._usable_leaves(job)
        if expect is None:
            raise failed(first_err, "no-leaves-sidecar") from first_err
        got = self.engine.sha256_chunk_leaves(job.ptr, desc.size, job.cs)
        ranges = self._bad_chunk_ranges(got, expect, job.cs, desc.size)
        if not ranges:
            # landed leaves MATCH the sidecar yet the root digest differs:
            # the sidecar and the descriptor disagree — a metadata-level
            # inconsistency, not a transfer corruption
            raise failed(first_err, "leaves-match-but-root-differs") from first_err
        self._fetch_ranges(job.url, job.headers, job.ptr, ranges)
        self._stat("pull-chunk-refetch", sum(r[1] for r in ranges))
        try:
            self._verify_device_digest(job.ptr, desc.size, desc)
        except er.ModelxError as second_err:
            raise failed(second_err,
                         f"refetch-did-not-fix ranges={len(ranges)}") from second_err

    # -------------------------------------------------------- +zstd blobs --

    @staticmethod
    def _sized_output(desc: types.Descriptor, out, got: int, raw_size: int):
        """The decoded bytes of ``out``, which must be the annotated size."""
        if got != raw_size:
            raise er.ModelxError(er.ErrCode.DIGEST_INVALID,
                                 f"zstd size mismatch for {desc.name}: {got} != {raw_size}")
        return out[:got]

    @staticmethod
    def _check_raw_digest(desc: types.Descriptor, leaves: bytes, target, size: int) -> None:
        digest, cs = target
        if dg.root_from_leaf_bytes(leaves, cs, size) != digest:
            raise er.ModelxError(er.ErrCode.DIGEST_INVALID,
                                 f"uncompressed digest mismatch for {desc.name}")

    @staticmethod
    def _report_decode_failure(desc: types.Descriptor, comp, err: Exception) -> None:
        """Diagnostic before the one retry of a failed decode: persist the
        (digest-verified) compressed bytes so the failure is analyzable
        offline — a second identical failure is deterministic (bad stored
        frame), a pass means a device-side race to hunt. Opt-in via
        MODELX_ZSTD_DUMP=<dir>: the blob can be gigabytes, so never write it
        into an arbitrary cwd by default."""
        dump_dir = os.environ.get("MODELX_ZSTD_DUMP", "")
        if not dump_dir:
            print(f"modelx: zstd decode failed ({err}); retrying once "
                  "(set MODELX_ZSTD_DUMP=<dir> to keep the blob)", file=sys.stderr)
            return
        try:
            os.makedirs(dump_dir, exist_ok=True)
            path = os.path.join(
                dump_dir, f"zstd_decode_fail_{desc.digest.split(':')[-1][:12]}.zst")
            with open(path, "wb") as f:
                f.write(bytes(comp[: desc.size].cpu().numpy().tobytes()))
            print(f"modelx: zstd decode failed ({err}); dumped {path}; retrying once",
                  file=sys.stderr)
        except Exception:
            pass

    def _merge_byte_planes(self, jobs) -> List["torch.Tensor"]:
        """Planar tensors back to interleaved bytes: jobs = [(planar uint8
        tensor, (E, G))]; ONE engine call (one stream sync) for the whole
        list, one ``pull-byte-planes-merge`` entry in ``last_stats``."""
        t0 = time.monotonic()
        outs = [self._device(p.numel()) for p, _ in jobs]
        self.engine.byte_planes(
            [(p.data_ptr(), o.data_ptr(), p.numel(), elem, group)
             for (p, (elem, group)), o in zip(jobs, outs)], True)
        self._stat("pull-byte-planes-merge", sum(p.numel() for p, _ in jobs), t0,
                   blobs=len(jobs))
        return outs

    def pull_zstd_blob_to_device(self, repository: str, desc: types.Descriptor,
                                 verify: bool = True, plan_entry=None) -> "torch.Tensor":
        """Pull a +zstd blob: land the compressed stream in HBM (streaming
        SHA-256 verify over the stored bytes), decode every frame in its own
        workgroup (core/hip/zstd.hip), then GPU-verify the uncompressed
        chunked digest from the raw-digest annotation. The whole path —
        transfer, hash, inflate, re-hash — never leaves the GPU.

        A blob with the byte-planes annotation decodes into a temporary,
        the merge kernel (core/hip/byteplane.hip) rebuilds the interleaved
        bytes, and only those are checked against the raw digest. A
        malformed annotation is refused before anything is fetched."""
        planes = rules.byte_planes(desc)
        comp = self.pull_blob_to_device(repository, desc, verify=verify, plan_entry=plan_entry)
        raw_size = rules.raw_size(desc)
        out = self._device(raw_size)

        def decode():
            return self.engine.zstd_decompress_device(comp.data_ptr(), desc.size,
                                                      out.data_ptr(), out.numel())

        t0 = time.monotonic()
        try:
            got = decode()
        except RuntimeError as e:
            self._report_decode_failure(desc, comp, e)
            got = decode()
        self._stat("pull-zstd-decompress", got, t0)
        out = self._sized_output(desc, out, got, raw_size)
        if planes:
            del comp  # the planar temporary and the result are the residents now
            out = self._merge_byte_planes([(out, planes)])[0]
        target = rules.raw_target(desc)
        if verify and target:
            leaves = self.engine.sha256_chunk_leaves(out.data_ptr(), got, target[1])
            self._check_raw_digest(desc, leaves, target, got)
        return out

    def _pull_zstd_batched(self, repository: str, jobs, verify: bool,
                           parallel: int) -> Dict[object, "torch.Tensor"]:
        """Many +zstd blobs in one orchestration pass: compressed bytes land
        (and stream-hash-verify) per blob, then ONE batched decode call and
        ONE batched leaf-digest call cover the whole set — the per-blob
        footer/table/sync round trips were the measured config-5 limiter
        (profiles/bench_shapes.md: 4.1 GiB/s effective vs 240+ GiB/s
        kernel). jobs = [(key, desc, plan_entry)]; returns {key: tensor}.

        Waves are capped at ~64 GiB of raw output so compressed+raw
        residency stays bounded on very large sets."""
        # byte-plane annotations, parsed (and a malformed one refused) before
        # anything is fetched; planar blobs decode into a temporary and ONE
        # merge call per batch rebuilds the interleaved bytes
        plane_of = {key: rules.byte_planes(desc) for key, desc, _ in jobs}
        waves = rules.zstd_waves(jobs, self.ZSTD_WAVE_CAP)
        if len(waves) > 1:
            outs: Dict[object, "torch.Tensor"] = {}
            for wave in waves:
                outs.update(self._pull_zstd_batched(repository, wave, verify, parallel))
            return outs

        comp = dict(_map(lambda job: (job[0], self.pull_blob_to_device(
            repository, job[1], verify=verify, plan_entry=job[2])), jobs, parallel))
        outs, items, raw_sizes = {}, [], []
        for key, desc, _ in jobs:
            raw_sizes.append(rules.raw_size(desc))
            o = outs[key] = self._device(raw_sizes[-1])
            items.append((comp[key].data_ptr(), desc.size, o.data_ptr(), o.numel()))
        t0 = time.monotonic()
        sizes = self.engine.zstd_decompress_many(items)
        self._stat("pull-zstd-decompress-batched", sum(sizes), t0, blobs=len(items))
        for (key, desc, _), got, raw_size in zip(jobs, sizes, raw_sizes):
            outs[key] = self._sized_output(desc, outs[key], got, raw_size)
        del comp, items  # decoded: the compressed tensors can go
        planar = [key for key, _, _ in jobs if plane_of[key]]
        if planar:
            # ONE merge call for the batch, before the raw digests are
            # checked: those describe the interleaved bytes
            merged = self._merge_byte_planes([(outs[key], plane_of[key]) for key in planar])
            outs.update(zip(planar, merged))
        checks = [(desc, outs[key], rules.raw_target(desc)) for key, desc, _ in jobs]
        checks = [c for c in checks if verify and c[2]]
        if checks:
            t0 = time.monotonic()
            leaves_list = self.engine.sha256_chunk_leaves_many(
                [(o.data_ptr(), o.numel(), target[1]) for _, o, target in checks])
            for (desc, o, target), leaves in zip(checks, leaves_list):
                self._check_raw_digest(desc, leaves, target, o.numel())
            self._stat("pull-zstd-raw-verify-batched", sum(c[1].numel() for c in checks), t0)
        return outs

    # ----------------------------------------------------- whole versions --

    @staticmethod
    def _manifest_of(plan, fetch_manifest) -> Tuple[types.Manifest, dict]:
        """(manifest, per-digest plan entries) from a pull plan; without a
        usable plan the manifest is fetched and there are no entries."""
        if plan and plan.get("manifest"):
            return types.Manifest.from_dict(plan["manifest"]), plan.get("blobs") or {}
        return fetch_manifest(), {}

    def pull_to_gpu(self, repository: str, version: str = "",
                    verify: bool = True, parallel: int = 1,
                    expand_dirs: bool = False) -> Dict[str, "torch.Tensor"]:
        """Pull every file blob of a manifest into HBM. Directory blobs are
        landed as raw archive bytes under their blob name; with
        ``expand_dirs=True`` plain-tar and tar+gz directory blobs go through
        ``pull_dir_to_gpu`` instead and their members appear under the
        archive names (``"shards/layer0/w.bin"``), the blob's own name not.
        ``parallel`` > 1 pulls blobs concurrently (reentrant engine; right
        for many-shard manifests where per-blob latency would stack).
        Multiple +zstd blobs decode through the batched engine call."""
        # one round trip for manifest + presigns + leaves when the server
        # supports pull plans (measured: the per-blob control plane
        # dominated many-small-blob indexes — docs/roadmap.md)
        manifest, plan_blobs = self._manifest_of(
            self.remote.get_pull_plan(repository, version),
            lambda: self.remote.get_manifest(repository, version))
        zstd_descs, dir_descs, plain_descs = rules.split_payloads(
            rules.payload_descriptors(manifest), expand_dirs)

        out: Dict[str, "torch.Tensor"] = {}
        if len(zstd_descs) > 1:
            jobs = [(d.name, d, plan_blobs.get(d.digest)) for d in zstd_descs]
            out.update(self._pull_zstd_batched(repository, jobs, verify, parallel))
            zstd_descs = []

        def one(desc) -> Dict[str, "torch.Tensor"]:
            entry = plan_blobs.get(desc.digest)
            if expand_dirs and desc.media_type in rules.DIR_MEDIA_TYPES:
                return self.pull_dir_to_gpu(repository, desc, verify=verify, plan_entry=entry)
            pull = (self.pull_zstd_blob_to_device
                    if desc.media_type == types.MEDIA_TYPE_MODEL_FILE_ZSTD
                    else self.pull_blob_to_device)
            return {desc.name: pull(repository, desc, verify=verify, plan_entry=entry)}

        # file blobs and directory blobs share one pool
        for part in _map(one, plain_descs + zstd_descs + dir_descs, parallel):
            clash = sorted(set(part) & set(out)) if dir_descs else []
            if clash:
                raise er.ModelxError(er.ErrCode.MANIFEST_INVALID,
                                     f"expand_dirs: {clash[0]!r} is named by more than one blob")
            out.update(part)
        return out

    def pull_many(self, repository: str, versions, parallel: int = 6,
                  verify: bool = True) -> Dict[str, Dict[str, "torch.Tensor"]]:
        """Pull several versions concurrently. The native engine's pull path
        is reentrant (per-call range state, shared pinned-slot pool), so
        many small blobs overlap their HTTP round-trips — the limiter for
        mixed indexes (BASELINE config 5) is per-blob latency, not
        bandwidth. All +zstd blobs ACROSS the versions decode through one
        batched engine call (config 5 stores one small blob per version, so
        per-version batching alone would never engage)."""
        # one POST for all versions' plans when the server supports it
        try:
            batch = self.remote.get_pull_plans(repository, versions)
        except Exception:
            batch = None

        def info(v):
            plan = (batch or {}).get(v) or self.remote.get_pull_plan(repository, v)
            return self._manifest_of(plan, lambda: self.remote.get_manifest(repository, v))

        infos = _map(info, versions, parallel)
        results: Dict[str, Dict[str, "torch.Tensor"]] = {v: {} for v in versions}
        zstd_jobs = []
        plain_jobs = []
        for v, (manifest, plan_blobs) in zip(versions, infos):
            zstd_descs, _, plain_descs = rules.split_payloads(
                rules.payload_descriptors(manifest))
            zstd_jobs += [((v, d.name), d, plan_blobs.get(d.digest)) for d in zstd_descs]
            plain_jobs += [(v, d, plan_blobs.get(d.digest)) for d in plain_descs]
        if len(zstd_jobs) > 1:
            for (v, name), t in self._pull_zstd_batched(repository, zstd_jobs,
                                                        verify, parallel).items():
                results[v][name] = t
        elif zstd_jobs:
            (v, name), d, entry = zstd_jobs[0]
            results[v][name] = self.pull_zstd_blob_to_device(repository, d, verify=verify,
                                                             plan_entry=entry)

        def one(job):
            v, d, entry = job
            return v, d.name, self.pull_blob_to_device(repository, d, verify=verify,
                                                       plan_entry=entry)

        for v, name, t in _map(one, plain_jobs, parallel):
            results[v][name] = t
        return results

    # -------------------------------------------------- directory blobs --

    def _stream_targz_to_device(self, repository: str, desc: types.Descriptor):
        """Streamed landing of a tar.gz compat blob (reference
        pull.go:184-203 pipes download∥extract): presigned GET (or registry
        stream) → zlib inflate → bounded pinned staging → HBM, with the
        STORED bytes digest-verified on the fly — host memory stays
        O(staging), never O(blob). gzip is inherently sequential, so the
        inflate runs on CPU; the GPU-native directory format
        (MEDIA_TYPE_MODEL_DIRECTORY_TAR) skips this path entirely."""
        import torch

        t0 = time.monotonic()
        located = self._download_url(repository, desc)
        if located is not None:
            import requests

            url, headers = located
            resp = requests.get(url, headers=headers, stream=True, verify=_tls_verify())
            resp.raise_for_status()
            source = resp.iter_content(chunk_size=1 << 20)
        else:
            source = self.remote.get_blob_content(repository, desc.digest)

        # verify the stored (compressed) bytes while streaming
        chunk_note = rules.chunk_digest_note(desc)
        cs = _annotated_chunk_size(desc) or dg.DEFAULT_CHUNK_SIZE
        hasher = dg.StreamingDigester(chunk_size=cs)

        inflater = zlib.decompressobj(16 + zlib.MAX_WBITS)  # gzip framing
        pieces: List["torch.Tensor"] = []
        staging = _PinnedStaging(
            self.slot_bytes, lambda piece: pieces.append(piece.to(f"cuda:{self.device}")))
        for piece in source:
            hasher.update(piece)
            staging.feed(inflater.decompress(piece))
        staging.feed(inflater.flush())
        staging.flush()
        if hasher.total != desc.size:
            raise er.ModelxError(er.ErrCode.UNKNOWN,
                                 f"tar.gz stream truncated: {hasher.total} != {desc.size}")
        if desc.digest and desc.digest not in (hasher.canonical_digest(),
                                               hasher.chunk_digest()) and \
                (not chunk_note or chunk_note != hasher.chunk_digest()):
            raise er.ModelxError(er.ErrCode.DIGEST_INVALID,
                                 f"stored digest mismatch for {desc.name}")
        if not pieces:
            pieces = [torch.empty(0, dtype=torch.uint8, device=f"cuda:{self.device}")]
        archive = pieces[0] if len(pieces) == 1 else torch.cat(pieces)
        tar_len = archive.numel()
        self._stat("pull-targz-stream", tar_len, t0, stored_bytes=desc.size)
        return archive, tar_len

    def pull_dir_to_gpu(self, repository: str, desc: types.Descriptor, verify: bool = True,
                        plan_entry=None) -> Dict[str, "torch.Tensor"]:
        """Land a directory blob and scatter its files into per-file HBM
        tensors with the CDNA4 tar kernels (core/hip/tar.hip). Plain-tar
        blobs (MEDIA_TYPE_MODEL_DIRECTORY_TAR) stay on-GPU end to end;
        tar+gz compat blobs are inflated on CPU first (gzip is sequential —
        the GPU-native path is the plain-tar format). ``verify`` and
        ``plan_entry`` are those of ``pull_blob_to_device`` and apply to
        plain-tar blobs; the tar+gz stream always digests the stored bytes
        as it goes and locates the blob itself."""
        if desc.media_type == types.MEDIA_TYPE_MODEL_DIRECTORY_TAR:
            archive = self.pull_blob_to_device(repository, desc, verify=verify,
                                               plan_entry=plan_entry)
            tar_len = desc.size
        elif desc.media_type == types.MEDIA_TYPE_MODEL_DIRECTORY_TARGZ:
            archive, tar_len = self._stream_targz_to_device(repository, desc)
        else:
            raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                                 f"not a directory blob: {desc.media_type}")
        entries = self.engine.tar_index(archive.data_ptr(), tar_len)
        out: Dict[str, "torch.Tensor"] = {}
        segs = []
        for e in entries:
            t = out[e["name"]] = self._device(int(e["size"]))
            if e["size"]:
                segs.append((int(e["offset"]), t.data_ptr(), int(e["size"])))
        if segs:
            self.engine.tar_scatter(archive.data_ptr(), segs)
        return out

    def pack_dir_on_gpu(self, name: str, files: Dict[str, "torch.Tensor"]) -> "torch.Tensor":
        """Pack device tensors into one plain-tar archive in HBM (the pack
        kernel of core/hip/tar.hip) — the push-side inverse of
        ``pull_dir_to_gpu``. Members are ``f"{name}/{relpath}"`` sorted by
        name, with deterministic headers, so equal inputs give byte-equal
        archives. Tensors must live on this client's device and be
        contiguous (any dtype: the member is the tensor's raw bytes)."""
        import torch

        members = []
        for rel in sorted(files):
            t = files[rel]
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name}/{rel}: not a torch.Tensor")
            if not t.is_cuda or t.device.index != self.device:
                raise ValueError(f"{name}/{rel}: tensor is on {t.device}, "
                                 f"not on cuda:{self.device}")
            if not t.is_contiguous():
                raise ValueError(f"{name}/{rel}: tensor is not contiguous")
            members.append((f"{name}/{rel}", t.data_ptr(), t.numel() * t.element_size()))
        # names and sizes are validated here, before any device work
        total = _core().tar_pack_layout([(n, s) for n, _, s in members])["total"]
        self._sync_producers()
        t0 = time.monotonic()
        archive = torch.empty(total, dtype=torch.uint8, device=f"cuda:{self.device}")
        # `files` keeps every source tensor alive: tar_pack returns only
        # after its stream has synchronized
        packed = self.engine.tar_pack(archive.data_ptr(), total, members)
        assert packed == total
        self._stat("gpu-tar-pack", total, t0, members=len(members))
        return archive

    # -------------------------------------------------------------- push --

    def digest_device_blob(self, ptr: int, size: int,
                           chunk_size: int = DEFAULT_GPU_CHUNK) -> Tuple[str, str]:
        """(chunked_digest, chunk_digest_annotation) of device memory."""
        root, _ = self.digest_device_blob_with_leaves(ptr, size, chunk_size)
        return root, root

    def digest_device_blob_with_leaves(self, ptr: int, size: int,
                                       chunk_size: int = DEFAULT_GPU_CHUNK) -> Tuple[str, bytes]:
        self._sync_producers()
        t0 = time.monotonic()
        leaves = self.engine.sha256_chunk_leaves(ptr, size, chunk_size)
        root = dg.root_from_leaf_bytes(leaves, chunk_size, size)
        self._stat("gpu-digest", size, t0)
        return root, leaves

    def _upload_small(self, repository: str, desc: types.Descriptor, data: bytes) -> None:
        loc = self.remote.get_blob_location(repository, desc, "upload")
        if loc is None:
            return self.remote.upload_blob_content(repository, desc, data)
        import requests

        p = (loc.properties.get("parts") or [{}])[0]
        for attempt in range(self.PART_RETRIES):
            try:
                requests.request(p.get("method") or "PUT", p["url"], headers=_signed_headers(p),
                                 data=data, verify=_tls_verify()).raise_for_status()
                return
            except Exception:
                if attempt == self.PART_RETRIES - 1:
                    raise

    def _upload_small_once(self, repository: str, desc: types.Descriptor,
                           data: bytes) -> types.Descriptor:
        """Upload a small host blob unless the registry already has it."""
        if not self.remote.head_blob(repository, desc.digest):
            self._upload_small(repository, desc, data)
        return desc

    def _push_part_retrying(self, part: dict, ptr: int, length: int) -> None:
        """One presigned part from device memory, retried on transport
        failure with a fresh connection (the engine drops broken sockets
        from its pool on error)."""
        for attempt in range(self.PART_RETRIES):
            try:
                self.engine.push_part_from_device(part["url"], part.get("method") or "PUT",
                                                  _signed_headers(part), ptr, length)
                return
            except RuntimeError:
                if attempt == self.PART_RETRIES - 1:
                    raise

    def push_blob_from_device(self, repository: str, desc: types.Descriptor, ptr: int,
                              part_bytes: int = DEFAULT_PART_BYTES,
                              parallel: int = DEFAULT_PUSH_PARALLEL) -> None:
        """Presigned (multi)part upload of device memory. HEAD-dedup first
        (push.go:169-177 semantics)."""
        self._sync_producers()
        t0 = time.monotonic()
        if self.remote.head_blob(repository, desc.digest):
            return
        size = desc.size
        nparts = max(1, (size + part_bytes - 1) // part_bytes)
        extra = {"part-count": str(nparts), "multipart": "true"} if nparts > 1 else None
        loc = self.remote.get_blob_location(repository, desc, "upload", extra=extra)
        if loc is None:
            # redirect-less registry: direct PUT through the registry
            # (reference pushBlob fallback, push.go:196-207), streamed D2H
            # in bounded slot-sized pieces
            reader = _DeviceReader(self.engine, ptr, size, self.slot_bytes)
            self.remote.upload_blob_content(repository, desc, reader if size else b"")
            self._stat("push-registry-stream", size, t0)
            return
        parts = loc.properties.get("parts") or []
        _map(lambda job: self._push_part_retrying(job[0], ptr + job[1][0], job[1][1]),
             zip(parts, rules.part_ranges(size, len(parts))), parallel)
        self._stat("push-upload", size, t0, parts=len(parts))

    def _canonical_digests(self, blobs, phase: str) -> List[str]:
        """Wire-canonical sha256 of [(ptr, size)], one CPU SHA-NI chain per
        blob over D2H, in parallel. Measured (config3, 64x1 GiB): the GPU
        multibuf kernel runs 64 chains in ONE wave at ~16 MiB/s per
        latency-bound lane (1.0 GiB/s aggregate) — a sequential chain has no
        parallelism for the GPU to use, so the SHA-NI units win by an order
        of magnitude across a few threads."""
        t0 = time.monotonic()
        digs = _map(lambda blob: self.engine.sha256_canonical_device(*blob), blobs,
                    min(len(blobs), os.cpu_count() or 8))
        self._stat(phase, sum(s for _, s in blobs), t0)
        return ["sha256:" + d.hex() for d in digs]

    def _digest_batched(self, tensors: Dict[str, "torch.Tensor"], chunk_size: int,
                        digest_mode: str, media_type_of) -> List[_PushBlob]:
        """Many uncompressed blobs (BASELINE config 3 shape): ONE batched
        leaf-digest call for all tensors."""
        self._sync_producers()
        where = [(t.data_ptr(), t.numel() * t.element_size()) for t in tensors.values()]
        t0 = time.monotonic()
        leaves_list = self.engine.sha256_chunk_leaves_many(
            [(p, s, chunk_size) for p, s in where])
        roots = [dg.root_from_leaf_bytes(lv, chunk_size, s)
                 for lv, (_, s) in zip(leaves_list, where)]
        self._stat("gpu-digest-batched", sum(s for _, s in where), t0, blobs=len(where))
        mains = roots
        if digest_mode == "sha256":
            mains = self._canonical_digests(where, "push-canonical-digest-batched")
        return [_PushBlob(name, p, s, media_type_of(name), main, root, lv, {}, None)
                for name, (p, s), main, root, lv in zip(tensors, where, mains, roots,
                                                        leaves_list)]

    def _prepare_zstd(self, t, size: int, chunk_size: int, planes):
        """Compress a tensor on-GPU, byte planes split first where asked.
        Returns (pointer, size, media type, annotations, keep-alive) of the
        stored bytes."""
        self._sync_producers()
        raw_root, _ = self.digest_device_blob_with_leaves(t.data_ptr(), size, chunk_size)
        bound = _core().zstd_compress_bound(size)
        comp = self._device(bound)
        elem = planes
        if planes == "auto":
            elem = t.element_size() if t.element_size() in types.BYTE_PLANES_ELEMS else 0
        src, planar = t, None
        notes = {types.ANNOTATION_RAW_DIGEST: raw_root,
                 types.ANNOTATION_RAW_SIZE: str(size)}
        if elem:
            group = elem * types.BYTE_PLANES_FRAME
            t0 = time.monotonic()
            src = planar = self._device(size)
            self.engine.byte_planes([(t.data_ptr(), planar.data_ptr(), size, elem, group)],
                                    False)
            self._stat("push-byte-planes-split", size, t0)
            notes[types.ANNOTATION_BYTE_PLANES] = types.format_byte_planes(elem, group)
        t0 = time.monotonic()
        comp_size = self.engine.zstd_compress_device(
            src.data_ptr(), size, types.BYTE_PLANES_FRAME, comp.data_ptr(), bound,
            literals_only=bool(elem))
        del src, planar  # the planar copy is freed before the upload
        self._stat("push-zstd-compress", size, t0, compressed=comp_size)
        return comp.data_ptr(), comp_size, types.MEDIA_TYPE_MODEL_FILE_ZSTD, notes, comp

    def _digest_one(self, name: str, t, chunk_size: int, digest_mode: str,
                    media_type: str, compress: str, planes) -> _PushBlob:
        size = t.numel() * t.element_size()
        ptr, notes, keep = t.data_ptr(), {}, None
        if compress == "zstd" and size:
            ptr, size, media_type, notes, keep = self._prepare_zstd(t, size, chunk_size,
                                                                    planes)
        root, leaves = self.digest_device_blob_with_leaves(ptr, size, chunk_size)
        main = root
        if digest_mode == "sha256":
            main, = self._canonical_digests([(ptr, size)], "push-canonical-digest")
        return _PushBlob(name, ptr, size, media_type, main, root, leaves, notes, keep)

    def _upload_blob(self, repository: str, blob: _PushBlob, chunk_size: int,
                     part_bytes: int, now) -> Tuple[types.Descriptor, types.Descriptor]:
        """Upload a digested blob and its leaves sidecar; returns both
        descriptors. The sidecar (32 B per chunk) enables chunk-level
        resume/refetch/dedup on pull; it is listed in the manifest so GC
        keeps it, with its own media type so clients can skip it."""
        leaves_digest = dg.sha256_digest(blob.leaves)
        desc = types.Descriptor(
            name=blob.name, media_type=blob.media_type, digest=blob.digest,
            size=blob.size, modified=now,
            annotations={types.ANNOTATION_CHUNK_DIGEST: blob.root,
                         types.ANNOTATION_CHUNK_SIZE: str(chunk_size),
                         types.ANNOTATION_LEAVES_BLOB: leaves_digest,
                         **blob.notes})
        self.push_blob_from_device(repository, desc, blob.ptr, part_bytes=part_bytes)
        ldesc = types.Descriptor(
            name=blob.name + ".leaves", media_type=types.MEDIA_TYPE_MODEL_LEAVES,
            digest=leaves_digest, size=len(blob.leaves), modified=now)
        return desc, self._upload_small_once(repository, ldesc, blob.leaves)

    def push_from_gpu(self, repository: str, version: str,
                      tensors: Dict[str, "torch.Tensor"], config_yaml: str = "",
                      chunk_size: int = DEFAULT_GPU_CHUNK,
                      part_bytes: int = DEFAULT_PART_BYTES,
                      compress: str = "", digest_mode: str = "chunked",
                      dirs: Optional[Dict[str, Dict[str, "torch.Tensor"]]] = None,
                      planes=0) -> types.Manifest:
        """Digest on GPU → presigned multipart upload → manifest PUT last.
        With ``compress="zstd"`` each tensor is compressed on-GPU into a
        seekable multi-frame zstd blob (core/hip/zstd.hip) first; the
        descriptor digest covers the stored (compressed) bytes and the
        raw-digest/raw-size annotations carry the uncompressed identity.

        ``planes`` (only with ``compress="zstd"``) is 0, an element size 2, 4
        or 8, or ``"auto"`` (each tensor's ``element_size()`` when that is 2,
        4 or 8, otherwise 0). A tensor pushed with planes is split on-GPU
        into one plane per byte position of its element
        (core/hip/byteplane.hip, groups of E × 128 KiB so every zstd frame
        holds one plane), compressed literals-only, and its descriptor gets
        the byte-planes annotation; raw-digest and raw-size still describe
        the tensor's own bytes. Dense float weights store smaller this way
        (profiles/byte_planes.md); mostly-zero tensors store larger, because
        literals-only coding cannot go below one bit per byte. While such a
        tensor is compressed HBM holds the source, its planar copy and the
        compress bound (about three times the tensor); the planar copy is
        freed before the upload.

        ``digest_mode="sha256"`` makes the main descriptor digest the
        wire-canonical plain sha256 (reference push.go:149-161 semantics —
        a stock Go modelx client digest-verifies the pulled blob with zero
        annotations consumed); the chunked digest then travels in the
        chunk-digest annotation, exactly like the CPU push path. The
        canonical chain streams D2H through the pinned ring onto the CPU's
        SHA-NI units. Default ``"chunked"`` keeps the all-GPU digest as the
        main digest (fastest; reference clients lose only verification).

        ``dirs`` maps a directory name to ``{relpath: tensor}``: each entry is
        packed on-GPU into one plain-tar archive (``pack_dir_on_gpu``) and
        pushed as a single MEDIA_TYPE_MODEL_DIRECTORY_TAR blob with the same
        digests, annotations and leaves sidecar as a file blob — many small
        tensors cost one blob's control-plane round trips, not one per
        tensor. ``pull_dir_to_gpu`` and the CPU ``Client.pull`` both read it
        back. Every directory is packed (and so validated) before the first
        upload, so until the push returns HBM holds each directory twice: the
        source tensors and their archive."""
        if compress not in ("", "zstd"):
            raise er.ModelxError(er.ErrCode.UNSUPPORTED, f"unknown compression {compress!r}")
        if digest_mode not in ("chunked", "sha256"):
            raise er.ModelxError(er.ErrCode.UNSUPPORTED, f"unknown digest_mode {digest_mode!r}")
        if planes != "auto":
            check_planes(planes, compress)
        elif compress != "zstd":
            check_planes(2, compress)  # any planes without zstd: UNSUPPORTED
        if dirs:
            if compress:
                raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                                     "dirs cannot be combined with compress: "
                                     "there is no tar+zstd directory media type")
            rules.check_dir_names(tensors, dirs)
            # pack (and thereby validate) every directory before the first
            # upload; the archives then travel as ordinary device blobs
            tensors = dict(tensors)
            for dname, files in dirs.items():
                tensors[dname] = self.pack_dir_on_gpu(dname, files)

        def media_type_of(name: str) -> str:
            return (types.MEDIA_TYPE_MODEL_DIRECTORY_TAR if name in (dirs or ())
                    else types.MEDIA_TYPE_MODEL_FILE)

        manifest = types.Manifest(media_type=types.MEDIA_TYPE_MODEL_MANIFEST_JSON)
        now = datetime.now(timezone.utc)
        # config blob (small, CPU)
        cfg = config_yaml.encode() or b"description: pushed from GPU\n"
        manifest.config = self._upload_small_once(repository, types.Descriptor(
            name="modelx.yaml", media_type=types.MEDIA_TYPE_MODEL_CONFIG_YAML,
            digest=dg.sha256_digest(cfg), size=len(cfg), modified=now), cfg)

        def upload(blob: _PushBlob):
            return self._upload_blob(repository, blob, chunk_size, part_bytes, now)

        def push_one(name: str):
            # digest and upload per tensor, so that a compressed copy lives
            # only until it is pushed
            blob = self._digest_one(name, tensors[name], chunk_size, digest_mode,
                                    media_type_of(name), compress, planes)
            descs = upload(blob)
            if blob.keep is None:
                self.register_chunks(tensors[name], blob.leaves, chunk_size)
            return descs

        if compress == "" and len(tensors) > 1:
            # many-blob fast path: one batched digest, uploads in parallel
            blobs = self._digest_batched(tensors, chunk_size, digest_mode, media_type_of)
            pushed = _map(upload, blobs, DEFAULT_PUSH_PARALLEL)
            for blob in blobs:
                self.register_chunks(tensors[blob.name], blob.leaves, chunk_size)
        else:
            pushed = [push_one(name) for name in tensors]
        for descs in pushed:
            manifest.blobs += descs
        manifest.blobs = types.sort_descriptors_by_name(manifest.blobs)
        self.remote.put_manifest(repository, version or "latest", manifest)
        return manifest
