"""GpuClient's pull and push orchestration, pinned on the CPU.

Every landing and upload strategy of ``modelx_amd/client/gpu.py`` is driven
here without a GPU and without the native extension: the client is built
with ``GpuClient.__new__`` and its two collaborators are functional host
models. Tensors live in host memory (``torch.empty`` loses ``device=`` and
``pin_memory=``), so the engine model does the real work on the bytes behind
each pointer. Each scenario asserts the ordered engine trace, the ordered
remote trace, ``last_stats`` without ``seconds``, the returned bytes and, for
failures, the error code and the bracketed ``path=`` suffix.

Shapes: chunk size 1024 and a 2563-byte blob (three chunks, the last one
partial), ``slot_bytes=4096`` and ``parallel=1`` unless a scenario says
otherwise. Pushes run through thread pools, so their traces are compared as
sorted multisets.

The remote model hands out presigned upload locations for payload blobs
only; the config blob and the leaves sidecars go through
``upload_blob_content``, since the presigned small-blob upload talks HTTP
directly.
"""
import base64
import ctypes
import hashlib
import io
import tarfile
import types as pytypes

import pytest
import torch

from modelx_amd.client import gpu
from modelx_amd.client.gpu import GpuClient
from modelx_amd.wire import digest as dg
from modelx_amd.wire import errors as er
from modelx_amd.wire import types

P = "<ptr>"
CS = 1024
REPO = "r/x"
BLOB = bytes((i * 7 + 3) % 251 for i in range(2563))
OTHER = bytes((i * 13 + 5) % 241 for i in range(2563))
ROOT = dg.chunked_digest(BLOB, CS)
CANON = dg.sha256_digest(BLOB)
LEAVES = b"".join(dg.chunk_leaves(BLOB, CS))
LEAVES_DIGEST = dg.sha256_digest(LEAVES)
ROOT_OTHER = dg.chunked_digest(OTHER, CS)
CANON_OTHER = dg.sha256_digest(OTHER)
LEAVES_OTHER = b"".join(dg.chunk_leaves(OTHER, CS))
LEAVES_OTHER_DIGEST = dg.sha256_digest(LEAVES_OTHER)
THIRD = bytes(b ^ 0x55 for b in BLOB)
CONFIG = b"description: pushed from GPU\n"
CONFIG_DIGEST = dg.sha256_digest(CONFIG)
SIGNED = {"x-sig": "s"}


def byte_planes(src: bytes, elem: int, group: int, merge: bool) -> bytes:
    """core/include/modelx/byteplane_host.hpp, on bytes."""
    out = bytearray(len(src))
    for base in range(0, len(src), group):
        n = min(group, len(src) - base)
        m = n // elem
        for p in range(elem):
            for i in range(m):
                if merge:
                    out[base + i * elem + p] = src[base + p * m + i]
                else:
                    out[base + p * m + i] = src[base + i * elem + p]
        out[base + m * elem:base + n] = src[base + m * elem:base + n]
    return bytes(out)


PLANAR = byte_planes(BLOB, 2, 1024, False)
ROOT_PLANAR = dg.chunked_digest(PLANAR, CS)
LEAVES_PLANAR_DIGEST = dg.sha256_digest(b"".join(dg.chunk_leaves(PLANAR, CS)))


def _leaves(data: bytes, cs: int) -> bytes:
    return b"".join(hashlib.sha256(data[o:o + cs]).digest()
                    for o in range(0, len(data), cs)) or hashlib.sha256(b"").digest()


def _flip(data: bytes, at: int = 5) -> bytes:
    b = bytearray(data)
    if b:
        b[min(at, len(b) - 1)] ^= 0xFF
    return bytes(b)


class EngineModel:
    """The GpuEngine methods the client calls, on host memory. Records
    ``(method, scalar args...)`` with pointers replaced by ``P``."""

    def __init__(self):
        self.store = {}   # url -> bytes, what ranged GETs serve
        self.sink = {}    # url -> bytes, what part uploads stored
        self.calls = []
        self.flip_first_full = False  # one byte of the first full fetch
        self.flip_every = False       # one byte of every fetch, ranged too
        self.stale_dedup = False      # the first gathered chunk is stale
        self.decode_failures = 0      # the first N decode calls raise
        self._full_fetches = 0
        self._index = {}              # leaf -> (address, length)

    # -- hashing
    def sha256_chunk_leaves(self, ptr, size, cs):
        self.calls.append(("sha256_chunk_leaves", P, size, cs))
        return _leaves(ctypes.string_at(ptr, size), cs)

    def sha256_chunk_leaves_many(self, items):
        self.calls.append(("sha256_chunk_leaves_many", [(P, s, cs) for _, s, cs in items]))
        return [_leaves(ctypes.string_at(p, s), cs) for p, s, cs in items]

    def sha256_canonical_device(self, ptr, size):
        self.calls.append(("sha256_canonical_device", P, size))
        return hashlib.sha256(ctypes.string_at(ptr, size)).digest()

    # -- transfers
    def _fetch(self, url, off, n, full):
        data = self.store[url][off:off + n]
        assert len(data) == n
        if full:
            self._full_fetches += 1
        if self.flip_every or (full and self.flip_first_full and self._full_fetches == 1):
            data = _flip(data)
        return data

    def _stats(self, size):
        return {"seconds": 0.0, "bytes": size, "gib_per_s": 0.0, "net_conn_seconds": 0.0}

    def pull_to_device(self, url, headers, size, ptr, conns):
        self.calls.append(("pull_to_device", url, headers, size, P, conns))
        ctypes.memmove(ptr, self._fetch(url, 0, size, True), size)
        return self._stats(size)

    def pull_to_device_hashed(self, url, headers, size, ptr, conns, cs):
        self.calls.append(("pull_to_device_hashed", url, headers, size, P, conns, cs))
        data = self._fetch(url, 0, size, True)
        ctypes.memmove(ptr, data, size)
        return self._stats(size), _leaves(data, cs)

    def pull_ranges_to_device(self, url, headers, ranges, ptr, conns):
        self.calls.append(("pull_ranges_to_device", url, headers, list(ranges), P, conns))
        for off, ln in ranges:
            ctypes.memmove(ptr + off, self._fetch(url, off, ln, False), ln)
        return self._stats(sum(ln for _, ln in ranges))

    def read_device(self, ptr, size):
        self.calls.append(("read_device", P, size))
        return ctypes.string_at(ptr, size)

    def push_part_from_device(self, url, method, headers, ptr, length):
        self.calls.append(("push_part_from_device", url, method, headers, P, length))
        self.sink[url] = ctypes.string_at(ptr, length)
        return {"status": 200}

    # -- chunk dedup
    def dedup_register(self, leaves, base, cs, size):
        self.calls.append(("dedup_register", len(leaves), P, cs, size))
        for i in range(len(leaves) // 32):
            ln = min(cs, size - i * cs)
            if ln > 0:
                self._index[(leaves[i * 32:(i + 1) * 32], ln)] = base + i * cs

    def dedup_reset(self, cap):
        self.calls.append(("dedup_reset", cap))
        self._index.clear()

    def dedup_pull(self, expect, dst, cs, size):
        self.calls.append(("dedup_pull", len(expect), P, cs, size))
        missing, hit_bytes = [], 0
        for i in range(len(expect) // 32):
            off = i * cs
            ln = min(cs, size - off)
            src = self._index.get((expect[i * 32:(i + 1) * 32], ln))
            if src is None:
                if missing and missing[-1][0] + missing[-1][1] == off:
                    missing[-1] = (missing[-1][0], missing[-1][1] + ln)
                else:
                    missing.append((off, ln))
                continue
            data = ctypes.string_at(src, ln)
            if self.stale_dedup and not hit_bytes:
                data = _flip(data)
            ctypes.memmove(dst + off, data, ln)
            hit_bytes += ln
        return missing, hit_bytes

    # -- byte planes and the identity "codec"
    def byte_planes(self, items, merge):
        self.calls.append(("byte_planes", [(P, P, n, e, g) for _, _, n, e, g in items], merge))
        for src, dst, n, elem, group in items:
            ctypes.memmove(dst, byte_planes(ctypes.string_at(src, n), elem, group, merge), n)

    def _decode(self, src, n, dst, cap):
        if self.decode_failures:
            self.decode_failures -= 1
            raise RuntimeError("injected decode failure")
        assert n <= cap
        ctypes.memmove(dst, ctypes.string_at(src, n), n)
        return n

    def zstd_decompress_device(self, src, n, dst, cap):
        self.calls.append(("zstd_decompress_device", P, n, P, cap))
        return self._decode(src, n, dst, cap)

    def zstd_decompress_many(self, items):
        self.calls.append(("zstd_decompress_many", [(P, n, P, cap) for _, n, _, cap in items]))
        return [self._decode(*it) for it in items]

    def zstd_compress_device(self, src, size, frame, dst, bound, literals_only=False):
        self.calls.append(("zstd_compress_device", P, size, frame, P, bound, literals_only))
        return self._decode(src, size, dst, bound)

    # -- directory blobs
    def tar_index(self, ptr, tar_len):
        self.calls.append(("tar_index", P, tar_len))
        with tarfile.open(fileobj=io.BytesIO(ctypes.string_at(ptr, tar_len))) as tf:
            return [{"name": m.name, "offset": m.offset_data, "size": m.size}
                    for m in tf.getmembers() if m.isfile()]

    def tar_scatter(self, ptr, segs):
        self.calls.append(("tar_scatter", P, [(off, P, n) for off, _, n in segs]))
        for off, dst, n in segs:
            ctypes.memmove(dst, ctypes.string_at(ptr + off, n), n)


def _strip_modified(obj):
    if isinstance(obj, dict):
        return {k: _strip_modified(v) for k, v in obj.items() if k != "modified"}
    if isinstance(obj, list):
        return [_strip_modified(v) for v in obj]
    return obj


class RemoteModel:
    """RegistryClient from dicts. ``redirect=False`` is a registry without
    presigned locations; ``plans=False`` one without pull plans."""

    SMALL = (types.MEDIA_TYPE_MODEL_CONFIG_YAML, types.MEDIA_TYPE_MODEL_LEAVES)

    def __init__(self, redirect=True, plans=True):
        self.redirect = redirect
        self.plans = plans
        self.manifests = {}      # version -> Manifest
        self.blobs = {}          # digest -> bytes served by get_blob_content
        self.present = set()     # digests head_blob finds
        self.uploaded = {}       # digest -> bytes taken by upload_blob_content
        self.plan_leaves = {}    # digest -> leaves64 override
        self.piece = 1 << 20
        self.corrupt_streams = 0  # the first N payload streams flip a byte
        self.calls = []

    @staticmethod
    def download_part(desc):
        return {"url": f"s3://{desc.name}", "signedHeader": {"x-sig": ["s"]}}

    def plan_entry(self, desc):
        entry = {"location": {"properties": {"parts": [self.download_part(desc)]}}}
        ld = desc.annotations.get(types.ANNOTATION_LEAVES_BLOB, "")
        if ld in self.plan_leaves:
            entry["leaves64"] = self.plan_leaves[ld]
        elif ld in self.blobs:
            entry["leaves64"] = base64.b64encode(self.blobs[ld]).decode()
        return entry

    def _plan(self, version):
        m = self.manifests[version or "latest"]
        return {"manifest": m.to_dict(),
                "blobs": {d.digest: self.plan_entry(d) for d in m.blobs if d.size}}

    def get_pull_plan(self, repository, version=""):
        self.calls.append(("get_pull_plan", repository, version))
        return self._plan(version) if self.plans else None

    def get_pull_plans(self, repository, refs):
        self.calls.append(("get_pull_plans", repository, list(refs)))
        if not self.plans:
            raise RuntimeError("no batched pull plans")
        return {v: self._plan(v) for v in refs}

    def get_manifest(self, repository, version=""):
        self.calls.append(("get_manifest", repository, version))
        return self.manifests[version or "latest"]

    def put_manifest(self, repository, version, manifest):
        self.calls.append(("put_manifest", repository, version,
                           _strip_modified(manifest.to_dict())))

    def head_blob(self, repository, digest):
        self.calls.append(("head_blob", repository, digest))
        return digest in self.present

    def get_blob_location(self, repository, desc, purpose, extra=None):
        self.calls.append(("get_blob_location", repository, desc.name, purpose, extra))
        if not self.redirect:
            return None
        if purpose == "download":
            return types.BlobLocation(purpose=purpose,
                                      properties={"parts": [self.download_part(desc)]})
        if desc.media_type in self.SMALL:
            return None
        n = int((extra or {}).get("part-count", 1))
        parts = [{"url": f"s3://{desc.name}?part={i}", "method": "PUT"} for i in range(n)]
        return types.BlobLocation(purpose=purpose, properties={"parts": parts})

    def get_blob_content(self, repository, digest, chunk_size=1 << 20):
        self.calls.append(("get_blob_content", repository, digest))
        if digest not in self.blobs:
            raise er.ModelxError(er.ErrCode.BLOB_UNKNOWN, digest)
        data = self.blobs[digest]
        if self.corrupt_streams:
            self.corrupt_streams -= 1
            data = _flip(data)
        for off in range(0, len(data), self.piece):
            yield data[off:off + self.piece]

    def upload_blob_content(self, repository, desc, data):
        body = data if isinstance(data, bytes) else data.read()
        self.calls.append(("upload_blob_content", repository, desc.name, desc.digest,
                           len(body)))
        self.uploaded[desc.digest] = body


def blob_desc(name="w", data=BLOB, main="chunked", chunk_note=True, leaves=True,
              media_type=types.MEDIA_TYPE_MODEL_FILE, extra=None):
    notes = {}
    if chunk_note:
        notes[types.ANNOTATION_CHUNK_DIGEST] = dg.chunked_digest(data, CS)
        notes[types.ANNOTATION_CHUNK_SIZE] = str(CS)
    if leaves:
        notes[types.ANNOTATION_LEAVES_BLOB] = dg.sha256_digest(_leaves(data, CS))
    notes.update(extra or {})
    digest = dg.chunked_digest(data, CS) if main == "chunked" else dg.sha256_digest(data)
    return types.Descriptor(name=name, media_type=media_type, digest=digest,
                            size=len(data), annotations=notes)


def zstd_desc(name="z", raw=BLOB, stored=None, raw_size=True, planes="", **kw):
    """A +zstd descriptor under the identity codec: the stored bytes are the
    raw bytes (or their planar form)."""
    stored = raw if stored is None else stored
    extra = {types.ANNOTATION_RAW_DIGEST: dg.chunked_digest(raw, CS)}
    if raw_size:
        extra[types.ANNOTATION_RAW_SIZE] = str(len(raw) if raw_size is True else raw_size)
    if planes:
        extra[types.ANNOTATION_BYTE_PLANES] = planes
    return blob_desc(name, stored, media_type=types.MEDIA_TYPE_MODEL_FILE_ZSTD,
                     extra=extra, **kw)


def leaves_desc(desc, data):
    lv = _leaves(data, CS)
    return types.Descriptor(name=desc.name + ".leaves",
                            media_type=types.MEDIA_TYPE_MODEL_LEAVES,
                            digest=dg.sha256_digest(lv), size=len(lv))


def host(data: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).clone()


def raw(t) -> bytes:
    return t.numpy().tobytes()


class Env:
    def __init__(self, monkeypatch, capsys):
        self.monkeypatch = monkeypatch
        self.capsys = capsys
        self.eng = EngineModel()
        self.rem = RemoteModel()
        g = GpuClient.__new__(GpuClient)
        g.remote, g.engine = self.rem, self.eng
        g.device, g.num_conns, g.slot_bytes = 0, 4, 4096
        g.last_stats = []
        g.dedup, g._dedup_tensors, g._dedup_registered = False, [], False
        self.g = g

    def serve(self, desc, data, sidecar=True):
        """Make a blob pullable: the object store has it, the registry
        streams it, and its leaves sidecar exists."""
        self.eng.store[f"s3://{desc.name}"] = data
        self.rem.blobs[desc.digest] = data
        ld = desc.annotations.get(types.ANNOTATION_LEAVES_BLOB, "")
        if ld and sidecar:
            self.rem.blobs[ld] = _leaves(data, CS)
        return desc

    def manifest(self, version, descs):
        self.rem.manifests[version] = types.Manifest(
            media_type=types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
            config=types.Descriptor(name="modelx.yaml", digest=CONFIG_DIGEST,
                                    media_type=types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                                    size=len(CONFIG)),
            blobs=list(descs))

    def stats(self):
        return [{k: v for k, v in s.items() if k != "seconds"} for s in self.g.last_stats]

    def expect(self, engine, remote, stats, unordered=False):
        got_e, got_r = self.eng.calls, self.rem.calls
        if unordered:
            got_e, got_r = sorted(got_e, key=repr), sorted(got_r, key=repr)
            engine, remote = sorted(engine, key=repr), sorted(remote, key=repr)
        assert got_e == engine
        assert got_r == remote
        assert self.stats() == stats

    def fails(self, code, suffix, fn):
        with pytest.raises(er.ModelxError) as ei:
            fn()
        assert ei.value.code == code
        assert ei.value.message.endswith(suffix), ei.value.message
        return ei.value


@pytest.fixture
def env(monkeypatch, capsys):
    real_empty = torch.empty

    def host_empty(*a, **kw):
        kw.pop("device", None)
        kw.pop("pin_memory", None)
        return real_empty(*a, **kw)

    monkeypatch.setattr(torch, "empty", host_empty)
    monkeypatch.setattr(GpuClient, "_sync_producers", lambda self: None)
    monkeypatch.setattr(gpu, "_core", lambda: pytypes.SimpleNamespace(
        zstd_compress_bound=lambda size: size + 64,
        tar_pack_layout=lambda members: {"total": 0}))
    monkeypatch.delenv("MODELX_ZSTD_DUMP", raising=False)
    return Env(monkeypatch, capsys)


GET_W = ("get_blob_location", REPO, "w", "download", None)
GET_LEAVES = ("get_blob_content", REPO, LEAVES_DIGEST)


# ------------------------------------------------- pull_blob_to_device --

def test_pull_chunked_clean(env):
    d = env.serve(blob_desc(), BLOB)
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024)],
        remote=[GET_W],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_flipped_byte_refetches_one_chunk(env):
    d = env.serve(blob_desc(), BLOB)
    env.eng.flip_first_full = True
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(0, 1024)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W, GET_LEAVES],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-chunk-refetch', 'bytes': 1024},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_flipped_byte_without_leaves_annotation(env):
    d = env.serve(blob_desc(leaves=False), BLOB)
    env.eng.flip_first_full = True
    env.fails(er.ErrCode.DIGEST_INVALID,
              f"[size=2563 media={types.MEDIA_TYPE_MODEL_FILE} path=no-leaves-sidecar]",
              lambda: env.g.pull_blob_to_device(REPO, d))
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'}])


def test_pull_flipped_byte_with_sidecar_one_leaf_too_long(env):
    long_leaves = LEAVES + b"\0" * 32
    d = blob_desc()
    d.annotations[types.ANNOTATION_LEAVES_BLOB] = dg.sha256_digest(long_leaves)
    env.serve(d, BLOB, sidecar=False)
    env.rem.blobs[dg.sha256_digest(long_leaves)] = long_leaves
    env.eng.flip_first_full = True
    env.fails(er.ErrCode.DIGEST_INVALID,
              f"[size=2563 media={types.MEDIA_TYPE_MODEL_FILE} path=no-leaves-sidecar]",
              lambda: env.g.pull_blob_to_device(REPO, d))
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W,
                ('get_blob_content',
                 REPO,
                 'sha256:1998e12f51fad7fc53633899830431a6fb717a71997f4245ad8bc6b2e7225af3')],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'}])


def test_pull_sidecar_matches_but_descriptor_digest_differs(env):
    d = blob_desc()
    d.digest = ROOT_OTHER
    env.serve(d, BLOB)
    env.fails(er.ErrCode.DIGEST_INVALID,
              f"[size=2563 media={types.MEDIA_TYPE_MODEL_FILE} "
              "path=leaves-match-but-root-differs]",
              lambda: env.g.pull_blob_to_device(REPO, d))
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W, GET_LEAVES],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'}])


def test_pull_store_serves_bad_bytes_on_ranged_fetches_too(env):
    d = env.serve(blob_desc(), BLOB)
    env.eng.flip_every = True
    env.fails(er.ErrCode.DIGEST_INVALID,
              f"[size=2563 media={types.MEDIA_TYPE_MODEL_FILE} "
              "path=refetch-did-not-fix ranges=1]",
              lambda: env.g.pull_blob_to_device(REPO, d))
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(0, 1024)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W, GET_LEAVES],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-chunk-refetch', 'bytes': 1024}])


def test_pull_canonical_digest_without_chunk_annotation(env):
    d = env.serve(blob_desc(main="canonical", chunk_note=False, leaves=False), BLOB)
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device', 's3://w', SIGNED, 2563, P, 4),
                ('sha256_canonical_device', P, 2563)],
        remote=[GET_W],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_canonical_digest_with_chunk_annotation(env):
    d = env.serve(blob_desc(main="canonical"), BLOB)
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024)],
        remote=[GET_W],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_canonical_digest_with_chunk_annotation_flipped(env):
    """The streamed root misses the annotation, the full verify then runs
    against the annotation at the annotation's own chunk size."""
    d = env.serve(blob_desc(main="canonical"), BLOB)
    env.eng.flip_first_full = True
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(0, 1024)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W, GET_LEAVES],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-chunk-refetch', 'bytes': 1024},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_slot_not_a_chunk_multiple(env):
    d = env.serve(blob_desc(), BLOB)
    env.g.slot_bytes = 3000
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device', 's3://w', SIGNED, 2563, P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_without_verify(env):
    d = env.serve(blob_desc(), BLOB)
    env.eng.flip_first_full = True
    out = env.g.pull_blob_to_device(REPO, d, verify=False)
    assert raw(out) == _flip(BLOB)
    env.expect(
        engine=[('pull_to_device', 's3://w', SIGNED, 2563, P, 4)],
        remote=[GET_W],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer'}])


def test_pull_zero_size_blob(env):
    d = env.serve(blob_desc(data=b""), b"")
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == b""
    env.expect(
        engine=[('pull_to_device', 's3://w', SIGNED, 0, P, 4),
                ('sha256_chunk_leaves', P, 0, 1024)],
        remote=[GET_W],
        stats=[{'bytes': 0,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer'},
               {'phase': 'pull-verify', 'bytes': 0}])


def test_pull_plan_entry_needs_no_remote_call(env):
    d = env.serve(blob_desc(), BLOB)
    env.eng.flip_first_full = True  # so that the inlined leaves are used
    out = env.g.pull_blob_to_device(REPO, d, plan_entry=env.rem.plan_entry(d))
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(0, 1024)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-chunk-refetch', 'bytes': 1024},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_plan_entry_with_tampered_leaves(env):
    d = env.serve(blob_desc(), BLOB)
    env.rem.plan_leaves[LEAVES_DIGEST] = base64.b64encode(LEAVES_OTHER).decode()
    env.eng.flip_first_full = True
    out = env.g.pull_blob_to_device(REPO, d, plan_entry=env.rem.plan_entry(d))
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(0, 1024)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_LEAVES],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-chunk-refetch', 'bytes': 1024},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_resume_fetches_the_differing_chunk(env):
    d = env.serve(blob_desc(), BLOB)
    have = host(BLOB[:1024] + OTHER[1024:2048] + BLOB[2048:])
    out = env.g.pull_blob_to_device(REPO, d, tensor=have, resume=True)
    assert out is have and raw(out) == BLOB
    env.expect(
        engine=[('sha256_chunk_leaves', P, 2563, 1024),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(1024, 1024)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W, GET_LEAVES],
        stats=[{'phase': 'pull-resume', 'bytes': 1024, 'skipped': 1539}])


def test_pull_resume_without_sidecar_is_a_full_pull(env):
    d = env.serve(blob_desc(leaves=False), BLOB)
    have = host(OTHER)
    out = env.g.pull_blob_to_device(REPO, d, tensor=have, resume=True)
    assert out is have and raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024)],
        remote=[GET_W],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def _redirectless(env, corrupt_streams):
    env.rem.redirect = False
    env.rem.piece = 700
    env.rem.corrupt_streams = corrupt_streams
    env.g.slot_bytes = 1000
    return env.serve(blob_desc(), BLOB)


def test_pull_registry_stream_clean(env):
    d = _redirectless(env, 0)
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W, ('get_blob_content', REPO, ROOT)],
        stats=[{'phase': 'pull-registry-stream', 'bytes': 2563}])


def test_pull_registry_stream_second_attempt_clean(env):
    d = _redirectless(env, 1)
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('sha256_chunk_leaves', P, 2563, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W,
                ('get_blob_content', REPO, ROOT),
                ('get_blob_content', REPO, ROOT)],
        stats=[{'phase': 'pull-registry-stream', 'bytes': 2563},
               {'phase': 'pull-registry-stream', 'bytes': 2563}])


def test_pull_registry_stream_both_attempts_corrupt(env):
    d = _redirectless(env, 2)
    err = env.fails(er.ErrCode.DIGEST_INVALID, f"!= {ROOT}",
                    lambda: env.g.pull_blob_to_device(REPO, d))
    assert err.message.startswith("GPU chunk digest mismatch for w: ")
    env.expect(
        engine=[('sha256_chunk_leaves', P, 2563, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W,
                ('get_blob_content', REPO, ROOT),
                ('get_blob_content', REPO, ROOT)],
        stats=[{'phase': 'pull-registry-stream', 'bytes': 2563},
               {'phase': 'pull-registry-stream', 'bytes': 2563}])


def _dedup(env, resident: bytes):
    env.g.dedup = True
    keep = host(resident)
    env.g.register_chunks(keep, _leaves(resident, CS), CS)
    env.eng.calls.clear()
    return env.serve(blob_desc(), BLOB)


def test_pull_dedup_hits(env):
    d = _dedup(env, BLOB[:2048])
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('dedup_pull', 96, P, 1024, 2563),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(2048, 515)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('dedup_register', 96, P, 1024, 2563)],
        remote=[GET_W, GET_LEAVES],
        stats=[{'phase': 'pull-dedup', 'bytes': 515, 'dedup_bytes': 2048}])


def test_pull_dedup_stale_gathered_chunk_is_refetched(env):
    d = _dedup(env, BLOB[:2048])
    env.eng.stale_dedup = True
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    assert env.capsys.readouterr().err == (
        "modelx: dedup refetch w: 1 ranges, chunks by origin "
        "{'gathered': 1, 'fetched': 0}\n")
    env.expect(
        engine=[('dedup_pull', 96, P, 1024, 2563),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(2048, 515)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(0, 1024)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('dedup_register', 96, P, 1024, 2563)],
        remote=[GET_W, GET_LEAVES],
        stats=[{'phase': 'pull-dedup',
                'bytes': 515,
                'dedup_bytes': 2048,
                'refetched_bytes': 1024,
                'refetched_ranges': 1}])


def test_pull_dedup_zero_hits_is_a_full_pull(env):
    d = _dedup(env, OTHER)
    out = env.g.pull_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('dedup_pull', 96, P, 1024, 2563),
                ('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('dedup_register', 96, P, 1024, 2563)],
        remote=[GET_W, GET_LEAVES],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_dedup_still_wrong_after_refetch(env):
    d = _dedup(env, BLOB[:2048])
    env.eng.stale_dedup = True
    env.eng.flip_every = True
    err = env.fails(er.ErrCode.DIGEST_INVALID, "",
                    lambda: env.g.pull_blob_to_device(REPO, d))
    assert err.message.startswith("GPU chunk digest mismatch for w: sha256c1k:")
    env.expect(
        engine=[('dedup_pull', 96, P, 1024, 2563),
                ('pull_ranges_to_device', 's3://w', SIGNED, [(2048, 515)], P, 4),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('pull_ranges_to_device',
                 's3://w',
                 SIGNED,
                 [(0, 1024), (2048, 515)],
                 P,
                 4),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[GET_W, GET_LEAVES],
        stats=[{'phase': 'pull-dedup',
                'bytes': 515,
                'dedup_bytes': 2048,
                'refetched_bytes': 1539,
                'refetched_ranges': 2}])


# --------------------------------------------------------------- +zstd --

def test_zstd_single_blob(env):
    d = env.serve(zstd_desc(), BLOB)
    out = env.g.pull_zstd_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_device', P, 2563, P, 2563),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_blob_location', REPO, 'z', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress', 'bytes': 2563}])


def test_zstd_size_mismatch(env):
    d = env.serve(zstd_desc(raw_size=3000), BLOB)
    env.fails(er.ErrCode.DIGEST_INVALID, "zstd size mismatch for z: 2563 != 3000",
              lambda: env.g.pull_zstd_blob_to_device(REPO, d))
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_device', P, 2563, P, 3000)],
        remote=[('get_blob_location', REPO, 'z', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress', 'bytes': 2563}])


def test_zstd_missing_raw_size_is_refused_after_the_fetch(env):
    d = env.serve(zstd_desc(raw_size=False), BLOB)
    env.fails(er.ErrCode.UNSUPPORTED, "+zstd blob z lacks the raw-size annotation",
              lambda: env.g.pull_zstd_blob_to_device(REPO, d))
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z', SIGNED, 2563, P, 4, 1024)],
        remote=[('get_blob_location', REPO, 'z', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_zstd_decode_failure_is_retried_once(env):
    d = env.serve(zstd_desc(), BLOB)
    env.eng.decode_failures = 1
    out = env.g.pull_zstd_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    assert env.capsys.readouterr().err == (
        "modelx: zstd decode failed (injected decode failure); retrying once "
        "(set MODELX_ZSTD_DUMP=<dir> to keep the blob)\n")
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_device', P, 2563, P, 2563),
                ('zstd_decompress_device', P, 2563, P, 2563),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_blob_location', REPO, 'z', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress', 'bytes': 2563}])


def test_zstd_second_decode_failure_propagates(env):
    d = env.serve(zstd_desc(), BLOB)
    env.eng.decode_failures = 2
    with pytest.raises(RuntimeError, match="injected decode failure"):
        env.g.pull_zstd_blob_to_device(REPO, d)
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_device', P, 2563, P, 2563),
                ('zstd_decompress_device', P, 2563, P, 2563)],
        remote=[('get_blob_location', REPO, 'z', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_zstd_byte_planes(env):
    d = env.serve(zstd_desc(stored=PLANAR, planes="2:1024"), PLANAR)
    out = env.g.pull_zstd_blob_to_device(REPO, d)
    assert raw(out) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_device', P, 2563, P, 2563),
                ('byte_planes', [(P, P, 2563, 2, 1024)], True),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_blob_location', REPO, 'z', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress', 'bytes': 2563},
               {'phase': 'pull-byte-planes-merge', 'bytes': 2563, 'blobs': 1}])


def test_zstd_malformed_byte_planes_is_refused_before_any_call(env):
    d = env.serve(zstd_desc(stored=PLANAR, planes="3:1024"), PLANAR)
    env.fails(er.ErrCode.UNSUPPORTED,
              f"unsupported {types.ANNOTATION_BYTE_PLANES} annotation '3:1024'",
              lambda: env.g.pull_zstd_blob_to_device(REPO, d))
    env.expect(engine=[], remote=[], stats=[])
    env.fails(er.ErrCode.UNSUPPORTED,
              f"unsupported {types.ANNOTATION_BYTE_PLANES} annotation '3:1024'",
              lambda: env.g._pull_zstd_batched(REPO, [("k", d, None)], True, 1))
    env.expect(engine=[], remote=[], stats=[])


def test_zstd_batched_two_blobs_one_planar(env):
    a = env.serve(zstd_desc("a", raw=OTHER), OTHER)
    b = env.serve(zstd_desc("b", stored=PLANAR, planes="2:1024"), PLANAR)
    out = env.g._pull_zstd_batched(REPO, [("ka", a, None), ("kb", b, None)], True, 1)
    assert {k: raw(t) for k, t in out.items()} == {"ka": OTHER, "kb": BLOB}
    env.expect(
        engine=[('pull_to_device_hashed', 's3://a', SIGNED, 2563, P, 4, 1024),
                ('pull_to_device_hashed', 's3://b', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_many', [(P, 2563, P, 2563), (P, 2563, P, 2563)]),
                ('byte_planes', [(P, P, 2563, 2, 1024)], True),
                ('sha256_chunk_leaves_many', [(P, 2563, 1024), (P, 2563, 1024)])],
        remote=[('get_blob_location', REPO, 'a', 'download', None),
                ('get_blob_location', REPO, 'b', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'a',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'b',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress-batched', 'bytes': 5126, 'blobs': 2},
               {'phase': 'pull-byte-planes-merge', 'bytes': 2563, 'blobs': 1},
               {'phase': 'pull-zstd-raw-verify-batched', 'bytes': 5126}])


def test_zstd_batched_missing_raw_size_and_size_mismatch(env):
    a = env.serve(zstd_desc("a", raw_size=False), BLOB)
    env.fails(er.ErrCode.UNSUPPORTED, "+zstd blob a lacks the raw-size annotation",
              lambda: env.g._pull_zstd_batched(REPO, [("ka", a, None)], True, 1))
    b = env.serve(zstd_desc("b", raw_size=3000), BLOB)
    env.fails(er.ErrCode.DIGEST_INVALID, "zstd size mismatch for b: 2563 != 3000",
              lambda: env.g._pull_zstd_batched(REPO, [("kb", b, None)], True, 1))
    c = zstd_desc("c")
    c.annotations[types.ANNOTATION_RAW_DIGEST] = ROOT_OTHER
    env.serve(c, BLOB)
    env.fails(er.ErrCode.DIGEST_INVALID, "uncompressed digest mismatch for c",
              lambda: env.g._pull_zstd_batched(REPO, [("kc", c, None)], True, 1))
    env.fails(er.ErrCode.DIGEST_INVALID, "uncompressed digest mismatch for c",
              lambda: env.g.pull_zstd_blob_to_device(REPO, c))
    env.expect(
        engine=[('pull_to_device_hashed', 's3://a', SIGNED, 2563, P, 4, 1024),
                ('pull_to_device_hashed', 's3://b', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_many', [(P, 2563, P, 3000)]),
                ('pull_to_device_hashed', 's3://c', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_many', [(P, 2563, P, 2563)]),
                ('sha256_chunk_leaves_many', [(P, 2563, 1024)]),
                ('pull_to_device_hashed', 's3://c', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_device', P, 2563, P, 2563),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_blob_location', REPO, 'a', 'download', None),
                ('get_blob_location', REPO, 'b', 'download', None),
                ('get_blob_location', REPO, 'c', 'download', None),
                ('get_blob_location', REPO, 'c', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'a',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'b',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress-batched', 'bytes': 2563, 'blobs': 1},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'c',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress-batched', 'bytes': 2563, 'blobs': 1},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'c',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress', 'bytes': 2563}])


# --------------------------------------------------------- pull_to_gpu --

def _mixed_manifest(env, nzstd):
    w = env.serve(blob_desc(), BLOB)
    descs = [w, leaves_desc(w, BLOB), blob_desc("empty", b"", leaves=False)]
    for i in range(nzstd):
        descs.append(env.serve(zstd_desc(f"z{i}", raw=(OTHER, THIRD)[i]), (OTHER, THIRD)[i]))
    env.manifest("v1", descs)
    return {d.name: env.eng.store[f"s3://{d.name}"] for d in descs[:1] + descs[3:]}


def test_pull_to_gpu_single_zstd_with_plan(env):
    want = _mixed_manifest(env, 1)
    out = env.g.pull_to_gpu(REPO, "v1")
    assert {k: raw(t) for k, t in out.items()} == want
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('pull_to_device_hashed', 's3://z0', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_device', P, 2563, P, 2563),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_pull_plan', REPO, 'v1')],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z0',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress', 'bytes': 2563}])


def test_pull_to_gpu_single_zstd_without_plan(env):
    want = _mixed_manifest(env, 1)
    env.rem.plans = False
    out = env.g.pull_to_gpu(REPO, "v1")
    assert {k: raw(t) for k, t in out.items()} == want
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('pull_to_device_hashed', 's3://z0', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_device', P, 2563, P, 2563),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_pull_plan', REPO, 'v1'),
                ('get_manifest', REPO, 'v1'),
                GET_W,
                ('get_blob_location', REPO, 'z0', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z0',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress', 'bytes': 2563}])


def test_pull_to_gpu_two_zstd_are_batched_with_plan(env):
    want = _mixed_manifest(env, 2)
    out = env.g.pull_to_gpu(REPO, "v1")
    assert {k: raw(t) for k, t in out.items()} == want
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z0', SIGNED, 2563, P, 4, 1024),
                ('pull_to_device_hashed', 's3://z1', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_many', [(P, 2563, P, 2563), (P, 2563, P, 2563)]),
                ('sha256_chunk_leaves_many', [(P, 2563, 1024), (P, 2563, 1024)]),
                ('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024)],
        remote=[('get_pull_plan', REPO, 'v1')],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z0',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z1',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress-batched', 'bytes': 5126, 'blobs': 2},
               {'phase': 'pull-zstd-raw-verify-batched', 'bytes': 5126},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_to_gpu_two_zstd_are_batched_without_plan(env):
    want = _mixed_manifest(env, 2)
    env.rem.plans = False
    out = env.g.pull_to_gpu(REPO, "v1")
    assert {k: raw(t) for k, t in out.items()} == want
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z0', SIGNED, 2563, P, 4, 1024),
                ('pull_to_device_hashed', 's3://z1', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_many', [(P, 2563, P, 2563), (P, 2563, P, 2563)]),
                ('sha256_chunk_leaves_many', [(P, 2563, 1024), (P, 2563, 1024)]),
                ('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024)],
        remote=[('get_pull_plan', REPO, 'v1'),
                ('get_manifest', REPO, 'v1'),
                ('get_blob_location', REPO, 'z0', 'download', None),
                ('get_blob_location', REPO, 'z1', 'download', None),
                GET_W],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z0',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z1',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress-batched', 'bytes': 5126, 'blobs': 2},
               {'phase': 'pull-zstd-raw-verify-batched', 'bytes': 5126},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def _tar(members) -> bytes:
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.USTAR_FORMAT) as tf:
        for name, data in members:
            info = tarfile.TarInfo(name)
            info.size = len(data)
            tf.addfile(info, io.BytesIO(data))
    return buf.getvalue()


def test_pull_to_gpu_expand_dirs(env):
    archive = _tar([("shards/a.bin", BLOB[:700]), ("shards/empty", b"")])
    w = env.serve(blob_desc(), BLOB)
    s = env.serve(blob_desc("shards", archive, leaves=False,
                            media_type=types.MEDIA_TYPE_MODEL_DIRECTORY_TAR), archive)
    env.manifest("v1", [w, s])
    out = env.g.pull_to_gpu(REPO, "v1", expand_dirs=True)
    assert {k: raw(t) for k, t in out.items()} == {
        "w": BLOB, "shards/a.bin": BLOB[:700], "shards/empty": b""}
    env.expect(
        engine=[('pull_to_device_hashed', 's3://w', SIGNED, 2563, P, 4, 1024),
                ('pull_to_device_hashed', 's3://shards', SIGNED, 10240, P, 4, 1024),
                ('tar_index', P, 10240),
                ('tar_scatter', P, [(512, P, 700)])],
        remote=[('get_pull_plan', REPO, 'v1')],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'bytes': 10240,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'shards',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 10240}])


def test_pull_to_gpu_expand_dirs_member_clashes_with_a_file_blob(env):
    archive = _tar([("w", BLOB[:700])])
    w = env.serve(blob_desc(), BLOB)
    s = env.serve(blob_desc("shards", archive, leaves=False,
                            media_type=types.MEDIA_TYPE_MODEL_DIRECTORY_TAR), archive)
    env.manifest("v1", [w, s])
    env.fails(er.ErrCode.MANIFEST_INVALID,
              "expand_dirs: 'w' is named by more than one blob",
              lambda: env.g.pull_to_gpu(REPO, "v1", expand_dirs=True))


# ----------------------------------------------------------- pull_many --

def _two_versions(env):
    env.manifest("v1", [env.serve(zstd_desc("z1", raw=THIRD), THIRD),
                        env.serve(blob_desc("w1"), BLOB)])
    env.manifest("v2", [env.serve(zstd_desc("z2", raw=OTHER), OTHER)])
    return {"v1": {"z1": THIRD, "w1": BLOB}, "v2": {"z2": OTHER}}


def test_pull_many_batches_zstd_across_versions(env):
    want = _two_versions(env)
    out = env.g.pull_many(REPO, ["v1", "v2"], parallel=1)
    assert {v: {k: raw(t) for k, t in m.items()} for v, m in out.items()} == want
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z1', SIGNED, 2563, P, 4, 1024),
                ('pull_to_device_hashed', 's3://z2', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_many', [(P, 2563, P, 2563), (P, 2563, P, 2563)]),
                ('sha256_chunk_leaves_many', [(P, 2563, 1024), (P, 2563, 1024)]),
                ('pull_to_device_hashed', 's3://w1', SIGNED, 2563, P, 4, 1024)],
        remote=[('get_pull_plans', REPO, ['v1', 'v2'])],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z1',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z2',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress-batched', 'bytes': 5126, 'blobs': 2},
               {'phase': 'pull-zstd-raw-verify-batched', 'bytes': 5126},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w1',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_many_falls_back_to_per_version_plans(env):
    want = _two_versions(env)
    env.rem.plans = False
    out = env.g.pull_many(REPO, ["v1", "v2"], parallel=1)
    assert {v: {k: raw(t) for k, t in m.items()} for v, m in out.items()} == want
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z1', SIGNED, 2563, P, 4, 1024),
                ('pull_to_device_hashed', 's3://z2', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_many', [(P, 2563, P, 2563), (P, 2563, P, 2563)]),
                ('sha256_chunk_leaves_many', [(P, 2563, 1024), (P, 2563, 1024)]),
                ('pull_to_device_hashed', 's3://w1', SIGNED, 2563, P, 4, 1024)],
        remote=[('get_pull_plans', REPO, ['v1', 'v2']),
                ('get_pull_plan', REPO, 'v1'),
                ('get_manifest', REPO, 'v1'),
                ('get_pull_plan', REPO, 'v2'),
                ('get_manifest', REPO, 'v2'),
                ('get_blob_location', REPO, 'z1', 'download', None),
                ('get_blob_location', REPO, 'z2', 'download', None),
                ('get_blob_location', REPO, 'w1', 'download', None)],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z1',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z2',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress-batched', 'bytes': 5126, 'blobs': 2},
               {'phase': 'pull-zstd-raw-verify-batched', 'bytes': 5126},
               {'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'w1',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563}])


def test_pull_many_single_zstd_blob_takes_the_single_path(env):
    env.manifest("v1", [env.serve(zstd_desc("z1"), BLOB)])
    out = env.g.pull_many(REPO, ["v1"], parallel=1)
    assert raw(out["v1"]["z1"]) == BLOB
    env.expect(
        engine=[('pull_to_device_hashed', 's3://z1', SIGNED, 2563, P, 4, 1024),
                ('zstd_decompress_device', P, 2563, P, 2563),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_pull_plans', REPO, ['v1'])],
        stats=[{'bytes': 2563,
                'gib_per_s': 0.0,
                'net_conn_seconds': 0.0,
                'name': 'z1',
                'phase': 'pull-transfer-hashed'},
               {'phase': 'pull-verify', 'bytes': 2563},
               {'phase': 'pull-zstd-decompress', 'bytes': 2563}])


# ------------------------------------------------------- push_from_gpu --

def _uploaded(env, name, nparts=1):
    return b"".join(env.eng.sink[f"s3://{name}?part={i}"] for i in range(nparts))


def test_push_one_tensor(env):
    m = env.g.push_from_gpu(REPO, "v1", {"w": host(BLOB)}, chunk_size=CS)
    assert _uploaded(env, "w") == BLOB
    assert env.rem.uploaded == {CONFIG_DIGEST: CONFIG, LEAVES_DIGEST: LEAVES}
    assert _strip_modified(m.to_dict()) == env.rem.calls[-1][3]
    env.expect(
        engine=[('push_part_from_device', 's3://w?part=0', 'PUT', {}, P, 2563),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_blob_location', REPO, 'modelx.yaml', 'upload', None),
                ('get_blob_location', REPO, 'w', 'upload', None),
                ('get_blob_location', REPO, 'w.leaves', 'upload', None),
                ('head_blob', REPO, CONFIG_DIGEST),
                ('head_blob', REPO, LEAVES_DIGEST),
                ('head_blob', REPO, ROOT),
                ('put_manifest',
                 REPO,
                 'v1',
                 {'schemaVersion': 1,
                  'mediaType': types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
                  'config': {'name': 'modelx.yaml',
                             'mediaType': types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                             'digest': CONFIG_DIGEST,
                             'size': 29},
                  'blobs': [{'name': 'w',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE,
                             'digest': ROOT,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_DIGEST}},
                            {'name': 'w.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_DIGEST,
                             'size': 96}]}),
                ('upload_blob_content', REPO, 'modelx.yaml', CONFIG_DIGEST, 29),
                ('upload_blob_content', REPO, 'w.leaves', LEAVES_DIGEST, 96)],
        stats=[{'phase': 'gpu-digest', 'bytes': 2563},
               {'phase': 'push-upload', 'bytes': 2563, 'parts': 1}],
        unordered=True)


def test_push_two_tensors_batched(env):
    env.g.push_from_gpu(REPO, "", {"w": host(BLOB), "o": host(OTHER)}, chunk_size=CS)
    assert _uploaded(env, "w") == BLOB and _uploaded(env, "o") == OTHER
    env.expect(
        engine=[('push_part_from_device', 's3://o?part=0', 'PUT', {}, P, 2563),
                ('push_part_from_device', 's3://w?part=0', 'PUT', {}, P, 2563),
                ('sha256_chunk_leaves_many', [(P, 2563, 1024), (P, 2563, 1024)])],
        remote=[('get_blob_location', REPO, 'modelx.yaml', 'upload', None),
                ('get_blob_location', REPO, 'o', 'upload', None),
                ('get_blob_location', REPO, 'o.leaves', 'upload', None),
                ('get_blob_location', REPO, 'w', 'upload', None),
                ('get_blob_location', REPO, 'w.leaves', 'upload', None),
                ('head_blob', REPO, CONFIG_DIGEST),
                ('head_blob', REPO, LEAVES_OTHER_DIGEST),
                ('head_blob', REPO, LEAVES_DIGEST),
                ('head_blob', REPO, ROOT_OTHER),
                ('head_blob', REPO, ROOT),
                ('put_manifest',
                 REPO,
                 'latest',
                 {'schemaVersion': 1,
                  'mediaType': types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
                  'config': {'name': 'modelx.yaml',
                             'mediaType': types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                             'digest': CONFIG_DIGEST,
                             'size': 29},
                  'blobs': [{'name': 'o',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE,
                             'digest': ROOT_OTHER,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT_OTHER,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_OTHER_DIGEST}},
                            {'name': 'o.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_OTHER_DIGEST,
                             'size': 96},
                            {'name': 'w',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE,
                             'digest': ROOT,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_DIGEST}},
                            {'name': 'w.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_DIGEST,
                             'size': 96}]}),
                ('upload_blob_content', REPO, 'modelx.yaml', CONFIG_DIGEST, 29),
                ('upload_blob_content', REPO, 'o.leaves', LEAVES_OTHER_DIGEST, 96),
                ('upload_blob_content', REPO, 'w.leaves', LEAVES_DIGEST, 96)],
        stats=[{'phase': 'gpu-digest-batched', 'bytes': 5126, 'blobs': 2},
               {'phase': 'push-upload', 'bytes': 2563, 'parts': 1},
               {'phase': 'push-upload', 'bytes': 2563, 'parts': 1}],
        unordered=True)


def test_push_two_tensors_canonical_digest(env):
    env.g.push_from_gpu(REPO, "v1", {"w": host(BLOB), "o": host(OTHER)}, chunk_size=CS,
                        digest_mode="sha256")
    env.expect(
        engine=[('push_part_from_device', 's3://o?part=0', 'PUT', {}, P, 2563),
                ('push_part_from_device', 's3://w?part=0', 'PUT', {}, P, 2563),
                ('sha256_canonical_device', P, 2563),
                ('sha256_canonical_device', P, 2563),
                ('sha256_chunk_leaves_many', [(P, 2563, 1024), (P, 2563, 1024)])],
        remote=[('get_blob_location', REPO, 'modelx.yaml', 'upload', None),
                ('get_blob_location', REPO, 'o', 'upload', None),
                ('get_blob_location', REPO, 'o.leaves', 'upload', None),
                ('get_blob_location', REPO, 'w', 'upload', None),
                ('get_blob_location', REPO, 'w.leaves', 'upload', None),
                ('head_blob', REPO, CONFIG_DIGEST),
                ('head_blob', REPO, CANON_OTHER),
                ('head_blob', REPO, LEAVES_OTHER_DIGEST),
                ('head_blob', REPO, CANON),
                ('head_blob', REPO, LEAVES_DIGEST),
                ('put_manifest',
                 REPO,
                 'v1',
                 {'schemaVersion': 1,
                  'mediaType': types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
                  'config': {'name': 'modelx.yaml',
                             'mediaType': types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                             'digest': CONFIG_DIGEST,
                             'size': 29},
                  'blobs': [{'name': 'o',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE,
                             'digest': CANON_OTHER,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT_OTHER,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_OTHER_DIGEST}},
                            {'name': 'o.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_OTHER_DIGEST,
                             'size': 96},
                            {'name': 'w',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE,
                             'digest': CANON,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_DIGEST}},
                            {'name': 'w.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_DIGEST,
                             'size': 96}]}),
                ('upload_blob_content', REPO, 'modelx.yaml', CONFIG_DIGEST, 29),
                ('upload_blob_content', REPO, 'o.leaves', LEAVES_OTHER_DIGEST, 96),
                ('upload_blob_content', REPO, 'w.leaves', LEAVES_DIGEST, 96)],
        stats=[{'phase': 'gpu-digest-batched', 'bytes': 5126, 'blobs': 2},
               {'phase': 'push-canonical-digest-batched', 'bytes': 5126},
               {'phase': 'push-upload', 'bytes': 2563, 'parts': 1},
               {'phase': 'push-upload', 'bytes': 2563, 'parts': 1}],
        unordered=True)


def test_push_one_tensor_canonical_digest(env):
    env.g.push_from_gpu(REPO, "v1", {"w": host(BLOB)}, chunk_size=CS,
                        digest_mode="sha256")
    env.expect(
        engine=[('push_part_from_device', 's3://w?part=0', 'PUT', {}, P, 2563),
                ('sha256_canonical_device', P, 2563),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_blob_location', REPO, 'modelx.yaml', 'upload', None),
                ('get_blob_location', REPO, 'w', 'upload', None),
                ('get_blob_location', REPO, 'w.leaves', 'upload', None),
                ('head_blob', REPO, CONFIG_DIGEST),
                ('head_blob', REPO, CANON),
                ('head_blob', REPO, LEAVES_DIGEST),
                ('put_manifest',
                 REPO,
                 'v1',
                 {'schemaVersion': 1,
                  'mediaType': types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
                  'config': {'name': 'modelx.yaml',
                             'mediaType': types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                             'digest': CONFIG_DIGEST,
                             'size': 29},
                  'blobs': [{'name': 'w',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE,
                             'digest': CANON,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_DIGEST}},
                            {'name': 'w.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_DIGEST,
                             'size': 96}]}),
                ('upload_blob_content', REPO, 'modelx.yaml', CONFIG_DIGEST, 29),
                ('upload_blob_content', REPO, 'w.leaves', LEAVES_DIGEST, 96)],
        stats=[{'phase': 'gpu-digest', 'bytes': 2563},
               {'phase': 'push-canonical-digest', 'bytes': 2563},
               {'phase': 'push-upload', 'bytes': 2563, 'parts': 1}],
        unordered=True)


def test_push_zstd_with_auto_planes(env):
    t = host(BLOB[:2562]).view(torch.int16)
    env.g.push_from_gpu(REPO, "v1", {"w": t}, chunk_size=CS, compress="zstd",
                        planes="auto")
    assert _uploaded(env, "w") == byte_planes(BLOB[:2562], 2, 2 * (128 << 10), False)
    env.expect(
        engine=[('byte_planes', [(P, P, 2562, 2, 262144)], False),
                ('push_part_from_device', 's3://w?part=0', 'PUT', {}, P, 2562),
                ('sha256_chunk_leaves', P, 2562, 1024),
                ('sha256_chunk_leaves', P, 2562, 1024),
                ('zstd_compress_device', P, 2562, 131072, P, 2626, True)],
        remote=[('get_blob_location', REPO, 'modelx.yaml', 'upload', None),
                ('get_blob_location', REPO, 'w', 'upload', None),
                ('get_blob_location', REPO, 'w.leaves', 'upload', None),
                ('head_blob', REPO, CONFIG_DIGEST),
                ('head_blob',
                 REPO,
                 'sha256:c4bd0c0259575d62adfba770641e9f230516633297eaebe6d192fcee6e13a989'),
                ('head_blob',
                 REPO,
                 'sha256c1k:1f7b435b6af3045248b14fc9409e61002e726b235999c6e4bcf1d893ec816606'),
                ('put_manifest',
                 REPO,
                 'v1',
                 {'schemaVersion': 1,
                  'mediaType': types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
                  'config': {'name': 'modelx.yaml',
                             'mediaType': types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                             'digest': CONFIG_DIGEST,
                             'size': 29},
                  'blobs': [{'name': 'w',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE_ZSTD,
                             'digest': 'sha256c1k:1f7b435b6af3045248b14fc9409e61002e726b235999c6e4bcf1d893ec816606',
                             'size': 2562,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: 'sha256c1k:1f7b435b6af3045248b14fc9409e61002e726b235999c6e4bcf1d893ec816606',
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: 'sha256:c4bd0c0259575d62adfba770641e9f230516633297eaebe6d192fcee6e13a989',
                                             types.ANNOTATION_RAW_DIGEST: 'sha256c1k:53335691c6dd54278b291b184bb45b981311b27b8d8fe440e811e634ed88be88',
                                             types.ANNOTATION_RAW_SIZE: '2562',
                                             types.ANNOTATION_BYTE_PLANES: '2:262144'}},
                            {'name': 'w.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': 'sha256:c4bd0c0259575d62adfba770641e9f230516633297eaebe6d192fcee6e13a989',
                             'size': 96}]}),
                ('upload_blob_content', REPO, 'modelx.yaml', CONFIG_DIGEST, 29),
                ('upload_blob_content',
                 REPO,
                 'w.leaves',
                 'sha256:c4bd0c0259575d62adfba770641e9f230516633297eaebe6d192fcee6e13a989',
                 96)],
        stats=[{'phase': 'gpu-digest', 'bytes': 2562},
               {'phase': 'push-byte-planes-split', 'bytes': 2562},
               {'phase': 'push-zstd-compress', 'bytes': 2562, 'compressed': 2562},
               {'phase': 'gpu-digest', 'bytes': 2562},
               {'phase': 'push-upload', 'bytes': 2562, 'parts': 1}],
        unordered=True)


def test_push_zstd_without_planes(env):
    env.g.push_from_gpu(REPO, "v1", {"w": host(BLOB)}, chunk_size=CS, compress="zstd")
    assert _uploaded(env, "w") == BLOB
    env.expect(
        engine=[('push_part_from_device', 's3://w?part=0', 'PUT', {}, P, 2563),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('sha256_chunk_leaves', P, 2563, 1024),
                ('zstd_compress_device', P, 2563, 131072, P, 2627, False)],
        remote=[('get_blob_location', REPO, 'modelx.yaml', 'upload', None),
                ('get_blob_location', REPO, 'w', 'upload', None),
                ('get_blob_location', REPO, 'w.leaves', 'upload', None),
                ('head_blob', REPO, CONFIG_DIGEST),
                ('head_blob', REPO, LEAVES_DIGEST),
                ('head_blob', REPO, ROOT),
                ('put_manifest',
                 REPO,
                 'v1',
                 {'schemaVersion': 1,
                  'mediaType': types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
                  'config': {'name': 'modelx.yaml',
                             'mediaType': types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                             'digest': CONFIG_DIGEST,
                             'size': 29},
                  'blobs': [{'name': 'w',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE_ZSTD,
                             'digest': ROOT,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_DIGEST,
                                             types.ANNOTATION_RAW_DIGEST: ROOT,
                                             types.ANNOTATION_RAW_SIZE: '2563'}},
                            {'name': 'w.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_DIGEST,
                             'size': 96}]}),
                ('upload_blob_content', REPO, 'modelx.yaml', CONFIG_DIGEST, 29),
                ('upload_blob_content', REPO, 'w.leaves', LEAVES_DIGEST, 96)],
        stats=[{'phase': 'gpu-digest', 'bytes': 2563},
               {'phase': 'push-zstd-compress', 'bytes': 2563, 'compressed': 2563},
               {'phase': 'gpu-digest', 'bytes': 2563},
               {'phase': 'push-upload', 'bytes': 2563, 'parts': 1}],
        unordered=True)


def test_push_three_parts(env):
    env.g.push_from_gpu(REPO, "v1", {"w": host(BLOB)}, chunk_size=CS, part_bytes=1000)
    assert _uploaded(env, "w", 3) == BLOB
    assert [len(env.eng.sink[f"s3://w?part={i}"]) for i in range(3)] == [854, 854, 855]
    env.expect(
        engine=[('push_part_from_device', 's3://w?part=0', 'PUT', {}, P, 854),
                ('push_part_from_device', 's3://w?part=1', 'PUT', {}, P, 854),
                ('push_part_from_device', 's3://w?part=2', 'PUT', {}, P, 855),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_blob_location', REPO, 'modelx.yaml', 'upload', None),
                ('get_blob_location',
                 REPO,
                 'w',
                 'upload',
                 {'part-count': '3', 'multipart': 'true'}),
                ('get_blob_location', REPO, 'w.leaves', 'upload', None),
                ('head_blob', REPO, CONFIG_DIGEST),
                ('head_blob', REPO, LEAVES_DIGEST),
                ('head_blob', REPO, ROOT),
                ('put_manifest',
                 REPO,
                 'v1',
                 {'schemaVersion': 1,
                  'mediaType': types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
                  'config': {'name': 'modelx.yaml',
                             'mediaType': types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                             'digest': CONFIG_DIGEST,
                             'size': 29},
                  'blobs': [{'name': 'w',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE,
                             'digest': ROOT,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_DIGEST}},
                            {'name': 'w.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_DIGEST,
                             'size': 96}]}),
                ('upload_blob_content', REPO, 'modelx.yaml', CONFIG_DIGEST, 29),
                ('upload_blob_content', REPO, 'w.leaves', LEAVES_DIGEST, 96)],
        stats=[{'phase': 'gpu-digest', 'bytes': 2563},
               {'phase': 'push-upload', 'bytes': 2563, 'parts': 3}],
        unordered=True)


def test_push_blob_already_present(env):
    env.rem.present.update((ROOT, CONFIG_DIGEST))
    env.g.push_from_gpu(REPO, "v1", {"w": host(BLOB)}, chunk_size=CS)
    assert env.eng.sink == {}
    env.expect(
        engine=[('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_blob_location', REPO, 'w.leaves', 'upload', None),
                ('head_blob', REPO, CONFIG_DIGEST),
                ('head_blob', REPO, LEAVES_DIGEST),
                ('head_blob', REPO, ROOT),
                ('put_manifest',
                 REPO,
                 'v1',
                 {'schemaVersion': 1,
                  'mediaType': types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
                  'config': {'name': 'modelx.yaml',
                             'mediaType': types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                             'digest': CONFIG_DIGEST,
                             'size': 29},
                  'blobs': [{'name': 'w',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE,
                             'digest': ROOT,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_DIGEST}},
                            {'name': 'w.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_DIGEST,
                             'size': 96}]}),
                ('upload_blob_content', REPO, 'w.leaves', LEAVES_DIGEST, 96)],
        stats=[{'phase': 'gpu-digest', 'bytes': 2563}],
        unordered=True)


def test_push_redirectless_registry(env):
    env.rem.redirect = False
    env.g.slot_bytes = 1000
    env.g.push_from_gpu(REPO, "v1", {"w": host(BLOB)}, chunk_size=CS)
    assert env.rem.uploaded == {CONFIG_DIGEST: CONFIG, LEAVES_DIGEST: LEAVES, ROOT: BLOB}
    env.expect(
        engine=[('read_device', P, 1000),
                ('read_device', P, 1000),
                ('read_device', P, 563),
                ('sha256_chunk_leaves', P, 2563, 1024)],
        remote=[('get_blob_location', REPO, 'modelx.yaml', 'upload', None),
                ('get_blob_location', REPO, 'w', 'upload', None),
                ('get_blob_location', REPO, 'w.leaves', 'upload', None),
                ('head_blob', REPO, CONFIG_DIGEST),
                ('head_blob', REPO, LEAVES_DIGEST),
                ('head_blob', REPO, ROOT),
                ('put_manifest',
                 REPO,
                 'v1',
                 {'schemaVersion': 1,
                  'mediaType': types.MEDIA_TYPE_MODEL_MANIFEST_JSON,
                  'config': {'name': 'modelx.yaml',
                             'mediaType': types.MEDIA_TYPE_MODEL_CONFIG_YAML,
                             'digest': CONFIG_DIGEST,
                             'size': 29},
                  'blobs': [{'name': 'w',
                             'mediaType': types.MEDIA_TYPE_MODEL_FILE,
                             'digest': ROOT,
                             'size': 2563,
                             'annotations': {types.ANNOTATION_CHUNK_DIGEST: ROOT,
                                             types.ANNOTATION_CHUNK_SIZE: '1024',
                                             types.ANNOTATION_LEAVES_BLOB: LEAVES_DIGEST}},
                            {'name': 'w.leaves',
                             'mediaType': types.MEDIA_TYPE_MODEL_LEAVES,
                             'digest': LEAVES_DIGEST,
                             'size': 96}]}),
                ('upload_blob_content', REPO, 'modelx.yaml', CONFIG_DIGEST, 29),
                ('upload_blob_content', REPO, 'w', ROOT, 2563),
                ('upload_blob_content', REPO, 'w.leaves', LEAVES_DIGEST, 96)],
        stats=[{'phase': 'gpu-digest', 'bytes': 2563},
               {'phase': 'push-registry-stream', 'bytes': 2563}],
        unordered=True)


def test_push_registers_chunks_when_dedup_is_on(env):
    env.g.dedup = True
    env.g.push_from_gpu(REPO, "v1", {"w": host(BLOB)}, chunk_size=CS)
    env.g.push_from_gpu(REPO, "v2", {"w": host(BLOB), "o": host(OTHER)}, chunk_size=CS)
    assert [c for c in env.eng.calls if c[0] == "dedup_register"] == [
        ("dedup_register", 96, P, CS, 2563)] * 3
    assert len(env.g._dedup_tensors) == 3


@pytest.mark.parametrize("dirs, message", [
    ({"a/b": {}}, "directory name 'a/b' contains '/'"),
    ({"w.leaves": {}}, "directory 'w.leaves': the name 'w.leaves' is already used by "
                       "another blob of this push"),
])
def test_push_bad_directory_names(env, dirs, message):
    with pytest.raises(ValueError) as ei:
        env.g.push_from_gpu(REPO, "v1", {"w": host(BLOB)}, chunk_size=CS, dirs=dirs)
    assert str(ei.value) == message
    env.expect(engine=[], remote=[], stats=[])

