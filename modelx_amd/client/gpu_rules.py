"""The rules of the GPU data plane, each written once.

Pure functions over descriptors, manifests and sizes: no engine, no network,
no torch. ``gpu.py`` decides nothing about a descriptor that is not asked
here, so a rule read in two places cannot drift apart.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

from ..wire import digest as dg
from ..wire import errors as er
from ..wire import types

# 128 KiB chunks put 65k+ SHA-256 chains in flight for multi-GiB blobs — the
# measured sweet spot on MI355X (1017 GiB/s vs 147 GiB/s at 1 MiB chunks,
# profiles/sha256_kernel.md)
DEFAULT_GPU_CHUNK = 128 << 10

DIR_MEDIA_TYPES = (types.MEDIA_TYPE_MODEL_DIRECTORY_TAR,
                   types.MEDIA_TYPE_MODEL_DIRECTORY_TARGZ)


def leaves_usable(leaves, size: int, chunk_size) -> bool:
    """Whether ``leaves`` is the packed 32 B/leaf array of a ``size``-byte
    blob at ``chunk_size``: a positive integer chunk size and exactly one
    leaf per chunk (one leaf for an empty blob). Leaves and the chunk size
    arrive from the remote; the device kernels address chunk ``i`` at
    ``i * chunk_size``, so a leaf too many is a write past the tensor.
    Callers treat unusable leaves like a missing sidecar."""
    if isinstance(chunk_size, bool) or not isinstance(chunk_size, int) or chunk_size <= 0:
        return False
    if not isinstance(leaves, (bytes, bytearray, memoryview)):
        return False
    if isinstance(size, bool) or not isinstance(size, int) or size < 0:
        return False
    want = (size - 1) // chunk_size + 1 if size else 1
    return len(leaves) == 32 * want


def annotated_chunk_size(desc: types.Descriptor) -> int:
    """The chunk-size annotation as a positive integer, or 0 when it is
    absent or anything else (the caller then falls back as for an absent
    one)."""
    note = desc.annotations.get(types.ANNOTATION_CHUNK_SIZE, "")
    if isinstance(note, bool):
        return 0
    if isinstance(note, int):
        return note if note > 0 else 0
    if isinstance(note, str) and note.isascii() and note.isdigit():
        return int(note)
    return 0


def _digest_chunk_size(digest: str) -> Optional[int]:
    """The chunk size a chunked digest string names, None for any other."""
    return dg.algo_chunk_size(digest.split(":", 1)[0]) if digest else None


def chunk_digest_note(desc: types.Descriptor) -> str:
    return desc.annotations.get(types.ANNOTATION_CHUNK_DIGEST, "")


def chunked_target(desc: types.Descriptor) -> Optional[Tuple[str, int]]:
    """The chunked digest a landed blob is verified against, with the chunk
    size that digest names: the main digest when it is chunked, else the
    chunk-digest annotation; None when the descriptor is canonical-only."""
    cs = _digest_chunk_size(desc.digest)
    if cs:
        return desc.digest, cs
    note = chunk_digest_note(desc)
    if note:
        return note, _digest_chunk_size(note) or dg.DEFAULT_CHUNK_SIZE
    return None


def leaf_chunk_size(desc: types.Descriptor) -> int:
    """The chunk size of a blob's leaves sidecar, which is also the size the
    transfer paths hash at: the chunk-size annotation, else the one the main
    digest names, else the GPU default."""
    return (annotated_chunk_size(desc) or _digest_chunk_size(desc.digest)
            or DEFAULT_GPU_CHUNK)


def raw_size_or_zero(desc: types.Descriptor) -> int:
    """Uncompressed size of a +zstd blob, 0 when the annotation is absent:
    for sizing that sums before anything is checked."""
    return int(desc.annotations.get(types.ANNOTATION_RAW_SIZE, 0) or 0)


def raw_size(desc: types.Descriptor) -> int:
    """Uncompressed size of a +zstd blob; the decoder needs it."""
    size = raw_size_or_zero(desc)
    if not size:
        raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                             f"+zstd blob {desc.name} lacks the raw-size annotation")
    return size


def raw_target(desc: types.Descriptor) -> Optional[Tuple[str, int]]:
    """The chunked digest of a +zstd blob's uncompressed bytes with its
    chunk size, None when the descriptor carries none."""
    digest = desc.annotations.get(types.ANNOTATION_RAW_DIGEST, "")
    if not digest:
        return None
    return digest, _digest_chunk_size(digest) or DEFAULT_GPU_CHUNK


def byte_planes(desc: types.Descriptor) -> Optional[tuple]:
    """``(E, G)`` of the byte-planes annotation or None; a malformed one
    raises UNSUPPORTED (``types.parse_byte_planes``)."""
    return types.parse_byte_planes(desc.annotations.get(types.ANNOTATION_BYTE_PLANES))


def zstd_waves(jobs: list, cap: int) -> List[list]:
    """Batched-decode jobs ``(key, desc, plan_entry)`` in waves of at most
    ``cap`` raw bytes, so compressed+raw residency stays bounded. A job
    larger than the cap is a wave of its own."""
    if len(jobs) < 2 or sum(raw_size_or_zero(d) for _, d, _ in jobs) <= cap:
        return [jobs]
    waves, wave, acc = [], [], 0
    for job in jobs:
        raw = raw_size_or_zero(job[1])
        if wave and acc + raw > cap:
            waves.append(wave)
            wave, acc = [], 0
        wave.append(job)
        acc += raw
    waves.append(wave)
    return waves


def payload_descriptors(manifest: types.Manifest,
                        skip_sidecars: bool = True) -> List[types.Descriptor]:
    """The blobs of a manifest a pull lands: non-empty, and no leaves
    sidecar (those are read on demand, never landed as payload)."""
    return [d for d in manifest.blobs
            if d.size and not (skip_sidecars
                               and d.media_type == types.MEDIA_TYPE_MODEL_LEAVES)]


def split_payloads(descs, expand_dirs: bool = False) -> Tuple[list, list, list]:
    """(zstd, directory, plain) descriptors. Directory blobs count as plain
    (landed as raw archive bytes) unless ``expand_dirs``."""
    zstd = [d for d in descs if d.media_type == types.MEDIA_TYPE_MODEL_FILE_ZSTD]
    rest = [d for d in descs if d.media_type != types.MEDIA_TYPE_MODEL_FILE_ZSTD]
    if not expand_dirs:
        return zstd, [], rest
    return (zstd, [d for d in rest if d.media_type in DIR_MEDIA_TYPES],
            [d for d in rest if d.media_type not in DIR_MEDIA_TYPES])


def part_ranges(size: int, nparts: int) -> List[Tuple[int, int]]:
    """(offset, length) of each part of a multipart push: equal parts, the
    last one takes the remainder."""
    base = size // nparts
    return [(i * base, base if i < nparts - 1 else size - i * base)
            for i in range(nparts)]


def check_dir_names(tensors, dirs) -> None:
    """Every descriptor name the manifest of a push will carry must be
    unique: the config, each blob and each blob's leaves sidecar."""
    taken = {"modelx.yaml"}
    for tname in tensors:
        taken.update((tname, tname + ".leaves"))
    for dname in dirs:
        if "/" in dname:
            raise ValueError(f"directory name {dname!r} contains '/'")
        for n in (dname, dname + ".leaves"):
            if n in taken:
                raise ValueError(f"directory {dname!r}: the name {n!r} is "
                                 "already used by another blob of this push")
        taken.update((dname, dname + ".leaves"))
