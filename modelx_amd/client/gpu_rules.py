"""The rules of the GPU data plane, each written once.

Pure functions over descriptors, manifests and sizes: no engine, no network,
no torch. ``gpu.py`` decides nothing about a descriptor that is not asked
here, so a rule read in two places cannot drift apart.
"""
from __future__ import annotations

import base64
import struct
from typing import Dict, List, Optional, Tuple

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


# Content-defined chunking (core/include/modelx/cdc_core.hpp): (min, bits, max)
CDC_DEFAULTS = (32 << 10, 16, 256 << 10)
CDC_MAGIC = b"MXCDC1\0\0"
_CDC_HEADER = struct.Struct("<8sIIII")
_CDC_RECORD = 4 + 32


def _cdc_valid(params) -> bool:
    if not isinstance(params, (tuple, list)) or len(params) != 3:
        return False
    if any(isinstance(v, bool) or not isinstance(v, int) for v in params):
        return False
    lo, bits, hi = params
    return 64 <= lo <= hi <= (16 << 20) and 1 <= bits <= 24


def cdc_params(cdc) -> Optional[Tuple[int, int, int]]:
    """The ``cdc`` option of ``GpuClient`` and ``push_from_gpu``: ``False``
    or ``None`` (off, returns None), ``True`` (the defaults) or
    ``(min, bits, max)``; invalid parameters are UNSUPPORTED."""
    if cdc is None or cdc is False:
        return None
    if cdc is True:
        return CDC_DEFAULTS
    if not _cdc_valid(cdc):
        raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                             f"unsupported cdc parameters {cdc!r}: need (min, bits, max) with "
                             "64 <= min <= max <= 16 MiB and 1 <= bits <= 24")
    return tuple(cdc)


def cdc_sidecar(params, ranges, digests: bytes) -> bytes:
    """The CDC sidecar body: header (magic, min, max, bits, count), then per
    chunk its length and SHA-256. ``ranges`` are the blob's (offset, length)
    chunks in order; offsets are implied by the lengths."""
    lo, bits, hi = params
    assert len(digests) == 32 * len(ranges)
    out = [_CDC_HEADER.pack(CDC_MAGIC, lo, hi, bits, len(ranges))]
    for i, (_, ln) in enumerate(ranges):
        out.append(struct.pack("<I", ln) + digests[32 * i:32 * i + 32])
    return b"".join(out)


def cdc_usable(data, sidecar_digest: str, size: int):
    """``(params, ranges, digests)`` of a CDC sidecar that describes a
    ``size``-byte blob, else None. The sidecar arrives from the remote and its
    ranges become device writes, so it counts as absent (the pull takes the
    next strategy) unless its digest matches, its magic and parameters are
    valid, every length is in 1..max and the lengths sum to ``size``."""
    if not isinstance(data, (bytes, bytearray)) or not sidecar_digest:
        return None
    if dg.sha256_digest(bytes(data)) != sidecar_digest:
        return None
    if len(data) < _CDC_HEADER.size:
        return None
    magic, lo, hi, bits, count = _CDC_HEADER.unpack_from(data)
    if magic != CDC_MAGIC or not _cdc_valid((lo, bits, hi)):
        return None
    if len(data) != _CDC_HEADER.size + count * _CDC_RECORD:
        return None
    ranges, digests, off = [], [], 0
    for i in range(count):
        at = _CDC_HEADER.size + i * _CDC_RECORD
        ln, = struct.unpack_from("<I", data, at)
        if ln == 0 or ln > hi:
            return None
        ranges.append((off, ln))
        digests.append(bytes(data[at + 4:at + _CDC_RECORD]))
        off += ln
    if off != size:
        return None
    return (lo, bits, hi), ranges, b"".join(digests)


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
    """The blobs of a manifest a pull lands: non-empty, and no leaves or
    CDC sidecar (those are read on demand, never landed as payload)."""
    return [d for d in manifest.blobs
            if d.size and not (skip_sidecars
                               and d.media_type in types.SIDECAR_MEDIA_TYPES)]


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


PART_CHECKSUM_HEADER = "x-amz-checksum-crc32c"


def check_part_checksum(part_checksum) -> None:
    """The ``part_checksum`` option of a GPU push: ``""`` (none) or
    ``"crc32c"``; anything else is UNSUPPORTED."""
    if part_checksum not in ("", "crc32c"):
        raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                             f"unknown part_checksum {part_checksum!r} "
                             "(supported: '' and 'crc32c')")


def check_dir_format(dir_format, dirs, cdc) -> None:
    """The ``dir_format`` option of a GPU push: ``"tar"`` or ``"tar+gz"``.
    ``"tar+gz"`` needs ``dirs`` and excludes ``cdc``, for the reason ``cdc``
    excludes ``compress``; anything else is UNSUPPORTED."""
    if dir_format not in ("tar", "tar+gz"):
        raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                             f"unknown dir_format {dir_format!r} "
                             "(supported: 'tar' and 'tar+gz')")
    if dir_format == "tar+gz":
        if not dirs:
            raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                                 "dir_format='tar+gz' needs dirs")
        if cdc:
            raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                                 "cdc cannot be combined with dir_format='tar+gz': "
                                 "chunking compressed bytes finds no shifted content")


def part_checksum_headers(crc: int) -> Dict[str, str]:
    """The upload header that carries a CRC-32C value: base64 of its four
    bytes, most significant first, as S3 reads ``x-amz-checksum-crc32c``."""
    return {PART_CHECKSUM_HEADER: base64.b64encode(crc.to_bytes(4, "big")).decode()}


# ---- client-side encryption (core/include/modelx/aead_core.hpp) ------------

_BLOB_KEY_LABEL = b"modelx-aead-v1\0"


def check_encrypt_key(key) -> None:
    """The ``key`` option of the clients: ``None`` or 32 bytes; anything
    else is UNSUPPORTED."""
    if key is not None and not (isinstance(key, (bytes, bytearray)) and len(key) == 32):
        raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                             "the encryption key must be 32 bytes (or None)")


def check_gpu_gunzip(value):
    """The ``gpu_gunzip`` option of GpuClient: ``False``, ``True`` (members
    that fall apart at sync markers) or ``"any"`` (also stock streams, by
    block search); anything else is UNSUPPORTED."""
    if value is False or value is True or value == "any":
        return value
    raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                         "gpu_gunzip must be False, True or \"any\"")


def encrypt_segment(seg) -> int:
    """The ``encrypt_segment`` option of a push: ``None`` (the default) or a
    multiple of 1024 from 1024 to 16 MiB; anything else is UNSUPPORTED."""
    if seg is None:
        return types.ENCRYPTION_DEFAULT_SEGMENT
    if not types.encryption_segment_ok(seg):
        raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                             f"unsupported encrypt_segment {seg!r}: need a multiple of "
                             "1024 from 1024 to 16 MiB")
    return seg


def sealed_size(n: int, seg: int) -> int:
    """Stored size of ``n`` sealed bytes: one 16-byte tag per segment."""
    return types.sealed_size(n, seg)


def blob_key(key: bytes, salt: bytes, seg: int, n: int) -> bytes:
    """The key one blob is sealed under. It binds the salt, the segment size
    and the length, so an annotation that was tampered with derives another
    key and every tag fails. The engine never sees the user's key."""
    import hashlib
    import hmac

    return hmac.new(bytes(key), _BLOB_KEY_LABEL + salt + struct.pack("<IQ", seg, n),
                    hashlib.sha256).digest()


def encryption_note(seg: int, n: int, salt: bytes) -> Dict[str, str]:
    """The annotation a sealed blob's descriptor carries."""
    return {types.ANNOTATION_ENCRYPTION: types.format_encryption(seg, n, salt)}


def encryption(desc: types.Descriptor) -> Optional[tuple]:
    """``(seg, n, salt)`` of a sealed blob or None; a malformed annotation,
    or one that does not fit the descriptor's size, raises UNSUPPORTED
    (``types.parse_encryption``)."""
    return types.parse_encryption(desc.annotations.get(types.ANNOTATION_ENCRYPTION), desc.size)


def opening_key(desc: types.Descriptor, key, what: str = "pull") -> Optional[tuple]:
    """``(blob key, seg, n)`` to open ``desc`` with, None for a blob that is
    not sealed. A sealed blob without a key is UNSUPPORTED: its stored bytes
    are never returned as content."""
    enc = encryption(desc)
    if enc is None:
        return None
    if key is None:
        raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                             f"{what}: blob {desc.name} is encrypted and no key was given")
    seg, n, salt = enc
    return blob_key(key, salt, seg, n), seg, n


def dedup_allowed(desc: types.Descriptor) -> bool:
    """Whether a landed blob may be registered in, or gathered from, the
    chunk-dedup table. A sealed blob may not: it is opened in place, which
    would rewrite chunks the table holds as resident."""
    return not desc.annotations.get(types.ANNOTATION_ENCRYPTION)


def refuse_sealed(descs, what: str) -> None:
    """UNSUPPORTED when any of ``descs`` is sealed: for paths that move
    stored bytes between devices and have no step that opens them."""
    for desc in descs:
        if desc.annotations.get(types.ANNOTATION_ENCRYPTION):
            raise er.ModelxError(er.ErrCode.UNSUPPORTED,
                                 f"{what}: blob {desc.name} is encrypted; pull it with "
                                 "GpuClient(key=...).pull_to_gpu")


def bad_tag(desc: types.Descriptor, segment: int) -> er.ModelxError:
    return er.ModelxError(er.ErrCode.DIGEST_INVALID,
                          f"authentication failed for {desc.name}: tag mismatch in "
                          f"segment {segment} (wrong key or altered blob)")


def check_dir_names(tensors, dirs, cdc: bool = False) -> None:
    """Every descriptor name the manifest of a push will carry must be
    unique: the config, each blob and each blob's leaves sidecar (and its
    CDC sidecar in a push with ``cdc``)."""
    suffixes = ("", ".leaves", ".cdc") if cdc else ("", ".leaves")
    taken = {"modelx.yaml"}
    for tname in tensors:
        taken.update(tname + sfx for sfx in suffixes)
    for dname in dirs:
        if "/" in dname:
            raise ValueError(f"directory name {dname!r} contains '/'")
        for n in (dname + sfx for sfx in suffixes):
            if n in taken:
                raise ValueError(f"directory {dname!r}: the name {n!r} is "
                                 "already used by another blob of this push")
        taken.update(dname + sfx for sfx in suffixes)
