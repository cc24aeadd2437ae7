"""Seekable-zstd test blobs with a damaged tail, shared by the CPU parser
tests (test_zstd.py) and the device-path tests (test_gpu_kernels.py).

Tail layout of a blob with n frames and no per-frame checksums:

    [0x184D2A5E u32][n*8+9 u32]  skippable-frame envelope
    n x [c_size u32][d_size u32] entries
    [n u32][descriptor u8][0x8F92EAB1 u32]  footer
"""
import struct

from modelx_amd import _core

FRAME_RAW = 4 << 10


def three_frame_blob():
    """(data, blob): 10 KiB in 4 KiB frames -> 3 frames."""
    data = bytes((i * 7 + i // 251) & 0xFF for i in range(10 << 10))
    blob = _core.zstd_compress_cpu(data, FRAME_RAW)
    assert len(_core.zstd_frames(blob)) == 3
    return data, blob


def _table_start(blob: bytes) -> int:
    (n,) = struct.unpack_from("<I", blob, len(blob) - 9)
    return len(blob) - (8 + n * 8 + 9)


def _flip(blob: bytes, pos: int) -> bytes:
    b = bytearray(blob)
    b[pos] ^= 0xFF
    return bytes(b)


def _add32(blob: bytes, pos: int, delta: int) -> bytes:
    b = bytearray(blob)
    (v,) = struct.unpack_from("<I", b, pos)
    struct.pack_into("<I", b, pos, v + delta)
    return bytes(b)


def corruptions(blob: bytes) -> dict:
    """name -> corrupt blob; every one must be refused by the strict parser."""
    t = _table_start(blob)
    b = bytearray(blob)
    struct.pack_into("<I", b, len(b) - 9, len(b))  # 8 + len*8 + 9 > len
    return {
        "truncated-16": blob[:16],
        "footer-magic": _flip(blob, len(blob) - 1),
        "nframes-exceeds-blob": bytes(b),
        "envelope-magic": _flip(blob, t),
        "envelope-length": _add32(blob, t + 4, 1),
        "entry-csize": _add32(blob, t + 8, 1),
    }


def with_checksum_flag(blob: bytes) -> bytes:
    """Same frames, table rewritten with descriptor bit 7 set and 12-byte
    entries (a zero checksum appended to each)."""
    t = _table_start(blob)
    (n,) = struct.unpack_from("<I", blob, len(blob) - 9)
    out = bytearray(blob[:t])
    out += struct.pack("<II", 0x184D2A5E, n * 12 + 9)
    for i in range(n):
        out += blob[t + 8 + i * 8 : t + 16 + i * 8] + b"\0\0\0\0"
    out += struct.pack("<IB", n, blob[-5] | 0x80) + blob[-4:]
    return bytes(out)
