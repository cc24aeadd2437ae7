"""Foreign zstd frames for the decoder tests: a seeded payload corpus encoded
by the system libzstd, a wrapper that turns such frames into a seekable blob,
and a frame walker that reports which RFC 8878 constructs a frame contains.

Our own encoder writes a narrow dialect (raw or Huffman literals, predefined
sequence tables, single-segment headers, no checksum), so a decoder fed only
its output never runs the rest of the format. The corpus here is chosen so
that libzstd emits the rest, and `walk` exists so the tests can prove that it
did (REQUIRED below) instead of trusting the installed libzstd to behave like
the one the corpus was designed against.

Needs neither torch nor the extension. The seekable tail that `wrap_seekable`
appends is described once, at the top of util_seek.py.
"""
import collections
import ctypes
import functools
import random
import struct

MAGIC = b"\x28\xb5\x2f\xfd"
LEVELS = (1, 3, 9, 19)

# ZSTD_cParameter ids of the advanced API
_C_LEVEL, _C_WINDOW_LOG, _C_CONTENT_SIZE, _C_CHECKSUM = 100, 101, 200, 201


# ------------------------------------------------------------- libzstd -----

@functools.lru_cache(maxsize=None)
def libzstd():
    z = ctypes.CDLL("libzstd.so.1")
    for fn in ("ZSTD_compressBound", "ZSTD_compress", "ZSTD_compress2", "ZSTD_decompress",
               "ZSTD_CCtx_setParameter", "ZSTD_freeCCtx"):
        getattr(z, fn).restype = ctypes.c_size_t
    z.ZSTD_isError.restype = ctypes.c_uint
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_versionString.restype = ctypes.c_char_p
    return z


def libzstd_version() -> str:
    return libzstd().ZSTD_versionString().decode()


def compress(data: bytes, level: int) -> bytes:
    """One frame from ZSTD_compress."""
    z = libzstd()
    bound = z.ZSTD_compressBound(ctypes.c_size_t(len(data)))
    dst = ctypes.create_string_buffer(bound)
    n = z.ZSTD_compress(dst, ctypes.c_size_t(bound), data, ctypes.c_size_t(len(data)),
                        ctypes.c_int(level))
    assert not z.ZSTD_isError(ctypes.c_size_t(n)), f"ZSTD_compress rc {n}"
    return dst.raw[:n]


def compress_advanced(data: bytes, level: int, *, checksum=False, content_size=True,
                      window_log=None) -> bytes:
    """One frame from ZSTD_compress2 with the header variants set."""
    z = libzstd()
    cctx = ctypes.c_void_p(z.ZSTD_createCCtx())
    assert cctx.value
    try:
        params = [(_C_LEVEL, level), (_C_CHECKSUM, int(checksum)),
                  (_C_CONTENT_SIZE, int(content_size))]
        if window_log is not None:
            params.append((_C_WINDOW_LOG, window_log))
        for pid, val in params:
            rc = z.ZSTD_CCtx_setParameter(cctx, ctypes.c_int(pid), ctypes.c_int(val))
            assert not z.ZSTD_isError(ctypes.c_size_t(rc)), (pid, val)
        bound = z.ZSTD_compressBound(ctypes.c_size_t(len(data)))
        dst = ctypes.create_string_buffer(bound)
        n = z.ZSTD_compress2(cctx, dst, ctypes.c_size_t(bound), data,
                             ctypes.c_size_t(len(data)))
        assert not z.ZSTD_isError(ctypes.c_size_t(n)), f"ZSTD_compress2 rc {n}"
        return dst.raw[:n]
    finally:
        z.ZSTD_freeCCtx(cctx)


def decompress(blob: bytes, raw_len: int) -> bytes:
    """libzstd's decode of one frame, or of a whole multi-frame blob (it skips
    the seek table's skippable frame)."""
    z = libzstd()
    out = ctypes.create_string_buffer(max(raw_len, 1))
    m = z.ZSTD_decompress(out, ctypes.c_size_t(raw_len), blob, ctypes.c_size_t(len(blob)))
    assert not z.ZSTD_isError(ctypes.c_size_t(m)), f"ZSTD_decompress rc {m}"
    return out.raw[:m]


# ------------------------------------------------------- seekable wrapper --

def wrap_seekable(frames, d_sizes) -> bytes:
    """Concatenate frames and append the seek table (layout: util_seek.py)."""
    frames = list(frames)
    d_sizes = list(d_sizes)
    assert len(frames) == len(d_sizes)
    n = len(frames)
    out = bytearray().join(frames)
    out += struct.pack("<II", 0x184D2A5E, n * 8 + 9)
    for f, d in zip(frames, d_sizes):
        out += struct.pack("<II", len(f), d)
    out += struct.pack("<IBI", n, 0, 0x8F92EAB1)
    return bytes(out)


def tiling(frames, d_sizes):
    """The (c_off, c_size, d_off, d_size) list a seek table of these frames
    must parse to."""
    out, c, d = [], 0, 0
    for f, ds in zip(frames, d_sizes):
        out.append((c, len(f), d, ds))
        c += len(f)
        d += ds
    return out


# ----------------------------------------------------------- frame walker --

_SEQ_MODE = ("predefined", "rle", "fse", "repeat")


def _walk_block(b: bytes, found) -> None:
    b0 = b[0]
    lit_type, size_fmt = b0 & 3, (b0 >> 2) & 3
    if lit_type < 2:  # raw / RLE literals
        if size_fmt in (0, 2):
            regen, hdr = b0 >> 3, 1
        elif size_fmt == 1:
            regen, hdr = (b0 >> 4) | (b[1] << 4), 2
        else:
            regen, hdr = (b0 >> 4) | (b[1] << 4) | (b[2] << 12), 3
        found["lit:raw" if lit_type == 0 else "lit:rle"] += 1
        pos = hdr + (regen if lit_type == 0 else 1)
    else:  # Huffman with a fresh table / treeless
        hdr = (3, 3, 4, 5)[size_fmt]
        v = int.from_bytes(b[:hdr], "little")
        comp = (v >> (14, 14, 18, 22)[size_fmt]) & (0x3FF, 0x3FF, 0x3FFF, 0x3FFFF)[size_fmt]
        streams = 1 if size_fmt == 0 else 4
        found["lit:%s-%d" % ("huffman" if lit_type == 2 else "treeless", streams)] += 1
        if lit_type == 2:
            found["weights:direct" if b[hdr] >= 128 else "weights:fse"] += 1
        pos = hdr + comp
    sb = b[pos]
    if sb < 128:
        nseq, pos = sb, pos + 1
    elif sb < 255:
        nseq, pos = ((sb - 128) << 8) + b[pos + 1], pos + 2
    else:
        nseq, pos = b[pos + 1] + (b[pos + 2] << 8) + 0x7F00, pos + 3
    if nseq == 0:
        found["nseq=0"] += 1
        assert pos == len(b), "bytes after an all-literals block"
        return
    modes = b[pos]
    assert modes & 3 == 0
    for kind, shift in (("ll", 6), ("of", 4), ("ml", 2)):
        found["%s:%s" % (kind, _SEQ_MODE[(modes >> shift) & 3])] += 1


def walk(frame: bytes) -> collections.Counter:
    """Which constructs one zstd frame contains, as a Counter of names (the
    vocabulary is REQUIRED plus lit:rle, lit:huffman-1, ll:rle, of:rle,
    hdr:no-content-size, block:compressed). Decodes no payload; asserts that
    the block chain ends exactly at the end of the frame."""
    found = collections.Counter()
    assert frame[:4] == MAGIC, "not a zstd frame"
    fhd = frame[4]
    single, fcs_flag = (fhd >> 5) & 1, fhd >> 6
    found["hdr:single-segment" if single else "hdr:window-descriptor"] += 1
    if fhd & 4:
        found["hdr:checksum"] += 1
    if fcs_flag == 0 and not single:
        found["hdr:no-content-size"] += 1
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3]
    pos += (1 if single else 0, 2, 4, 8)[fcs_flag]
    nblocks = 0
    while True:
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        pos += 3
        last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
        nblocks += 1
        if btype == 0:
            found["block:raw"] += 1
            pos += bsize
        elif btype == 1:
            found["block:rle"] += 1
            pos += 1
        else:
            assert btype == 2, "reserved block type"
            found["block:compressed"] += 1
            _walk_block(frame[pos:pos + bsize], found)
            pos += bsize
        if last:
            break
    if nblocks >= 4:
        found["frame:>=4-blocks"] += 1
    if fhd & 4:
        pos += 4
    assert pos == len(frame), "block chain does not end at the end of the frame"
    return found


# What the corpus as a whole must reach (the decoder paths our own encoder
# never produces, plus the ones it does). Not required, because no libzstd
# level emitted them for these payloads: lit:rle, lit:huffman-1 (a fresh
# 1-stream table), ll:rle, of:rle.
REQUIRED = (
    "block:raw", "block:rle", "frame:>=4-blocks",
    "lit:raw", "lit:huffman-4", "lit:treeless-4", "lit:treeless-1",
    "weights:direct", "weights:fse", "nseq=0",
    "ll:predefined", "ll:fse", "ll:repeat",
    "of:predefined", "of:fse", "of:repeat",
    "ml:predefined", "ml:fse", "ml:repeat", "ml:rle",
    "hdr:single-segment", "hdr:window-descriptor", "hdr:checksum",
)


# ----------------------------------------------------------------- corpus --

def lz_repeats(seed: int, size: int, max_off: int, alphabet: int) -> bytes:
    """Random literal runs mixed with copies from up to max_off bytes back
    (the generator of test_zstd.py::_payloads, parametrised)."""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < size:
        if rng.random() < 0.6 and len(out) > 64:
            off = rng.randrange(1, min(len(out), max_off))
            start = len(out) - off
            ln = rng.randrange(4, 300)
            if ln <= off:
                out += out[start:start + ln]
            else:  # the copy overlaps its own output
                for k in range(ln):
                    out.append(out[start + k])
        else:
            n = rng.randrange(1, 50)
            out.extend(rng.randbytes(n) if alphabet == 256
                       else bytes(rng.randrange(alphabet) for _ in range(n)))
    return bytes(out[:size])


def bf16_bytes(seed: int, nbytes: int) -> bytes:
    """Little-endian bf16 bytes of N(0, 0.02) samples (truncated float32)."""
    import numpy as np

    x = np.random.default_rng(seed).normal(0.0, 0.02, nbytes // 2).astype(np.float32)
    return (x.view(np.uint32) >> 16).astype("<u2").tobytes()


@functools.lru_cache(maxsize=None)
def payloads() -> dict:
    rng = random.Random(20240229)
    runs = bytearray()
    for _ in range(20_000):
        runs += bytes([rng.randrange(256)]) * rng.randrange(1, 40)
    return {
        "text": b"the quick brown fox jumps over the lazy dog " * 7000,
        "repeats": lz_repeats(1234, 300_000, 60_000, 256),
        "far-offsets": lz_repeats(4321, 400_000, 390_000, 64),
        "aab": bytes(rng.choice(b"aab") for _ in range(140_000)),
        "sym64": bytes(rng.randrange(64) for _ in range(300_000)),
        "zeros": bytes(300_000),
        "random": rng.randbytes(200_000),
        "bf16": bf16_bytes(7, 400_000),
        "runs": bytes(runs),
        "abc-splice": b"abc" * 50_000 + rng.randbytes(100) + b"abc" * 50_000,
        "empty": b"",
        "one-byte": b"a",
        "random-63": rng.randbytes(63),
        "shrdlu-900": bytes(rng.choice(b"etaoin shrdlu") for _ in range(900)),
    }


Item = collections.namedtuple("Item", "name variant payload frame")

# header variants through the advanced API: (variant name, kwargs)
_ADVANCED = (
    ("checksum", dict(checksum=True)),
    ("checksum+window17", dict(checksum=True, content_size=False, window_log=17)),
)


PAYLOAD_NAMES = ("text", "repeats", "far-offsets", "aab", "sym64", "zeros", "random", "bf16",
                 "runs", "abc-splice", "empty", "one-byte", "random-63", "shrdlu-900")


def corpus_keys() -> tuple:
    """(name, variant) of every corpus frame, in corpus order, without
    generating or encoding anything (for test ids at collection time).
    Level-major, so that the zero-length frames each sit between non-empty
    neighbours."""
    keys = []
    for level in LEVELS:
        keys += [(name, "L%d" % level) for name in PAYLOAD_NAMES]
        if level in (1, 19):
            keys += [(name, "L%d+%s" % (level, vname))
                     for name in ("far-offsets", "shrdlu-900") for vname, _ in _ADVANCED]
    return tuple(keys)


@functools.lru_cache(maxsize=None)
def corpus() -> tuple:
    """One Item per corpus_keys() entry. Encoded once per process."""
    p = payloads()
    assert tuple(p) == PAYLOAD_NAMES
    adv = dict(_ADVANCED)
    items = []
    for name, variant in corpus_keys():
        level, _, vname = variant[1:].partition("+")
        frame = (compress_advanced(p[name], int(level), **adv[vname]) if vname
                 else compress(p[name], int(level)))
        items.append(Item(name, variant, p[name], frame))
    return tuple(items)


def coverage(items=None) -> collections.Counter:
    total = collections.Counter()
    for it in (corpus() if items is None else items):
        total += walk(it.frame)
    return total


def corpus_blob(items=None):
    """(blob, payload): all corpus frames in one seekable blob, and the bytes
    it must decode to."""
    items = corpus() if items is None else items
    return (wrap_seekable([it.frame for it in items], [len(it.payload) for it in items]),
            b"".join(it.payload for it in items))
