"""The device zstd codec (core/hip/zstd.hip) against libzstd.

Decoder: frames written by the system libzstd (util_zframes.py: levels
1/3/9/19 plus header variants), wrapped into seekable blobs, so that the
256-thread kernel runs the parts of RFC 8878 our own encoder never emits:
FSE-described, RLE and repeat sequence tables, treeless literals on the LDS
table of the previous block, 1-stream literals, raw and RLE blocks, matches
that reach back across blocks, window-descriptor headers, checksums.
test_zframes.py proves on the CPU that the corpus contains each of them.

Encoder: frame sizes from 512 B to 512 KiB at their edge lengths and at odd
source and destination phases, the 4096-frame compress batch and the
8192-frame decode chunk, and an exact destination capacity.

Everything is byte-exact. The expected value is always the original payload,
or hashlib / libzstd acting on it, never the output of the code under test.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")  # before the extension (engineering-notes #16)

import util_seek  # noqa: E402
import util_zframes as uz  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LEAD = 64    # guard bytes before a destination view
GUARD = 64   # ... and after it
FILL = 0xA5


@pytest.fixture(scope="module")
def engine():
    from modelx_amd import _core

    assert _core.hip_available(), "native extension loaded but no HIP device"
    return _core.GpuEngine(device=0, num_slots=8, slot_bytes=32 << 20, num_streams=4)


@pytest.fixture(scope="module")
def corpus():
    """Encoded once per module (level 19 is the slow part)."""
    return uz.corpus()


@pytest.fixture(scope="module")
def one_blob(corpus):
    return uz.corpus_blob(corpus)


def _item(corpus, name, variant):
    (it,) = [it for it in corpus if (it.name, it.variant) == (name, variant)]
    return it


def _to_dev(data: bytes, phase: int = 0):
    """data in HBM, starting `phase` bytes past an 8-byte boundary."""
    buf = torch.empty(phase + len(data) + 8, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0
    view = buf[phase:phase + len(data)]
    if data:
        view.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize()  # the engine runs on its own streams
    return view


class Guarded:
    """n destination bytes at `phase` past an 8-byte boundary, inside an
    allocation filled with 0xA5, with guard bytes on both sides."""

    def __init__(self, n: int, phase: int = 0):
        self.n, self.start = n, LEAD + phase
        self.buf = torch.full((self.start + n + GUARD,), FILL, dtype=torch.uint8,
                              device="cuda")
        assert self.buf.data_ptr() % 8 == 0
        torch.cuda.synchronize()

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + self.start

    def bytes(self, n=None) -> bytes:
        n = self.n if n is None else n
        return self.buf[self.start:self.start + n].cpu().numpy().tobytes()

    def untouched_outside(self, used=None) -> bool:
        """Every byte outside [0, used) of the view still holds the fill."""
        used = self.n if used is None else used
        host = self.buf.cpu()
        return bool((host[:self.start] == FILL).all()
                    and (host[self.start + used:] == FILL).all())


def _decode(engine, blob: bytes, raw_len: int, *, src_phase=0, dst_phase=0):
    src = _to_dev(blob, src_phase)
    dst = Guarded(raw_len, dst_phase)
    n = engine.zstd_decompress_device(src.data_ptr(), len(blob), dst.ptr, raw_len)
    return n, dst


# ------------------------------------------------- decoder: libzstd frames --

def test_all_frames_in_one_blob(engine, corpus, one_blob):
    blob, payload = one_blob
    empties = [i for i, it in enumerate(corpus) if not it.payload]
    assert empties and all(0 < i < len(corpus) - 1 and corpus[i - 1].payload
                           and corpus[i + 1].payload for i in empties)
    n, dst = _decode(engine, blob, len(payload))
    assert n == len(payload)
    got = dst.bytes()
    if got != payload:  # name the first frame that differs
        off = 0
        for it in corpus:
            assert got[off:off + len(it.payload)] == it.payload, (it.name, it.variant)
            off += len(it.payload)
    assert dst.untouched_outside()


def test_one_item_per_payload_and_level(engine, corpus):
    blobs = [uz.wrap_seekable([it.frame], [len(it.payload)]) for it in corpus]
    srcs = [_to_dev(b) for b in blobs]
    dsts = [Guarded(len(it.payload)) for it in corpus]
    assert len(corpus) > 4  # one launch per item, round-robin over the 4 streams
    sizes = engine.zstd_decompress_many(
        [(s.data_ptr(), len(b), d.ptr, d.n) for s, b, d in zip(srcs, blobs, dsts)])
    assert sizes == [len(it.payload) for it in corpus]
    for it, d in zip(corpus, dsts):
        assert d.bytes() == it.payload, (it.name, it.variant)
        assert d.untouched_outside(), (it.name, it.variant)


@pytest.mark.parametrize("name,variant", [("far-offsets", "L19"), ("aab", "L1")])
def test_source_and_destination_phase(engine, corpus, name, variant):
    # mx_par_copy takes its 8-byte path only when source and destination
    # agree modulo 8, and splits head/body/tail by the destination's phase
    it = _item(corpus, name, variant)
    blob = uz.wrap_seekable([it.frame], [len(it.payload)])
    for src_phase in (0, 1, 3):
        src = _to_dev(blob, src_phase)
        for dst_phase in range(9):
            dst = Guarded(len(it.payload), dst_phase)
            n = engine.zstd_decompress_device(src.data_ptr(), len(blob), dst.ptr, dst.n)
            assert n == len(it.payload), (src_phase, dst_phase)
            assert dst.bytes() == it.payload, (src_phase, dst_phase)
            assert dst.untouched_outside(), (src_phase, dst_phase)


def test_checksum_wide_seek_table(engine, one_blob):
    blob, payload = one_blob
    wide = util_seek.with_checksum_flag(blob)
    assert len(wide) > len(blob)
    n, dst = _decode(engine, wide, len(payload))
    assert n == len(payload) and dst.bytes() == payload and dst.untouched_outside()


def test_lying_d_size_is_refused_within_bounds(engine, corpus):
    """Frame 1's d_size understated by one, frame 2's overstated by one: the
    envelope, the c_size sum and the total stay valid, so the host parser
    passes the table on. Every write of decode_frame/decode_block is bounded
    by the d_size the kernel passes as dstcap (fcs > dstcap, out + ll + ml >
    dstcap, out + bsize > dstcap, lit_regen > dstcap), so the kernel must
    report the frames and leave the bytes after the destination alone. Frame 1
    carries no content size in its header, so it is the per-sequence bound
    that stops it, not the header check."""
    items = [_item(corpus, "aab", "L3"),
             _item(corpus, "far-offsets", "L1+checksum+window17"),
             _item(corpus, "shrdlu-900", "L3")]
    assert uz.walk(items[1].frame)["hdr:no-content-size"] == 1
    frames = [it.frame for it in items]
    sizes = [len(it.payload) for it in items]
    payload = b"".join(it.payload for it in items)
    good = uz.wrap_seekable(frames, sizes)
    bad = uz.wrap_seekable(frames, [sizes[0], sizes[1] - 1, sizes[2] + 1])
    src = _to_dev(bad)
    dst = Guarded(len(payload))
    with pytest.raises(RuntimeError):
        engine.zstd_decompress_device(src.data_ptr(), len(bad), dst.ptr, dst.n)
    assert dst.untouched_outside()
    n, dst = _decode(engine, good, len(payload))
    assert n == len(payload) and dst.bytes() == payload and dst.untouched_outside()


# ------------------------------------------------------- batch boundaries --

BATCH_FRAME = 512
BATCH_SIZE = 8193 * BATCH_FRAME + 3  # 8194 frames: 3 compress batches, 2 decode chunks


@pytest.fixture(scope="module")
def batch_payload():
    import random

    rng = random.Random(8194)
    rep = uz.lz_repeats(8194, BATCH_SIZE - 500_000, 100_000, 256)
    a, b = 1_000_003, 2_500_001  # splices off the frame grid
    data = rep[:a] + rng.randbytes(200_000) + rep[a:b] + bytes(300_000) + rep[b:]
    assert len(data) == BATCH_SIZE
    return data


def test_compress_and_decode_across_launch_batches(engine, corpus, batch_payload):
    from modelx_amd import _core

    data = batch_payload
    nframes = 8194
    src = _to_dev(data)
    bound = _core.zstd_compress_bound(len(data), BATCH_FRAME)
    comp = Guarded(bound)
    n = engine.zstd_compress_device(src.data_ptr(), len(data), BATCH_FRAME, comp.ptr, bound)
    assert n <= bound and comp.untouched_outside(n)
    blob = comp.bytes(n)

    table = _core.zstd_seek_table(blob)
    assert len(table) == nframes
    assert [e[3] for e in table] == [BATCH_FRAME] * (nframes - 1) + [3]
    assert [e[2] for e in table] == [i * BATCH_FRAME for i in range(nframes)]
    c_off = 0
    for e in table:  # contiguous compressed spans from 0 up to the table
        assert e[0] == c_off
        c_off += e[1]
    assert c_off + 8 + nframes * 8 + 9 == n

    assert uz.decompress(blob, len(data)) == data

    # the blob stays where the compressor put it: decode from there
    single = Guarded(len(data))
    m = engine.zstd_decompress_device(comp.ptr, n, single.ptr, single.n)
    assert m == len(data) and single.bytes() == data and single.untouched_outside()

    # next to a two-frame blob, so that max_chunk (8192 against 2) and the
    # per-stream literal-scratch offsets differ between the items
    two = [_item(corpus, "far-offsets", "L19"), _item(corpus, "aab", "L1")]
    two_blob = uz.wrap_seekable([it.frame for it in two], [len(it.payload) for it in two])
    two_payload = b"".join(it.payload for it in two)
    two_src = _to_dev(two_blob)
    d_big, d_two = Guarded(len(data)), Guarded(len(two_payload))
    sizes = engine.zstd_decompress_many(
        [(comp.ptr, n, d_big.ptr, d_big.n),
         (two_src.data_ptr(), len(two_blob), d_two.ptr, d_two.n)])
    assert sizes == [len(data), len(two_payload)]
    assert d_big.bytes() == data and d_big.untouched_outside()
    assert d_two.bytes() == two_payload and d_two.untouched_outside()


# ---------------------------------------------------- encoder edge shapes --

@pytest.fixture(scope="module")
def mixed_payload():
    """1.2 MB of text, bf16 bytes and zeros in stretches of 300 B to 300 KB,
    so that a frame of any size may be all of one kind or a mix."""
    import random

    rng = random.Random(512)
    text = b"the quick brown fox jumps over the lazy dog " * 7000
    bf16 = uz.bf16_bytes(11, 400_000)
    out = bytearray()
    kind = 0
    while len(out) < 1_200_000:
        n = int(300 * 1000 ** rng.random())
        if kind == 0:
            start = rng.randrange(len(text) - n)
            out += text[start:start + n]
        elif kind == 1:
            start = rng.randrange(0, len(bf16) - n, 2)
            out += bf16[start:start + n]
        else:
            out += bytes(n)
        kind = (kind + 1) % 3
    return bytes(out)


def _edge_sizes(frame_raw):
    return [0, 1, frame_raw - 1, frame_raw, frame_raw + 1, 2 * frame_raw + 17]


@pytest.mark.parametrize("literals_only", [False, True], ids=["lz", "literals-only"])
@pytest.mark.parametrize("frame_raw", [512, 4096, 65536, 131072, 524288])
def test_encoder_edge_shapes(engine, mixed_payload, frame_raw, literals_only):
    from modelx_amd import _core

    seen = uz.collections.Counter()
    for k, size in enumerate(_edge_sizes(frame_raw)):
        assert size <= 1_100_000
        # another stretch of the payload for every size
        start = (k * 150_001) % (len(mixed_payload) - size)
        data = mixed_payload[start:start + size]
        bound = _core.zstd_compress_bound(size, frame_raw)
        for src_phase, dst_phase in ((0, 0), (3, 0), (0, 5), (3, 5)):
            tag = (size, src_phase, dst_phase)
            src = _to_dev(data, src_phase)
            comp = Guarded(bound, dst_phase)
            n = engine.zstd_compress_device(src.data_ptr(), size, frame_raw, comp.ptr, bound,
                                            literals_only)
            assert n <= bound, tag
            assert comp.untouched_outside(n), tag
            blob = comp.bytes(n)

            nframes = max(1, -(-size // frame_raw))
            table = _core.zstd_seek_table(blob)
            assert [(e[2], e[3]) for e in table] == [
                (i * frame_raw, min(frame_raw, size - i * frame_raw))
                for i in range(nframes)], tag
            c_off = 0
            for e in table:
                assert e[0] == c_off, tag
                c_off += e[1]
                seen += uz.walk(blob[e[0]:e[0] + e[1]])
            assert c_off + 8 + nframes * 8 + 9 == n, tag

            assert uz.decompress(blob, size) == data, tag
            assert _core.zstd_decompress_cpu(blob) == data, tag
            back = Guarded(size, dst_phase)
            m = engine.zstd_decompress_device(comp.ptr, n, back.ptr, size)
            assert m == size and back.bytes() == data, tag
            assert back.untouched_outside(), tag
    print("frame_raw", frame_raw, "literals_only", literals_only, dict(seen))
    if frame_raw == 524288:
        assert seen["frame:>=4-blocks"] > 0  # multi-block frames of our own encoder
    if literals_only:
        assert not [k for k in seen if k[:3] in ("ll:", "of:", "ml:")]


def test_exact_destination_capacity(engine, mixed_payload):
    from modelx_amd import _core

    frame_raw = 4096
    data = mixed_payload[70_000:70_000 + 5 * frame_raw + 17]
    src = _to_dev(data)
    bound = _core.zstd_compress_bound(len(data), frame_raw)
    first = Guarded(bound)
    n = engine.zstd_compress_device(src.data_ptr(), len(data), frame_raw, first.ptr, bound)
    blob = first.bytes(n)
    assert uz.decompress(blob, len(data)) == data

    exact = Guarded(n)
    assert engine.zstd_compress_device(src.data_ptr(), len(data), frame_raw,
                                       exact.ptr, n) == n
    assert exact.bytes() == blob and exact.untouched_outside()

    # one byte short: the seek table no longer fits. A capacity below the
    # frames' total is refused before anything is packed.
    for cap in (n - 1, 10):
        short = Guarded(n)
        with pytest.raises(RuntimeError):
            engine.zstd_compress_device(src.data_ptr(), len(data), frame_raw, short.ptr, cap)
        assert short.untouched_outside(cap), cap

    again = Guarded(bound)
    assert engine.zstd_compress_device(src.data_ptr(), len(data), frame_raw,
                                       again.ptr, bound) == n
    assert again.bytes(n) == blob and again.untouched_outside(n)


# ------------------------------------------------- MODELX_ZSTD_FLAGS = 3 ---

def test_serial_switches_in_a_child(engine, one_blob):
    """Bit 0 (serial Huffman encoder) and bit 1 (serial literal-stream
    decoder) in a fresh process; every other test here runs with both off."""
    assert os.environ.get("MODELX_ZSTD_FLAGS", "0") in ("", "0")
    _, payload = one_blob
    bf16 = uz.payloads()["bf16"]
    engine.synchronize()
    torch.cuda.synchronize()  # nothing of ours in flight while the child runs
    env = dict(os.environ, MODELX_ZSTD_FLAGS="3")
    r = subprocess.run([sys.executable, os.path.join(HERE, "zstd_flags_child.py")],
                       env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    (line,) = [ln for ln in r.stdout.splitlines() if ln.startswith("ZFLAGS ")]
    got = json.loads(line[len("ZFLAGS "):])
    assert got["flags"] == "3"
    assert got["corpus_len"] == len(payload)
    assert got["corpus"] == hashlib.sha256(payload).hexdigest()
    want = hashlib.sha256(bf16).hexdigest()
    assert got["bf16_len"] == len(bf16)
    assert got["bf16_libzstd"] == want and got["bf16_device"] == want
    assert got["bf16_huffman_blocks"] > 0  # the serial Huffman encoder did run
