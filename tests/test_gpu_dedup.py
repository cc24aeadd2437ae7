"""Chunk-dedup kernels (core/hip/dedup.hip) against a host model.

The model is a dict digest -> chunk bytes: the first registration of a digest
wins, a probe hits only when the chunk length matches too, and a digest whose
first 8 bytes are zero is never stored. Every pull lands in a sentinel-filled
buffer that is larger than the blob, and the WHOLE buffer is compared with
what the model predicts: hit chunks hold the source bytes; missed chunks, the
slack behind the blob and the guards on both sides still hold the sentinel.

Leaves come from hashlib (modelx_amd.wire.digest.chunk_leaves) or are made by
hand; no GPU path serves as a reference. Each test owns its engine, so the
table state is that test's alone."""
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from modelx_amd.wire import digest as dg

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64  # bytes kept before and after every destination window
CAP = 1024  # table capacity of the tests that do not care


def _engine(cap=CAP):
    from modelx_amd import _core

    assert _core.hip_available(), "native extension loaded but no HIP device"
    e = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=4)
    if cap:
        e.dedup_reset(cap)
    return e


def _rand(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _device(data: bytes, offset=0):
    """(keep-alive tensor, device address) of `data` placed `offset` bytes
    into a larger allocation (torch allocations are 256-byte aligned)."""
    buf = torch.zeros(offset + len(data) + 16, dtype=torch.uint8, device="cuda")
    if data:
        buf[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    torch.cuda.synchronize()  # the engine does not order against torch's stream
    return buf, buf.data_ptr() + offset


def _chunks(data: bytes, cs: int):
    return [data[o:o + cs] for o in range(0, len(data), cs)] if data else [b""]


class Model:
    def __init__(self):
        self.tab = {}

    def register(self, leaves, data, cs):
        for leaf, chunk in zip(leaves, _chunks(data, cs)):
            if leaf[:8] != bytes(8):
                self.tab.setdefault(leaf, chunk)

    def hits(self, leaves, cs, total):
        """{chunk index: source bytes} of the chunks a pull must gather."""
        out = {}
        for i, leaf in enumerate(leaves):
            want = min(cs, total - i * cs)
            got = self.tab.get(leaf)
            if want > 0 and leaf[:8] != bytes(8) and got is not None and len(got) == want:
                out[i] = got
        return out


def _merged_missing(hit_idx, cs, total):
    out = []
    for i in range((total + cs - 1) // cs):
        if i in hit_idx:
            continue
        off, ln = i * cs, min(cs, total - i * cs)
        if out and out[-1][0] + out[-1][1] == off:
            out[-1] = (out[-1][0], out[-1][1] + ln)
        else:
            out.append((off, ln))
    return out


def _sentinel_buffer(nbytes):
    buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf


def _assert_buffer(buf, window, hits, cs):
    """Hit chunks equal their source bytes; every other byte of the
    allocation is still the sentinel."""
    expect = bytearray([SENTINEL]) * buf.numel()
    for i, chunk in hits.items():
        expect[window + i * cs: window + i * cs + len(chunk)] = chunk
    torch.cuda.synchronize()
    got = buf.cpu().numpy().tobytes()
    if got != bytes(expect):
        bad = next(k for k in range(len(got)) if got[k] != expect[k])
        rel = bad - window
        raise AssertionError(
            f"destination differs first at window offset {rel} (chunk {rel // cs}, "
            f"byte {rel % cs}): got {got[bad]:#x}, expected {expect[bad]:#x}")


def _pull_check(engine, leaves, cs, total, hits, dst_off=0):
    """dedup_pull into a sentinel buffer with guards and a chunk of slack;
    `hits` is what the model says must be gathered."""
    window = GUARD + dst_off
    buf = _sentinel_buffer(window + total + cs + GUARD)
    missing, deduped = engine.dedup_pull(b"".join(leaves), buf.data_ptr() + window, cs, total)
    missing = [tuple(m) for m in missing]
    assert missing == _merged_missing(set(hits), cs, total)
    assert deduped + sum(ln for _, ln in missing) == total
    _assert_buffer(buf, window, hits, cs)
    return missing, deduped


# ------------------------------------------------------------------ phases --

# ~40 chunks with a 1..15-byte tail. 1000 = 8 mod 16, so consecutive chunks
# alternate 16-byte phase inside one call; 17 walks through all 16 phases and
# its 3-byte tail makes `head > len` reachable in the gather kernel.
PHASE_CASES = [(4096, 39 * 4096 + 7), (1000, 39 * 1000 + 11), (17, 39 * 17 + 3)]


@pytest.mark.parametrize("cs,total", PHASE_CASES)
def test_phases(cs, total):
    """Source base phases 0..15 x destination phase 0 / same as source / 5:
    the gather kernel's byte path (phases differ), its head/body/tail split
    (phases agree), head > len and sub-16-byte chunks."""
    engine = _engine()
    rng = np.random.default_rng(cs)
    n = (total + cs - 1) // cs
    src = _rand(rng, total)
    # the pulled blob shares a seeded random half of its full chunks, and the
    # tail chunk, with the registered one; the rest is fresh content
    shared = set(rng.permutation(n - 1)[: (n - 1) // 2].tolist()) | {n - 1}
    want = b"".join(c if i in shared else _rand(rng, len(c))
                    for i, c in enumerate(_chunks(src, cs)))
    src_leaves = dg.chunk_leaves(src, cs)
    want_leaves = dg.chunk_leaves(want, cs)
    for src_off in range(16):
        engine.dedup_reset(0)
        model = Model()
        keep, ptr = _device(src, src_off)
        assert engine.dedup_register(b"".join(src_leaves), ptr, cs, total) == 0
        model.register(src_leaves, src, cs)
        hits = model.hits(want_leaves, cs, total)
        assert set(hits) == shared
        for dst_off in sorted({0, src_off, 5}):
            _pull_check(engine, want_leaves, cs, total, hits, dst_off)
        del keep


# ------------------------------------------------------------- tail length --

def test_tail_length_is_part_of_the_key():
    """Equal bytes give an equal digest; a chunk is a hit only when the
    resident chunk's length is the length the pulling blob wants there."""
    engine = _engine()
    rng = np.random.default_rng(1)
    cs, tail_len = 4096, 100
    blob = _rand(rng, 2 * cs + tail_len)
    leaves = dg.chunk_leaves(blob, cs)
    model = Model()
    keep, ptr = _device(blob)
    assert engine.dedup_register(b"".join(leaves), ptr, cs, len(blob)) == 0
    model.register(leaves, blob, cs)

    # the registered tail's digest stands where a FULL chunk is wanted: miss
    fresh = hashlib.sha256(_rand(rng, 50)).digest()
    pull = [leaves[0], leaves[2], fresh]
    hits = model.hits(pull, cs, 2 * cs + 50)
    assert set(hits) == {0}
    _pull_check(engine, pull, cs, 2 * cs + 50, hits)

    # reverse: the same digest as a 100-byte tail, at another index: hit
    pull = [leaves[1], leaves[0], leaves[1], leaves[2]]
    total = 3 * cs + tail_len
    hits = model.hits(pull, cs, total)
    assert set(hits) == {0, 1, 2, 3}
    _pull_check(engine, pull, cs, total, hits, dst_off=3)

    # a full chunk's digest where a 100-byte tail is wanted: miss
    pull = [leaves[0]]
    assert model.hits(pull, cs, tail_len) == {}
    _pull_check(engine, pull, cs, tail_len, {})
    del keep


# -------------------------------------------------------- synthetic leaves --

def test_zero_prefix_leaf_is_never_stored():
    engine = _engine()
    rng = np.random.default_rng(2)
    cs = 256
    blob = _rand(rng, 3 * cs)
    leaves = dg.chunk_leaves(blob, cs)
    leaves[1] = bytes(8) + _rand(rng, 24)  # key 0 is the table's "empty"
    model = Model()
    keep, ptr = _device(blob)
    assert engine.dedup_register(b"".join(leaves), ptr, cs, len(blob)) == 0
    model.register(leaves, blob, cs)
    hits = model.hits(leaves, cs, len(blob))
    assert set(hits) == {0, 2}
    missing, _ = _pull_check(engine, leaves, cs, len(blob), hits)
    assert missing == [(cs, cs)]
    # alone, and after a second registration, it is still missing
    assert engine.dedup_register(b"".join(leaves), ptr, cs, len(blob)) == 0
    _pull_check(engine, [leaves[1]], cs, cs, {})
    del keep


def test_shared_key_prefix_keeps_entries_apart():
    """Two digests with equal first 8 bytes (the CAS key) live in two slots
    and each gathers its own bytes."""
    engine = _engine()
    rng = np.random.default_rng(3)
    cs = 512
    prefix = b"\x07" + _rand(rng, 7)
    leaf_a, leaf_b = prefix + _rand(rng, 24), prefix + _rand(rng, 24)
    blob_a, blob_b = _rand(rng, cs), _rand(rng, cs)
    model = Model()
    keep_a, ptr_a = _device(blob_a, 1)
    keep_b, ptr_b = _device(blob_b, 9)
    assert engine.dedup_register(leaf_a, ptr_a, cs, cs) == 0
    model.register([leaf_a], blob_a, cs)
    assert engine.dedup_register(leaf_b, ptr_b, cs, cs) == 0
    model.register([leaf_b], blob_b, cs)
    for pull in ([leaf_a, leaf_b], [leaf_b, leaf_a, leaf_b]):
        total = len(pull) * cs
        hits = model.hits(pull, cs, total)
        assert len(hits) == len(pull)
        _pull_check(engine, pull, cs, total, hits)
    # same prefix, third digest: not resident
    _pull_check(engine, [prefix + _rand(rng, 24)], cs, cs, {})
    del keep_a, keep_b


# ------------------------------------------------- probe window, wrap-around --

def test_probe_window_wraps_and_counts_drops():
    """100 distinct leaves whose home slot is 253 of 256: the 64-slot probe
    window wraps past the end of the table, keeps 64 and drops 36."""
    engine = _engine(256)
    rng = np.random.default_rng(4)
    cs, n = 64, 100
    blob = _rand(rng, n * cs)
    leaves = [b"\xfd" + _rand(rng, 31) for _ in range(n)]
    assert len(set(leaves)) == n
    chunks = _chunks(blob, cs)
    keep, ptr = _device(blob, 4)
    assert engine.dedup_register(b"".join(leaves), ptr, cs, n * cs) == 36

    # which 64 won the slots is the hardware's choice; everything else is not
    window = GUARD
    buf = _sentinel_buffer(window + n * cs + cs + GUARD)
    missing, deduped = engine.dedup_pull(b"".join(leaves), buf.data_ptr() + window, cs, n * cs)
    missing = [tuple(m) for m in missing]
    missed = {off // cs + k for off, ln in missing for k in range(ln // cs)}
    hit_idx = set(range(n)) - missed
    assert len(hit_idx) == 64 and deduped == 64 * cs
    assert missing == _merged_missing(hit_idx, cs, n * cs)
    assert deduped + sum(ln for _, ln in missing) == n * cs
    _assert_buffer(buf, window, {i: chunks[i] for i in hit_idx}, cs)

    # the count is a running sum: ten more for the same full window
    more = [b"\xfd" + _rand(rng, 31) for _ in range(10)]
    keep2, ptr2 = _device(blob[: 10 * cs])
    assert engine.dedup_register(b"".join(more), ptr2, cs, 10 * cs) == 46
    del keep, keep2


# -------------------------------------------------- repeats in one launch --

def test_repeated_leaves_in_one_call_take_one_slot():
    """64 copies of one leaf in ONE register call must occupy one slot of a
    64-slot table, not 64: the 8 chunks registered next all find room.

    Inside one insert launch a lane that loses the CAS to an equal key reads
    the winner's digest before the winner has stored it; without the host
    dropping repeats first, each copy claims a slot of its own and the
    second call returns 8 (observed on an MI355X before that fix)."""
    engine = _engine(64)
    rng = np.random.default_rng(5)
    cs = 64
    one = _rand(rng, cs)
    blob = one * 64
    leaves = dg.chunk_leaves(blob, cs)
    assert len(set(leaves)) == 1
    model = Model()
    keep, ptr = _device(blob)
    assert engine.dedup_register(b"".join(leaves), ptr, cs, len(blob)) == 0
    model.register(leaves, blob, cs)

    blob2 = _rand(rng, 8 * cs)
    leaves2 = dg.chunk_leaves(blob2, cs)
    keep2, ptr2 = _device(blob2, 7)
    assert engine.dedup_register(b"".join(leaves2), ptr2, cs, len(blob2)) == 0
    model.register(leaves2, blob2, cs)

    hits = model.hits(leaves2, cs, len(blob2))
    assert len(hits) == 8
    missing, deduped = _pull_check(engine, leaves2, cs, len(blob2), hits)
    assert missing == [] and deduped == len(blob2)
    hits = model.hits(leaves, cs, len(blob))
    assert len(hits) == 64
    _pull_check(engine, leaves, cs, len(blob), hits, dst_off=5)
    del keep, keep2


# --------------------------------------------------------------- lifecycle --

def test_lifecycle():
    engine = _engine(cap=0)
    rng = np.random.default_rng(6)
    cs = 128
    blob = _rand(rng, 5 * cs + 9)
    leaves = dg.chunk_leaves(blob, cs)
    empty = [hashlib.sha256(b"").digest()]

    # before any register: everything missing, nothing written
    missing, deduped = _pull_check(engine, leaves, cs, len(blob), {})
    assert missing == [(0, len(blob))] and deduped == 0
    buf = _sentinel_buffer(2 * GUARD)
    assert tuple(engine.dedup_pull(empty[0], buf.data_ptr() + GUARD, cs, 0)) == ([], 0)
    _assert_buffer(buf, GUARD, {}, cs)

    engine.dedup_reset(64)
    model = Model()
    keep, ptr = _device(blob, 3)
    assert engine.dedup_register(b"".join(leaves), ptr, cs, len(blob)) == 0
    model.register(leaves, blob, cs)
    hits = model.hits(leaves, cs, len(blob))
    assert len(hits) == 6
    _pull_check(engine, leaves, cs, len(blob), hits)

    # an empty blob registers and pulls as ([], 0)
    keep0, ptr0 = _device(b"")
    assert engine.dedup_register(empty[0], ptr0, cs, 0) == 0
    assert tuple(engine.dedup_pull(empty[0], buf.data_ptr() + GUARD, cs, 0)) == ([], 0)
    _assert_buffer(buf, GUARD, {}, cs)

    # reset(0) forgets everything ...
    engine.dedup_reset(0)
    missing, deduped = _pull_check(engine, leaves, cs, len(blob), {})
    assert missing == [(0, len(blob))] and deduped == 0
    # ... and keeps the capacity of 64: one leaf per home slot fills the
    # table, so a 65th has nowhere to go (any larger table would take it)
    fill = [bytes([s, 1]) + _rand(rng, 30) for s in range(64)]
    keep2, ptr2 = _device(_rand(rng, 64 * cs))
    assert engine.dedup_register(b"".join(fill), ptr2, cs, 64 * cs) == 0
    assert engine.dedup_register(bytes([64, 1]) + _rand(rng, 30), ptr2, cs, cs) == 1
    del keep, keep0, keep2


# -------------------------------------------------------------- rejections --

def test_rejections_leave_no_trace():
    """Leaves that do not fit (total, chunk_size), a zero chunk size and a
    bad capacity raise on the host, before any copy or launch; the engine
    stays usable. The surplus leaf is resident, so without the host check it
    would be gathered to dst + 2 * chunk_size, behind the blob's end (the
    destination allocation spans all three chunks, so even that write would
    stay inside it)."""
    engine = _engine()
    rng = np.random.default_rng(7)
    cs = 1024
    blob = _rand(rng, 3 * cs)
    leaves = dg.chunk_leaves(blob, cs)
    packed = b"".join(leaves)
    keep, ptr = _device(blob)
    assert engine.dedup_register(packed, ptr, cs, 3 * cs) == 0
    model = Model()
    model.register(leaves, blob, cs)

    window = GUARD
    buf = _sentinel_buffer(window + 3 * cs + GUARD)
    dst = buf.data_ptr() + window
    bad_calls = {
        "pull, one leaf too many": lambda: engine.dedup_pull(packed, dst, cs, 2 * cs),
        "pull, one leaf too few": lambda: engine.dedup_pull(packed[:32], dst, cs, 2 * cs),
        "pull, 33 bytes of leaves": lambda: engine.dedup_pull(packed[:33], dst, cs, cs),
        "pull, chunk size 0": lambda: engine.dedup_pull(packed, dst, 0, 3 * cs),
        "register, one leaf too many":
            lambda: engine.dedup_register(packed, ptr, cs, 2 * cs),
        "register, one leaf too few":
            lambda: engine.dedup_register(packed[:32], ptr, cs, 2 * cs),
        "register, 33 bytes of leaves":
            lambda: engine.dedup_register(packed[:33], ptr, cs, cs),
        "register, chunk size 0": lambda: engine.dedup_register(packed, ptr, 0, 3 * cs),
        "leaves, chunk size 0": lambda: engine.sha256_chunk_leaves(ptr, 3 * cs, 0),
        "leaves_many, chunk size 0":
            lambda: engine.sha256_chunk_leaves_many([(ptr, cs, cs), (ptr, 3 * cs, 0)]),
        "capacity 96": lambda: engine.dedup_reset(96),
        "capacity 32": lambda: engine.dedup_reset(32),
    }
    for name, call in bad_calls.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name}: accepted")
        _assert_buffer(buf, window, {}, cs)
        # same engine, same table: a good register and pull still work
        assert engine.dedup_register(packed, ptr, cs, 3 * cs) == 0, name
        _pull_check(engine, leaves, cs, 3 * cs, model.hits(leaves, cs, 3 * cs), dst_off=1)
    assert engine.sha256_chunk_leaves(ptr, 3 * cs, cs) == packed
    del keep
