"""The pull side of directory blobs on the GPU: ``engine.tar_index``
(``tar_index_kernel`` plus the engine's copies) against the host model
``_core.tar_index_host`` and Python's ``tarfile`` on the foreign and damaged
archives of util_tarcorpus.py, and ``engine.tar_scatter`` against a numpy model
of the same copies at every pair of 16 B phases, across the 4 MiB piece edge
and at zero length, with guard bytes around every destination."""
import numpy as np
import pytest
import util_tarcorpus as tc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SLACK = 2 * MIB
FILL = 0xA5


@pytest.fixture(scope="module")
def engine():
    from modelx_amd import _core

    return _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=2)


@pytest.fixture(scope="module")
def arena():
    """One device buffer for every archive: the archive goes to the front,
    everything behind it is live 0xA5. A read past tar_len stays inside the
    allocation and meets bytes that are no tar header, so a missing bound
    shows as a wrong result."""
    return torch.empty((256 << 10) + SLACK, dtype=torch.uint8, device="cuda:0")


def _place(arena, blob: bytes) -> int:
    assert len(blob) + SLACK <= arena.numel()
    arena.fill_(FILL)
    if blob:
        arena[:len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
    torch.cuda.synchronize()
    return arena.data_ptr()


# ------------------------------------------------------------------ index --

def test_index_matches_host_model_and_tarfile(engine, arena):
    from modelx_amd import _core

    good = tc.good_archives()
    assert len(good) >= 20
    for name, blob in good.items():
        got = engine.tar_index(_place(arena, blob), len(blob))
        assert got == _core.tar_index_host(blob), name
        assert got == tc.listing(blob), name
    for name, (blob, expect) in tc.ragged_archives().items():
        got = engine.tar_index(_place(arena, blob), len(blob))
        assert got == expect == _core.tar_index_host(blob), name


def test_malformed_archives_rejected(engine, arena):
    """Every damaged archive raises, with the host model's message (cause
    and header offset), and the engine indexes a good archive afterwards.
    No case claims more than 1 MiB beyond tar_len; 2 MiB of slack are live
    behind each."""
    from modelx_amd import _core

    bad = tc.bad_archives()
    assert len(bad) >= 25
    for name, blob in bad.items():
        with pytest.raises(RuntimeError) as host:
            _core.tar_index_host(blob)
        ptr = _place(arena, blob)
        with pytest.raises(RuntimeError) as dev:
            engine.tar_index(ptr, len(blob))
        assert str(dev.value) == str(host.value), name
    blob = tc.good_archives()["tarfile-pax"]
    assert engine.tar_index(_place(arena, blob), len(blob)) == tc.listing(blob)


def test_foreign_gnu_archive_end_to_end(engine):
    """A GNU-format archive written by tarfile: index, scatter into fresh
    tensors, every file's bytes as tarfile extracts them."""
    blob = tc.good_archives()["tarfile-gnu"]
    archive = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    entries = engine.tar_index(archive.data_ptr(), len(blob))
    expect = tc.payloads(blob)
    assert [e["name"] for e in entries] == [n for n, _ in expect] and len(entries) == 11
    out = [torch.full((e["size"] + 32,), FILL, dtype=torch.uint8, device="cuda:0")
           for e in entries]
    torch.cuda.synchronize()
    engine.tar_scatter(archive.data_ptr(),
                       [(e["offset"], t.data_ptr() + 16, e["size"]) for e, t in zip(entries, out)])
    for e, t, (name, data) in zip(entries, out, expect):
        got = t.cpu().numpy().tobytes()
        assert got[16:16 + e["size"]] == data, name
        assert got[:16] == got[16 + e["size"]:] == bytes([FILL]) * 16, name


# ---------------------------------------------------------------- scatter --

def _scatter_and_compare(engine, src, segs, dst_len):
    """One tar_scatter call of segs = [(src_off, dst_off, len)] into a
    0xA5-filled buffer; the whole buffer against numpy doing the same copies."""
    assert src.data_ptr() % 16 == 0
    dst = torch.full((dst_len,), FILL, dtype=torch.uint8, device="cuda:0")
    assert dst.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    engine.tar_scatter(src.data_ptr(), [(s, dst.data_ptr() + d, n) for s, d, n in segs])
    host = src.cpu().numpy()
    model = np.full(dst_len, FILL, dtype=np.uint8)
    for s, d, n in segs:
        assert s + n <= host.size and d + n <= dst_len
        model[d:d + n] = host[s:s + n]
    got = dst.cpu().numpy()
    if not np.array_equal(got, model):
        first = int(np.flatnonzero(got != model)[0])
        seg = next((x for x in segs if x[1] - 32 <= first < x[1] + x[2] + 32), None)
        raise AssertionError(f"destination differs from the model first at byte {first}; "
                             f"nearest segment (src_off, dst_off, len) = {seg}")


def _lay_out(cases):
    """cases = [(src_phase, dst_phase, len)] -> segments with disjoint
    destinations, at least 16 guard bytes apart, and the buffer length."""
    segs, cursor = [], 16
    for i, (sp, dp, n) in enumerate(cases):
        d = ((cursor + 15) & ~15) + dp
        segs.append((16 * (i % 61) + sp, d, n))
        cursor = d + n + 16
    return segs, ((cursor + 15) & ~15) + 16


def test_scatter_all_phase_pairs(engine):
    """Every (source phase, destination phase) in 0..15 x 0..15 at lengths
    around the 16 B vector and one past 4096: the same-phase path (head,
    vector body, tail), the bytewise path, and len < head."""
    lengths = [1, 15, 16, 17, 33, 4097]
    cases = [(sp, dp, n) for n in lengths for sp in range(16) for dp in range(16)]
    segs, dst_len = _lay_out(cases)
    g = torch.Generator(device="cuda:0").manual_seed(11)
    src = torch.randint(0, 256, (8192,), dtype=torch.uint8, device="cuda:0", generator=g)
    assert len(segs) == 6 * 256
    for (s, d, n), (sp, dp, _) in zip(segs, cases):
        assert s % 16 == sp and d % 16 == dp
    _scatter_and_compare(engine, src, segs, dst_len)


def test_scatter_across_piece_edge(engine):
    """Segments the engine splits into 4 MiB pieces, at equal and unequal
    phases: every piece after the first starts 4 MiB further on both sides."""
    lengths = [4 * MIB - 1, 4 * MIB + 1, 9 * MIB + 777]
    cases = [(sp, dp, n) for n in lengths for sp, dp in ((0, 0), (1, 1), (0, 1), (15, 8))]
    segs, dst_len = _lay_out(cases)
    g = torch.Generator(device="cuda:0").manual_seed(12)
    src = torch.randint(0, 256, (10 * MIB,), dtype=torch.uint8, device="cuda:0", generator=g)
    _scatter_and_compare(engine, src, segs, dst_len)


def test_scatter_zero_length_segments(engine):
    g = torch.Generator(device="cuda:0").manual_seed(13)
    src = torch.randint(0, 256, (4096,), dtype=torch.uint8, device="cuda:0", generator=g)
    # alone: returns, writes nothing
    _scatter_and_compare(engine, src, [(5, 48, 0)], 128)
    _scatter_and_compare(engine, src, [(0, 0, 0), (4096, 128, 0)], 128)
    # between two real ones
    _scatter_and_compare(engine, src, [(3, 32, 100), (700, 160, 0), (1001, 200, 333)], 1024)
    torch.cuda.synchronize()
