"""Content-defined chunk dedup on the GPU: the candidate kernel
(core/hip/cdc.hip) and the off-grid dedup kernels (core/hip/dedup.hip) against
the host model (_core.cdc_*_host) and hashlib, then the client end to end."""
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_cdc import PARAMS, shifted_pair

from modelx_amd import _core

pytestmark = pytest.mark.gpu

TILE = _core.CDC_TILE_BYTES
SIZES = (0, 1, 31, 32, 33, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def engine():
    assert _core.hip_available(), "native extension loaded but no HIP device"
    return _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=4)


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(9).integers(0, 256, max(SIZES) + 64, dtype=np.uint8)


def _device(data, offset=0, fill=0, tail=64):
    """`data` placed `offset` bytes into a `fill`-filled allocation."""
    buf = torch.full((offset + len(data) + tail,), fill, dtype=torch.uint8, device="cuda")
    if len(data):
        buf[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    torch.cuda.synchronize()  # the engine does not order against torch's stream
    return buf


@pytest.mark.parametrize("bits", [2, 6, 16])  # 2 overflows every tile's list: the host path
@pytest.mark.parametrize("offset", [0, 1, 15])
def test_candidates_equal_the_host_model(engine, noise, offset, bits):
    whole = noise.tobytes()
    for size in SIZES:
        want = _core.cdc_candidates_host(whole[:size], bits)
        assert want or size < max(SIZES)  # the largest size has candidates at every bits
        for fill in (0x00, 0xFF):  # what lies on either side of the range must not matter
            buf = _device(whole[:size], offset + 48, fill)
            assert engine.cdc_candidates(buf.data_ptr() + offset + 48, size, bits) == want, (
                size, fill)


@pytest.mark.parametrize("params", [PARAMS, _core.CDC_DEFAULTS])
@pytest.mark.parametrize("zeros", [False, True])
def test_chunks_and_their_digests(engine, params, zeros):
    data = bytes(1 << 20) if zeros else np.random.default_rng(8).integers(
        0, 256, 1 << 20, dtype=np.uint8).tobytes()
    buf = _device(data, 3)
    ptr = buf.data_ptr() + 3
    chunks = engine.cdc_chunks(ptr, len(data), *params)
    assert chunks == _core.cdc_chunks_host(data, *params)
    if zeros:  # no candidates in constant data: cut by max alone
        assert {l for _, l in chunks} == {params[2]}
    digests = engine.sha256_multibuf([(ptr + o, l) for o, l in chunks])
    assert digests == b"".join(hashlib.sha256(data[o:o + l]).digest() for o, l in chunks)
    with pytest.raises(ValueError, match="UNSUPPORTED"):
        engine.cdc_chunks(ptr, len(data), 63, 6, 1024)


def _digests(data, ranges):
    return b"".join(hashlib.sha256(data[o:o + l]).digest() for o, l in ranges)


@pytest.mark.parametrize("params", [PARAMS, (2048, 11, 32768)])  # short bodies; unrolled bodies
def test_register_and_pull_ranges(params):
    engine = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=4)
    engine.dedup_reset(1 << 14)
    a, b = shifted_pair()
    ra, rb = _core.cdc_chunks_host(a, *params), _core.cdc_chunks_host(b, *params)
    src = _device(a)
    engine.dedup_register_ranges(_digests(a, ra), src.data_ptr(), ra)
    have = {}
    for o, l in ra:
        have.setdefault(hashlib.sha256(a[o:o + l]).digest(), (o, l))
    base = 11  # odd; 11 + 37 is a multiple of 16, so chunks behind the insertion agree in phase
    dst = _device(bytes(len(b)), base, SENTINEL)
    dst[:] = SENTINEL
    torch.cuda.synchronize()
    missing, dedup_bytes = engine.dedup_pull_ranges(_digests(b, rb), rb, dst.data_ptr() + base)

    expect = bytearray([SENTINEL]) * dst.numel()
    phases, want_missing = set(), []
    for o, l in rb:
        hit = have.get(hashlib.sha256(b[o:o + l]).digest())
        if hit:
            expect[base + o:base + o + l] = b[o:o + l]
            phases.add((hit[0] - (base + o)) % 16 == 0)
        elif want_missing and sum(want_missing[-1]) == o:
            want_missing[-1] = (want_missing[-1][0], want_missing[-1][1] + l)
        else:
            want_missing.append((o, l))
    assert phases == {True, False}
    assert dst.cpu().numpy().tobytes() == bytes(expect)
    assert [tuple(m) for m in missing] == want_missing
    assert dedup_bytes + sum(l for _, l in missing) == len(b) and dedup_bytes >= len(b) // 2


# ------------------------------------------------------------- end to end --

@pytest.fixture(scope="module")
def pushed(tmp_path_factory):
    """A and B pushed with CDC sidecars; yields (registry url, A, B)."""
    from util_servers import start_modelxd_s3, start_s3d

    from modelx_amd.client.gpu import GpuClient
    from modelx_amd.wire import errors as er
    from modelx_amd.wire import types

    s3d = start_s3d(str(tmp_path_factory.mktemp("s3-cdc")))
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    try:
        a, b = shifted_pair()
        g = GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20)
        for version, data in (("a", a), ("b", b)):
            m = g.push_from_gpu("cdc/model", version, {"w.bin": _device(data, tail=0)}, cdc=PARAMS)
            side = [d for d in m.blobs if d.media_type == types.MEDIA_TYPE_MODEL_CDC]
            assert len(side) == 1 and m.blobs[0].annotations[
                types.ANNOTATION_CDC_BLOB] == side[0].digest
        assert [s["chunks"] for s in g.last_stats if s["phase"] == "push-cdc"] == [
            len(_core.cdc_chunks_host(d, *PARAMS)) for d in (a, b)]
        with pytest.raises(er.ModelxError):
            g.push_from_gpu("cdc/model", "z", {"w.bin": _device(a, tail=0)}, cdc=True,
                            compress="zstd")
        yield mdx.url, a, b
    finally:
        mdx.stop()
        s3d.stop()


def _pull_a_then_b(url, poison=False, **options):
    from modelx_amd.client.gpu import GpuClient

    g = GpuClient(url, device=0, num_slots=4, slot_bytes=8 << 20, dedup=True, **options)
    got_a = g.pull_to_gpu("cdc/model", "a")
    assert list(got_a) == ["w.bin"]  # no sidecar is landed as a tensor
    if poison:  # a registered source chunk changes under the table
        got_a["w.bin"][100_000:100_064] ^= 0xFF
        torch.cuda.synchronize()
    g.last_stats.clear()
    got_b = g.pull_to_gpu("cdc/model", "b")["w.bin"].cpu().numpy().tobytes()
    return got_a["w.bin"], got_b, {s["phase"]: s for s in g.last_stats}


def test_shifted_blob_is_gathered_from_hbm(pushed):
    url, a, b = pushed
    got_a, got_b, stats = _pull_a_then_b(url, cdc=PARAMS)
    assert got_a.cpu().numpy().tobytes() == a and got_b == b
    cdc = stats["pull-cdc"]
    assert cdc["dedup_bytes"] >= len(b) // 2
    assert cdc["dedup_bytes"] + cdc["bytes"] == len(b)
    assert cdc["chunks"] == len(_core.cdc_chunks_host(b, *PARAMS))


def test_grid_dedup_alone_misses_the_shifted_blob(pushed):
    url, _, b = pushed
    _, got_b, stats = _pull_a_then_b(url)
    assert got_b == b and "pull-cdc" not in stats
    assert stats.get("pull-dedup", {}).get("dedup_bytes", 0) < len(b) // 2


def test_poisoned_source_degrades_to_a_fetch(pushed):
    url, _, b = pushed
    _, got_b, stats = _pull_a_then_b(url, poison=True, cdc=PARAMS)
    assert got_b == b
    assert stats["pull-cdc"]["dedup_bytes"] >= len(b) // 2 and "pull-chunk-refetch" in stats
