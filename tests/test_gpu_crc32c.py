"""CRC-32C on the GPU: ``GpuEngine.crc32c_ranges`` (core/hip/crc32c.hip)
against the bytewise reference of test_crc32c, at the head, row, segment and
combine boundaries of the kernel's split, and ``part_checksum="crc32c"`` end
to end against modelx-s3d + modelxd."""
import functools
import os

import pytest

torch = pytest.importorskip("torch")

from modelx_amd import _core
from modelx_amd.client import gpu_rules as rules
from modelx_amd.client.gpu import _signed_headers
from modelx_amd.wire import digest as dg
from modelx_amd.wire import errors as er
from modelx_amd.wire import paths as pm
from modelx_amd.wire import types

from test_crc32c import ref_crc32c, seeded

pytestmark = pytest.mark.gpu

S = _core.CRC32C_SEGMENT_BYTES
LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, S - 1, S, S + 1, 3 * S + 1041]
HOST = seeded(3 * S + 1041 + 16)


@pytest.fixture(scope="module")
def engine():
    return _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=2)


@pytest.fixture(scope="module")
def dev():
    """HOST in HBM; torch's allocations are at least 16 B aligned, so a range's
    offset into it is its misalignment."""
    t = torch.frombuffer(bytearray(HOST), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


@functools.lru_cache(maxsize=None)
def ref(off: int, length: int) -> int:
    return ref_crc32c(HOST[off:off + length])


@pytest.mark.parametrize("offset", [0, 1, 5, 15])
@pytest.mark.parametrize("length", LENGTHS)
def test_range_matches_reference(engine, dev, length, offset):
    assert engine.crc32c_ranges([(dev.data_ptr() + offset, length)]) == [ref(offset, length)]


def test_many_ranges_in_one_launch(engine, dev):
    """Unequal lengths, an empty range, two that overlap: each its own value,
    in order."""
    spans = [(3, S + 100), (0, 0), (40, 5000), (1000, 5000), (7, 9), (S, 2 * S + 77), (9, 0)]
    got = engine.crc32c_ranges([(dev.data_ptr() + o, n) for o, n in spans])
    assert got == [ref(o, n) for o, n in spans]


def test_more_ranges_than_the_grid(engine, dev):
    """One-row ranges, more than the capped grid has waves (8192) or
    workgroups; 61 distinct windows, so a range mapped to a neighbour's
    descriptor shows."""
    spans = [(16 * (i % 61), 1024) for i in range(8192 + 300)]
    got = engine.crc32c_ranges([(dev.data_ptr() + o, n) for o, n in spans])
    assert got == [ref(o, n) for o, n in spans]


def test_all_zero_range(engine):
    """Zeros contribute nothing to the raw registers, so the value is the
    initial-value term alone: lost, it hides behind nothing here."""
    z = torch.zeros(2 * S, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert engine.crc32c_ranges([(z.data_ptr(), 2 * S)]) == [ref_crc32c(bytes(2 * S))]


# ------------------------------------------------------------ end to end --

@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    from util_servers import start_modelxd_s3, start_s3d

    s3d = start_s3d(str(tmp_path_factory.mktemp("s3-crc")))
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    yield mdx, s3d
    mdx.stop()
    s3d.stop()


@pytest.fixture(scope="module")
def client(stack):
    from modelx_amd.client.gpu import GpuClient

    return GpuClient(stack[0].url, device=0, num_slots=4, slot_bytes=1 << 20)


def test_push_with_part_checksums_round_trips(client, dev):
    src = dev[5:5 + 3 * 65536 + 777]  # four parts, the last one ragged, sources unaligned
    client.last_stats.clear()
    client.push_from_gpu("crc/model", "v1", {"w.bin": src}, part_bytes=65536,
                         part_checksum="crc32c")
    phase, = [s for s in client.last_stats if s["phase"] == "push-part-checksum"]
    assert phase["bytes"] == src.numel() and phase["parts"] == 4
    back = client.pull_to_gpu("crc/model", "v1")
    assert torch.equal(back["w.bin"], src)


@pytest.mark.parametrize("flip", [0, 1], ids=["right", "bit-flipped"])
def test_store_checks_a_device_part(client, stack, dev, flip):
    n = 70001
    src = dev[1:1 + n]
    desc = types.Descriptor(name="p.bin", media_type=types.MEDIA_TYPE_MODEL_FILE,
                            digest=dg.sha256_digest(HOST[1:1 + n]), size=n)
    repo = f"crc/part{flip}"
    part = client.remote.get_blob_location(repo, desc, "upload").properties["parts"][0]
    crc, = client.engine.crc32c_ranges([(src.data_ptr(), n)])
    s3d = stack[1]
    root = s3d.proc.args[s3d.proc.args.index("--root") + 1]
    path = os.path.join(root, "modelx", "registry", pm.blob_digest_path(repo, desc.digest))

    def push():
        headers = {**_signed_headers(part), **rules.part_checksum_headers(crc ^ flip)}
        client.engine.push_part_from_device(part["url"], part.get("method") or "PUT", headers,
                                            src.data_ptr(), n)
    if flip:
        with pytest.raises(RuntimeError, match="HTTP 400"):
            push()
        assert not os.path.exists(path)
    else:
        push()
        with open(path, "rb") as f:
            assert f.read() == HOST[1:1 + n]


def test_unknown_part_checksum_is_unsupported(client, dev):
    with pytest.raises(er.ModelxError) as e:
        client.push_from_gpu("crc/md5", "v1", {"w.bin": dev[:64]}, part_checksum="md5")
    assert e.value.code == er.ErrCode.UNSUPPORTED
