"""gzip on the GPU: ``GpuEngine.gzip_compress_device`` (core/hip/deflate.hip)
equals the host model of test_deflate byte for byte at every payload, length
and source phase, zlib inflates every one of its outputs, batches after the
first are run at 1 to 7 chunks, the Huffman builder across one workgroup
(core/hip/deflate_lengths.hip) equals the builder on the host, and
``push_from_gpu(dir_format="tar+gz")`` end to end against modelx-s3d + modelxd."""
import gc
import gzip
import hashlib
import io
import os
import tarfile

import pytest

torch = pytest.importorskip("torch")

from modelx_amd import _core
from modelx_amd.wire import paths as pm
from modelx_amd.wire import types as wt

from test_deflate import (C, LENGTHS, OFFSETS, PAYLOADS, check_member, histograms, model,
                          payload, words)
from test_gpu_aead import stored_object, to_dev, to_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    return _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=2)


@pytest.fixture(scope="module")
def devs():
    return {name: to_dev(payload(name)) for name in PAYLOADS}


def compress(engine, ptr, n, **kw):
    """The member and the 16 guard bytes behind it."""
    bound = _core.gzip_compress_bound(n)
    out = torch.full((bound + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    stored = engine.gzip_compress_device(ptr, n, out.data_ptr(), bound, **kw)
    got = to_host(out)
    return got[:stored], got[stored:stored + 16]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_device_equals_host_model(engine, devs, name, n, offset):
    """Byte for byte the host model, and, so that a fault the two share cannot
    hide, zlib inflates the device's bytes to the source at every case."""
    got, guard = compress(engine, devs[name].data_ptr() + offset, n)
    check_member(got, payload(name)[offset:offset + n])
    assert got == model(name, offset, n)
    assert guard == b"\xa5" * 16


@pytest.mark.parametrize("part", range(4))
def test_builder_on_device_equals_builder_on_host(engine, part):
    """build_lengths across the 256 threads of one workgroup (the chunk
    kernel's group context) against the group of one on the host, on the
    histograms of test_deflate: the Kraft sum above one, complement keys and
    keys with the top bits set, the fillers, up to 92 steps through the three
    arg-max cells. One launch of one workgroup each."""
    cases = histograms()[part::4]
    assert len(cases) > 300
    for hid, hist, maxbits, complete in cases:
        ok, lens, _ = _core.deflate_code_lengths_host(hist, maxbits, complete)
        assert engine.deflate_code_lengths_device(hist, maxbits, complete) == (ok, lens), hid


def test_builder_on_device_refuses_what_it_cannot_hold(engine):
    for hist, maxbits in (([1], 15), ([1] * 287, 15), ([1, 1], 0), ([1, 1], 16), ([65536, 1], 15)):
        with pytest.raises(ValueError):
            engine.deflate_code_lengths_device(hist, maxbits, True)


@pytest.fixture(scope="module")
def mixed():
    """Seven chunks, stored (random) and Huffman (words) in turn, the last one
    short, with room for the source phases."""
    parts = [payload("random")[:C], words(7, C), words(8, C), payload("random")[C:2 * C],
             words(9, C), payload("random")[100:100 + C], words(10, 5000)]
    data = b"".join(parts) + bytes(16)
    return data, to_dev(data)


@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("batch_chunks", [1, 2, 3, 7])
def test_later_batches(engine, mixed, batch_chunks, offset):
    """Batches after the first: slots, sizes and addresses are indexed within
    the batch, chunk offsets, BFINAL and the CRC join across it."""
    data, dev = mixed
    n = 6 * C + 5000
    got, guard = compress(engine, dev.data_ptr() + offset, n, batch_chunks=batch_chunks)
    assert got == _core.gzip_compress_host(data[offset:offset + n])
    check_member(got, data[offset:offset + n])
    assert guard == b"\xa5" * 16


@pytest.mark.parametrize("batch_chunks", [0, 4097])
def test_engine_refuses_a_bad_batch(engine, devs, batch_chunks):
    out = torch.empty(4096, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="batch_chunks"):
        engine.gzip_compress_device(devs["words"].data_ptr(), 1000, out.data_ptr(), 4096,
                                    batch_chunks=batch_chunks)


def test_more_chunks_than_the_grid(engine):
    """800 chunks, each stamped with its index: the grid is capped at 768
    workgroups, so the last 32 are reached by its stride."""
    data = bytearray(words(5, 800 * C))
    for i in range(800):
        data[i * C:i * C + 4] = i.to_bytes(4, "little")
    data = bytes(data)
    src = to_dev(data)
    got, _ = compress(engine, src.data_ptr(), len(data))
    assert got == _core.gzip_compress_host(data)


def test_engine_refuses_a_short_destination(engine, devs):
    out = torch.empty(4096, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="bound"):
        engine.gzip_compress_device(devs["words"].data_ptr(), 1000, out.data_ptr(),
                                    _core.gzip_compress_bound(1000) - 1)


# ------------------------------------------------------------ end to end --

@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    from util_servers import start_modelxd_s3, start_s3d

    s3d = start_s3d(str(tmp_path_factory.mktemp("s3-gzip")))
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    yield mdx, s3d
    mdx.stop()
    s3d.stop()


@pytest.fixture(scope="module")
def client(stack):
    from modelx_amd.client.gpu import GpuClient

    made = [GpuClient(stack[0].url, device=0, num_slots=4, slot_bytes=1 << 20)]
    yield made[0]
    made.clear()
    gc.collect()


@pytest.mark.parametrize("digest_mode", ["chunked", "sha256"])
def test_targz_directory_push(client, stack, devs, tmp_path, digest_mode):
    from modelx_amd.client import Client

    files = {"a.bin": devs["words"][5:5 + 2 * C + 4999],  # unaligned source, ragged length
             "empty.bin": devs["words"][:0],
             "sub/r.bin": devs["random"][1:3002]}
    want = {"a.bin": payload("words")[5:5 + 2 * C + 4999], "empty.bin": b"",
            "sub/r.bin": payload("random")[1:3002]}
    repo = "gzip/" + digest_mode
    client.last_stats.clear()
    manifest = client.push_from_gpu(repo, "v1", {}, dirs={"d": files}, dir_format="tar+gz",
                                    digest_mode=digest_mode, part_bytes=65536)
    desc, = [b for b in manifest.blobs if b.name == "d"]
    assert desc.media_type == wt.MEDIA_TYPE_MODEL_DIRECTORY_TARGZ
    phases = {s["phase"]: s for s in client.last_stats}
    archive_bytes = phases["gpu-tar-pack"]["bytes"]
    assert archive_bytes > 2 * C
    assert phases["push-gzip"]["bytes"] == archive_bytes
    assert phases["push-gzip"]["stored"] == desc.size
    assert phases["push-gzip"]["chunks"] == (archive_bytes + C - 1) // C

    root = stack[1].proc.args[stack[1].proc.args.index("--root") + 1]
    stored = stored_object(os.path.join(root, "modelx", "registry",
                                        pm.blob_digest_path(repo, desc.digest)))
    assert len(stored) == desc.size
    if digest_mode == "sha256":
        assert desc.digest == "sha256:" + hashlib.sha256(stored).hexdigest()
    with tarfile.open(fileobj=io.BytesIO(gzip.decompress(stored))) as tf:
        assert {m.name: tf.extractfile(m).read() for m in tf.getmembers()} == {
            "d/" + k: v for k, v in want.items()}

    back = client.pull_to_gpu(repo, "v1", expand_dirs=True)
    assert {k: to_host(t) for k, t in back.items()} == {"d/" + k: v for k, v in want.items()}

    Client(stack[0].url).pull(repo, "v1", str(tmp_path), quiet=True)
    for k, v in want.items():
        with open(tmp_path / "d" / k, "rb") as f:
            assert f.read() == v

    again = client.push_from_gpu(repo, "v2", {}, dirs={"d": files}, dir_format="tar+gz",
                                 digest_mode=digest_mode, part_bytes=65536)
    assert [b.digest for b in again.blobs if b.name == "d"] == [desc.digest]
