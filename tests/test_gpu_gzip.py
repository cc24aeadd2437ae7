"""gzip on the GPU: ``GpuEngine.gzip_compress_device`` (core/hip/deflate.hip)
equals the host model of test_deflate byte for byte at every payload, length
and source phase, and ``push_from_gpu(dir_format="tar+gz")`` end to end against
modelx-s3d + modelxd."""
import gc
import gzip
import hashlib
import io
import os
import tarfile
import zlib

import pytest

torch = pytest.importorskip("torch")

from modelx_amd import _core
from modelx_amd.wire import paths as pm
from modelx_amd.wire import types as wt

from test_deflate import C, LENGTHS, PAYLOADS, model, payload, words
from test_gpu_aead import stored_object, to_dev, to_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    return _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=2)


@pytest.fixture(scope="module")
def devs():
    return {name: to_dev(payload(name)) for name in PAYLOADS}


def compress(engine, ptr, n):
    """The member and the 16 guard bytes behind it."""
    bound = _core.gzip_compress_bound(n)
    out = torch.full((bound + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    stored = engine.gzip_compress_device(ptr, n, out.data_ptr(), bound)
    got = to_host(out)
    return got[:stored], got[stored:stored + 16]


@pytest.mark.parametrize("offset", [0, 1, 5, 15])
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_device_equals_host_model(engine, devs, name, n, offset):
    got, guard = compress(engine, devs[name].data_ptr() + offset, n)
    assert got == model(name, offset, n)
    assert guard == b"\xa5" * 16
    if name == "words" and n == 2 * C + 1041:
        assert zlib.decompress(got, 31) == payload(name)[offset:offset + n]


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
