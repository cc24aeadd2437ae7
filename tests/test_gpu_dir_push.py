"""Directory push from HBM: the tar pack kernel (core/hip/tar.hip) against
the host layout, ``GpuClient.pack_dir_on_gpu``, ``push_from_gpu(dirs=...)``
and ``pull_to_gpu(expand_dirs=True)`` — round trips on the GPU and through
the ordinary CPU client."""
import hashlib
import io
import os
import tarfile

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    from util_servers import start_modelxd_s3, start_s3d

    s3_root = tmp_path_factory.mktemp("s3-dirpush")
    s3d = start_s3d(str(s3_root))
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    yield mdx, s3d
    mdx.stop()
    s3d.stop()


@pytest.fixture(scope="module")
def client(stack):
    from modelx_amd.client.gpu import GpuClient

    mdx, _ = stack
    return GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20)


def _raw(t) -> bytes:
    """The tensor's bytes on the host (any dtype)."""
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b""


def _as_u8(t):
    return t.view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8,
                                                             device=t.device)


def _store_path(s3d, repo, digest):
    from modelx_amd.wire import paths as pm

    root = s3d.proc.args[s3d.proc.args.index("--root") + 1]
    return os.path.join(root, "modelx", "registry", pm.blob_digest_path(repo, digest))


def _dir_files():
    """A nested path, a zero-size member, a bf16 tensor and a 120-character
    file name; sizes that are no multiple of 512."""
    g = torch.Generator(device="cuda:0").manual_seed(7)

    def rnd(n):
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0", generator=g)

    return {
        "layer0/w.bin": rnd(3 * MIB + 5),
        "layer0/deeper/still/b.bin": rnd(777),
        "empty.bin": torch.empty(0, dtype=torch.uint8, device="cuda:0"),
        "scales.bf16": torch.randn(1000, 33, device="cuda:0", generator=g).to(torch.bfloat16),
        "x-" + "l" * 114 + ".bin": rnd(4097),
        "ids.i64": torch.arange(321, dtype=torch.int64, device="cuda:0"),
    }


@pytest.fixture(scope="module")
def pushed(client):
    """One push shared by the round-trip tests: v1 (chunked digest)."""
    files = _dir_files()
    assert len("x-" + "l" * 114 + ".bin") == 120
    solo = torch.randint(0, 256, (MIB + 3,), dtype=torch.uint8, device="cuda:0")
    client.last_stats.clear()
    manifest = client.push_from_gpu("dirpush/model", "v1", {"solo.bin": solo},
                                    dirs={"shards": files})
    return files, solo, manifest


# ------------------------------------------------------ kernel vs layout --

def test_pack_kernel_matches_layout_all_phases(client):
    """engine.tar_pack against the archive assembled on the CPU from
    tar_pack_layout: every source phase 0..15 with the small sizes, phases
    0/1/8/15 across the 4 MiB piece boundary, destination pre-filled so an
    unwritten pad byte or an overrun shows."""
    from modelx_amd import _core

    small = [0, 1, 15, 16, 17, 511, 512, 513]
    big = [4 * MIB - 1, 4 * MIB, 4 * MIB + 1, 9 * MIB + 777]
    base = torch.randint(0, 256, (10 * MIB,), dtype=torch.uint8, device="cuda:0")
    assert base.data_ptr() % 16 == 0
    cases = [(k, n) for n in small for k in range(16)]
    cases += [(k, n) for n in big for k in (0, 1, 8, 15)]
    views = [base[k:k + n] for k, n in cases]
    names = [f"m/{n}_{k}" for k, n in cases]
    members = [(nm, v.data_ptr(), v.numel()) for nm, v in zip(names, views)]
    for (k, n), v in zip(cases, views):
        assert v.numel() == n and (n == 0 or v.data_ptr() % 16 == k)

    lay = _core.tar_pack_layout([(nm, n) for nm, (_, n) in zip(names, cases)])
    total = lay["total"]
    host = base.cpu().numpy().tobytes()
    expect = bytearray()
    hoff = 0
    for (k, n), e in zip(cases, lay["entries"]):
        assert len(expect) == e["header_off"]
        expect += lay["headers"][hoff:hoff + e["header_len"]]
        hoff += e["header_len"]
        assert len(expect) == e["payload_off"]
        expect += host[k:k + n]
        expect += bytes(-n % 512)
    expect += bytes(1024)
    assert len(expect) == total

    guard = 4096
    dst = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert client.engine.tar_pack(dst.data_ptr(), total, members) == total
    got = dst.cpu().numpy().tobytes()
    if got[:total] != bytes(expect):
        first = next(i for i in range(total) if got[i] != expect[i])
        raise AssertionError(f"archive differs from the layout first at byte {first}")
    assert got[total:] == b"\xa5" * guard

    # capacity is checked before anything is written
    with pytest.raises(RuntimeError):
        client.engine.tar_pack(dst.data_ptr(), total - 1, members)


# --------------------------------------------------------------- tarfile --

def test_packed_archive_readable_by_tarfile(client):
    files = {
        "plain.bin": torch.randint(0, 256, (1000,), dtype=torch.uint8, device="cuda:0"),
        # 101+ bytes with a usable split: ustar prefix field
        "p" * 60 + "/" + "q" * 80: torch.randint(0, 256, (513,), dtype=torch.uint8,
                                                 device="cuda:0"),
        # no slash inside the 200-byte file name: PAX path= record
        "r" * 200: torch.randint(0, 256, (MIB + 1,), dtype=torch.uint8, device="cuda:0"),
        "zero": torch.empty(0, dtype=torch.uint8, device="cuda:0"),
    }
    client.last_stats.clear()
    archive = client.pack_dir_on_gpu("top", files)
    assert archive.dtype == torch.uint8 and archive.device.index == 0
    st = next(s for s in client.last_stats if s["phase"] == "gpu-tar-pack")
    assert st["bytes"] == archive.numel() and st["members"] == len(files)
    blob = archive.cpu().numpy().tobytes()
    with tarfile.open(fileobj=io.BytesIO(blob), mode="r:") as tf:
        infos = tf.getmembers()
        assert [ti.name for ti in infos] == sorted(f"top/{n}" for n in files)
        for ti in infos:
            assert tf.extractfile(ti).read() == _raw(files[ti.name.split("/", 1)[1]])
            assert ti.mode == 0o644 and ti.mtime == 0 and ti.uid == 0 and ti.gid == 0
    # the GPU index agrees with tarfile on every resolved name
    entries = client.engine.tar_index(archive.data_ptr(), archive.numel())
    assert [e["name"] for e in entries] == [ti.name for ti in infos]
    assert [e["size"] for e in entries] == [ti.size for ti in infos]


# ------------------------------------------------------- GPU round trip --

def test_dir_push_pull_roundtrip_on_gpu(client, pushed):
    from modelx_amd.wire import types as wt

    files, solo, manifest = pushed
    blobs = {b.name: b for b in manifest.blobs}
    shards = blobs["shards"]
    assert shards.media_type == wt.MEDIA_TYPE_MODEL_DIRECTORY_TAR
    assert shards.digest.startswith("sha256c")
    assert shards.annotations[wt.ANNOTATION_CHUNK_DIGEST] == shards.digest
    assert int(shards.annotations[wt.ANNOTATION_CHUNK_SIZE]) > 0
    assert shards.annotations[wt.ANNOTATION_LEAVES_BLOB] == blobs["shards.leaves"].digest
    assert blobs["shards.leaves"].media_type == wt.MEDIA_TYPE_MODEL_LEAVES
    assert blobs["solo.bin"].media_type == wt.MEDIA_TYPE_MODEL_FILE
    assert any(s.get("phase") == "gpu-tar-pack" and s["members"] == len(files)
               for s in client.last_stats)
    stored = client.remote.get_manifest("dirpush/model", "v1")
    assert {b.name for b in stored.blobs} == set(blobs)

    out = client.pull_to_gpu("dirpush/model", "v1", expand_dirs=True)
    assert set(out) == {"solo.bin"} | {f"shards/{n}" for n in files}
    assert torch.equal(out["solo.bin"], solo)
    for n, t in files.items():
        got = out[f"shards/{n}"]
        assert got.dtype == torch.uint8
        assert torch.equal(got, _as_u8(t).reshape(-1)), n

    # directory blobs share the worker pool and honour verify=False
    fast = client.pull_to_gpu("dirpush/model", "v1", expand_dirs=True, parallel=3,
                              verify=False)
    assert set(fast) == set(out)
    assert all(torch.equal(fast[n], out[n]) for n in out)

    raw = client.pull_to_gpu("dirpush/model", "v1")
    assert set(raw) == {"solo.bin", "shards"}
    assert raw["shards"].numel() == shards.size
    assert torch.equal(raw["shards"], client.pack_dir_on_gpu("shards", files))


def test_dir_push_single_blob_path(client):
    """dirs alone (one blob): the per-blob path, not the many-blob one."""
    from modelx_amd.wire import types as wt

    files = {"a.bin": torch.randint(0, 256, (70001,), dtype=torch.uint8, device="cuda:0")}
    m = client.push_from_gpu("dirpush/single", "v1", {}, dirs={"only": files})
    blobs = {b.name: b for b in m.blobs}
    assert set(blobs) == {"only", "only.leaves"}
    assert blobs["only"].media_type == wt.MEDIA_TYPE_MODEL_DIRECTORY_TAR
    assert blobs["only"].annotations[wt.ANNOTATION_LEAVES_BLOB] == blobs["only.leaves"].digest
    out = client.pull_to_gpu("dirpush/single", "v1", expand_dirs=True)
    assert set(out) == {"only/a.bin"}
    assert torch.equal(out["only/a.bin"], files["a.bin"])


# ------------------------------------------------------- CPU round trip --

def test_dir_roundtrip_to_cpu_client(stack, client, pushed, tmp_path):
    from modelx_amd.client import Client

    mdx, _ = stack
    files, solo, _ = pushed
    out = tmp_path / "cpu-out"
    Client(mdx.url).pull("dirpush/model", "v1", str(out), quiet=True)
    assert (out / "solo.bin").read_bytes() == _raw(solo)
    for n, t in files.items():
        assert (out / "shards" / n).read_bytes() == _raw(t), n
    on_disk = {os.path.relpath(os.path.join(r, f), out / "shards")
               for r, _, fs in os.walk(out / "shards") for f in fs}
    assert on_disk == set(files)


def test_dir_push_sha256_digest_mode(stack, client, pushed, tmp_path):
    from modelx_amd.client import Client
    from modelx_amd.wire import types as wt

    mdx, _ = stack
    files, solo, manifest = pushed
    m = client.push_from_gpu("dirpush/model", "canon", {"solo.bin": solo},
                             dirs={"shards": files}, digest_mode="sha256")
    shards = next(b for b in m.blobs if b.name == "shards")
    # the reference hashes the bytes that come back from the store
    archive = client.pull_to_gpu("dirpush/model", "canon")["shards"].cpu().numpy().tobytes()
    assert shards.digest == "sha256:" + hashlib.sha256(archive).hexdigest()
    assert shards.size == len(archive)
    assert archive == client.pack_dir_on_gpu("shards", files).cpu().numpy().tobytes()
    v1 = next(b for b in manifest.blobs if b.name == "shards")
    assert shards.annotations[wt.ANNOTATION_CHUNK_DIGEST] == v1.digest
    assert shards.media_type == wt.MEDIA_TYPE_MODEL_DIRECTORY_TAR
    out = tmp_path / "canon-out"
    Client(mdx.url).pull("dirpush/model", "canon", str(out), quiet=True)
    for n, t in files.items():
        assert (out / "shards" / n).read_bytes() == _raw(t), n


# ------------------------------------------------ determinism and dedup --

def test_dir_digest_is_deterministic(client, pushed):
    files, solo, manifest = pushed
    v1 = next(b for b in manifest.blobs if b.name == "shards")
    client.last_stats.clear()
    m2 = client.push_from_gpu("dirpush/model", "v2", {"solo.bin": solo},
                              dirs={"shards": files})
    assert next(b for b in m2.blobs if b.name == "shards").digest == v1.digest
    # the archive already exists: HEAD-dedup, no second upload of its bytes
    assert not any(s.get("phase") == "push-upload" and s["bytes"] == v1.size
                   for s in client.last_stats)
    shuffled = {n: files[n] for n in reversed(list(files))}
    assert list(shuffled) != list(files)
    m3 = client.push_from_gpu("dirpush/model", "v3", {"solo.bin": solo},
                              dirs={"shards": shuffled})
    assert next(b for b in m3.blobs if b.name == "shards").digest == v1.digest


# ------------------------------------------------------------ rejections --

def _bad_pushes():
    ok = torch.zeros(1000, dtype=torch.uint8, device="cuda:0")
    wide = torch.zeros(64, 64, dtype=torch.uint8, device="cuda:0")
    return {
        "cpu-tensor": (ValueError, {"w": ok}, {"d": {"a": torch.zeros(10, dtype=torch.uint8)}},
                       {}),
        "non-contiguous": (ValueError, {"w": ok}, {"d": {"a": wide[:, ::2]}}, {}),
        "dotdot": (ValueError, {"w": ok}, {"d": {"a/../b": ok}}, {}),
        "dir-equals-tensor": (ValueError, {"w": ok}, {"w": {"a": ok}}, {}),
        "dir-equals-leaves-sidecar": (ValueError, {"w": ok}, {"w.leaves": {"a": ok}}, {}),
        "dir-equals-config": (ValueError, {"w": ok}, {"modelx.yaml": {"a": ok}}, {}),
        "trailing-slash": (ValueError, {"w": ok}, {"d": {"a/": ok}}, {}),
        "zstd-with-dirs": (None, {"w": ok}, {"d": {"a": ok}}, {"compress": "zstd"}),
    }


@pytest.mark.parametrize("case", ["cpu-tensor", "non-contiguous", "dotdot",
                                  "dir-equals-tensor", "dir-equals-leaves-sidecar",
                                  "dir-equals-config", "trailing-slash", "zstd-with-dirs"])
def test_dir_push_rejections_upload_nothing(stack, client, case):
    from modelx_amd.wire import errors as er

    _, s3d = stack
    exc_type, tensors, dirs, kwargs = _bad_pushes()[case]
    repo = f"dirpush/reject-{case}"
    if exc_type is None:
        with pytest.raises(er.ModelxError) as exc:
            client.push_from_gpu(repo, "v1", tensors, dirs=dirs, **kwargs)
        assert exc.value.code == er.ErrCode.UNSUPPORTED
    else:
        with pytest.raises(exc_type):
            client.push_from_gpu(repo, "v1", tensors, dirs=dirs, **kwargs)
    with pytest.raises(er.ModelxError):
        client.remote.get_manifest(repo, "v1")
    # not even the config blob went out
    blobs_dir = os.path.dirname(os.path.dirname(_store_path(s3d, repo, "sha256:" + "0" * 64)))
    assert not os.path.exists(blobs_dir)


def test_pack_dir_rejects_wrong_device_and_layout(client):
    ok = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError):
        client.pack_dir_on_gpu("d", {"a": torch.zeros(16, dtype=torch.uint8)})
    with pytest.raises(ValueError):
        client.pack_dir_on_gpu("d", {"a": torch.zeros(8, 8, device="cuda:0").t()})
    with pytest.raises(ValueError):
        client.pack_dir_on_gpu("", {"a": ok})
    with pytest.raises(ValueError):
        client.pack_dir_on_gpu("d", {"a\0b": ok})


# ------------------------------------------------------------ corruption --

def test_dir_pull_detects_corruption(stack, client):
    """One flipped byte in the stored archive. A blob with a leaves sidecar
    refetches its bad chunk, and the store hands back the same flipped byte,
    so the pull ends in DIGEST_INVALID exactly as for a file blob."""
    from modelx_amd.wire import errors as er

    _, s3d = stack
    files = {"a.bin": torch.randint(0, 256, (2 * MIB,), dtype=torch.uint8, device="cuda:0"),
             "b.bin": torch.randint(0, 256, (MIB,), dtype=torch.uint8, device="cuda:0")}
    m = client.push_from_gpu("dirpush/corrupt", "v1", {}, dirs={"shards": files})
    desc = next(b for b in m.blobs if b.name == "shards")
    obj = _store_path(s3d, "dirpush/corrupt", desc.digest)
    with open(obj, "r+b") as f:
        f.seek(MIB + 12345)
        b0 = f.read(1)
        f.seek(MIB + 12345)
        f.write(bytes([b0[0] ^ 1]))
    with pytest.raises(er.ModelxError) as exc:
        client.pull_to_gpu("dirpush/corrupt", "v1", expand_dirs=True)
    assert exc.value.code == er.ErrCode.DIGEST_INVALID
