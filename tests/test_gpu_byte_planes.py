"""Byte-plane zstd on the GPU: the split/merge kernels (core/hip/byteplane.hip)
against the host model, and ``push_from_gpu(compress="zstd", planes=...)`` /
``pull_to_gpu`` / ``pull_many`` end to end against modelx-s3d + modelxd, in
both directions with the CPU client."""
import os

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FRAME = 128 << 10
CANARY = 64
LEAD = 256  # destination views start this far into their allocation (+ shift)


@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    from util_servers import start_modelxd_s3, start_s3d

    s3_root = tmp_path_factory.mktemp("s3-planes")
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


@pytest.fixture(scope="module")
def engine():
    from modelx_amd import _core

    return _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=2)


def _raw(t) -> bytes:
    """The tensor's bytes on the host (any dtype)."""
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b""


def _store_path(s3d, repo, digest):
    from modelx_amd.wire import paths as pm

    root = s3d.proc.args[s3d.proc.args.index("--root") + 1]
    return os.path.join(root, "modelx", "registry", pm.blob_digest_path(repo, digest))


# ------------------------------------------------- kernels vs host model --

def _sizes(elem, group):
    return [1, group - 1, group, group + 1, 2 * group + elem + 3]


class _Dst:
    """A destination view with CANARY bytes of 0xA5 on both sides."""

    def __init__(self, size, shift):
        self.size = size
        self.lo = LEAD + shift
        self.buf = torch.full((self.lo + size + CANARY + 16,), 0xA5, dtype=torch.uint8,
                              device="cuda:0")
        self.view = self.buf[self.lo:self.lo + size]

    def check(self, expect: bytes, what):
        host = self.buf.cpu().numpy().tobytes()
        assert host[self.lo - CANARY:self.lo] == b"\xA5" * CANARY, f"{what}: canary before"
        assert host[self.lo + self.size:self.lo + self.size + CANARY] == b"\xA5" * CANARY, \
            f"{what}: canary after"
        assert host[self.lo:self.lo + self.size] == expect, what


def _src(data: bytes, shift):
    import numpy as np

    buf = torch.zeros(LEAD + shift + len(data), dtype=torch.uint8, device="cuda:0")
    buf[LEAD + shift:] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())
    return buf, buf[LEAD + shift:]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "sliced-1"])
@pytest.mark.parametrize("frame", [64, FRAME], ids=["G=64E", "G=128KiE"])
@pytest.mark.parametrize("elem", [2, 4, 8])
def test_kernels_match_host_model(engine, elem, frame, shift):
    """Split and merge at every edge size, all sizes as items of ONE call,
    with a zero-size item among them; canaries around every destination."""
    import numpy as np

    from modelx_amd import _core

    group = elem * frame
    rng = np.random.default_rng(elem * 131 + frame + shift)
    for merge in (False, True):
        items, checks, keep = [], [], []
        for size in _sizes(elem, group):
            data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
            sbuf, sview = _src(data, shift)
            dst = _Dst(size, shift)
            if shift == 0:
                assert sview.data_ptr() % 256 == 0 and dst.view.data_ptr() % 256 == 0
            else:
                assert sview.data_ptr() % 16 == 1 and dst.view.data_ptr() % 16 == 1
            items.append((sview.data_ptr(), dst.view.data_ptr(), size, elem, group))
            checks.append((dst, _core.byte_planes_cpu(data, elem, group, merge), size))
            keep.append(sbuf)
        # a zero-size item is a no-op, whatever its pointers
        zdst = _Dst(0, shift)
        items.insert(2, (0, zdst.view.data_ptr(), 0, elem, group))
        torch.cuda.synchronize()
        engine.byte_planes(items, merge)
        for dst, expect, size in checks:
            dst.check(expect, f"E={elem} G={group} size={size} merge={merge} shift={shift}")
        zdst.check(b"", "zero-size item")


def test_split_then_merge_is_identity_on_device(engine):
    """Both kernels chained on the device, mixed element sizes in one call."""
    sizes = [(2, 3 * 2 * FRAME + 5), (4, 4 * FRAME), (8, 8 * FRAME + 9)]
    srcs = [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0") for _, n in sizes]
    mids = [torch.empty_like(s) for s in srcs]
    outs = [torch.empty_like(s) for s in srcs]
    torch.cuda.synchronize()
    engine.byte_planes([(s.data_ptr(), m.data_ptr(), s.numel(), e, e * FRAME)
                        for s, m, (e, _) in zip(srcs, mids, sizes)], False)
    engine.byte_planes([(m.data_ptr(), o.data_ptr(), m.numel(), e, e * FRAME)
                        for m, o, (e, _) in zip(mids, outs, sizes)], True)
    for s, m, o in zip(srcs, mids, outs):
        assert torch.equal(s, o)
        assert not torch.equal(s, m)


@pytest.mark.parametrize("bad", ["elem", "group-zero", "group-multiple", "overlap"])
def test_bad_items_raise_before_anything_runs(engine, bad):
    """A bad item anywhere in the list: RuntimeError, and not even the good
    item before it has run."""
    n = 4096
    src = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda:0")
    dst = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    good = (src.data_ptr(), dst.data_ptr(), n, 2, 128)
    second = {
        "elem": (src.data_ptr() + n, dst.data_ptr() + n, n, 3, 96),
        "group-zero": (src.data_ptr() + n, dst.data_ptr() + n, n, 2, 0),
        "group-multiple": (src.data_ptr() + n, dst.data_ptr() + n, n, 4, 6),
        "overlap": (src.data_ptr(), src.data_ptr() + n - 1, n, 2, 128),
    }[bad]
    before = src.clone()
    torch.cuda.synchronize()
    for merge in (False, True):
        with pytest.raises(RuntimeError):
            engine.byte_planes([good, second], merge)
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
    assert torch.equal(src, before)


# ------------------------------------------------------------ end to end --

def _randn(n, dtype, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    return (torch.randn(n, device="cuda:0", generator=g) * 0.02).to(dtype)


def _blob(manifest, name):
    (d,) = [b for b in manifest.blobs if b.name == name]
    return d


def _phases(client, phase):
    return [s for s in client.last_stats if s.get("phase") == phase]


@pytest.fixture(scope="module")
def pushed_bf16(client):
    """planes=2 push of a bf16 tensor of 2G+6 bytes."""
    group = 2 * FRAME
    t = _randn((2 * group + 6) // 2, torch.bfloat16, seed=1)
    assert t.numel() * t.element_size() == 2 * group + 6
    client.last_stats.clear()
    manifest = client.push_from_gpu("planes/bf16", "v1", {"w.bf16": t}, compress="zstd",
                                    planes=2)
    assert len(_phases(client, "push-byte-planes-split")) == 1
    return t, manifest


@pytest.fixture(scope="module")
def pushed_auto(client):
    """planes="auto" push of an fp32 and a uint8 tensor: one planes blob and
    one plain +zstd blob in one version."""
    f = _randn((2 * 4 * FRAME + 12) // 4, torch.float32, seed=2)
    u = torch.randint(0, 256, (300_001,), dtype=torch.uint8, device="cuda:0")
    client.last_stats.clear()
    manifest = client.push_from_gpu("planes/auto", "v1", {"f.f32": f, "u.u8": u},
                                    compress="zstd", planes="auto")
    assert len(_phases(client, "push-byte-planes-split")) == 1
    return f, u, manifest


def test_push_planes_descriptor_and_stored_bytes(stack, pushed_bf16):
    from modelx_amd import _core
    from modelx_amd.wire import types

    _, s3d = stack
    t, manifest = pushed_bf16
    desc = _blob(manifest, "w.bf16")
    raw = _raw(t)
    assert desc.media_type == types.MEDIA_TYPE_MODEL_FILE_ZSTD
    assert desc.annotations[types.ANNOTATION_BYTE_PLANES] == f"2:{2 * FRAME}"
    assert desc.annotations[types.ANNOTATION_RAW_SIZE] == str(len(raw))
    with open(_store_path(s3d, "planes/bf16", desc.digest), "rb") as f:
        stored = f.read()
    assert len(stored) == desc.size
    assert _core.zstd_decompress_cpu(stored) == _core.byte_planes_cpu(raw, 2, 2 * FRAME, False)
    # literals-only planes beat what the plain path stores for these bytes
    assert desc.size < len(_core.zstd_compress_cpu(raw, FRAME))


def test_pull_to_gpu_single_planes_blob(client, pushed_bf16):
    t, _ = pushed_bf16
    client.last_stats.clear()
    back = client.pull_to_gpu("planes/bf16", "v1")
    assert torch.equal(back["w.bf16"], t.view(torch.uint8))
    assert len(_phases(client, "pull-byte-planes-merge")) == 1


def test_cpu_client_pulls_gpu_pushed_planes(stack, pushed_bf16, pushed_auto, tmp_path):
    from modelx_amd.client import Client

    mdx, _ = stack
    t, _ = pushed_bf16
    f, u, _ = pushed_auto
    c = Client(mdx.url)
    c.pull("planes/bf16", "v1", str(tmp_path / "a"), quiet=True)
    assert (tmp_path / "a" / "w.bf16").read_bytes() == _raw(t)
    c.pull("planes/auto", "v1", str(tmp_path / "b"), quiet=True)
    assert (tmp_path / "b" / "f.f32").read_bytes() == _raw(f)
    assert (tmp_path / "b" / "u.u8").read_bytes() == _raw(u)


def test_auto_annotates_by_element_size(stack, pushed_auto):
    from modelx_amd import _core
    from modelx_amd.wire import types

    _, s3d = stack
    f, u, manifest = pushed_auto
    fd, ud = _blob(manifest, "f.f32"), _blob(manifest, "u.u8")
    assert fd.annotations[types.ANNOTATION_BYTE_PLANES] == f"4:{4 * FRAME}"
    assert types.ANNOTATION_BYTE_PLANES not in ud.annotations
    assert ud.media_type == fd.media_type == types.MEDIA_TYPE_MODEL_FILE_ZSTD
    with open(_store_path(s3d, "planes/auto", fd.digest), "rb") as fh:
        assert _core.zstd_decompress_cpu(fh.read()) == _core.byte_planes_cpu(
            _raw(f), 4, 4 * FRAME, False)
    with open(_store_path(s3d, "planes/auto", ud.digest), "rb") as fh:
        assert _core.zstd_decompress_cpu(fh.read()) == _raw(u)


def test_batched_pull_merges_once(client, pushed_auto):
    """One planes blob and one plain +zstd blob in one version go through
    the batched decode: one merge call for the batch."""
    f, u, _ = pushed_auto
    client.last_stats.clear()
    back = client.pull_to_gpu("planes/auto", "v1")
    assert torch.equal(back["f.f32"], f.view(torch.uint8))
    assert torch.equal(back["u.u8"], u)
    assert len(_phases(client, "pull-zstd-decompress-batched")) == 1
    merges = _phases(client, "pull-byte-planes-merge")
    assert len(merges) == 1 and merges[0]["blobs"] == 1


def test_pull_many_merges_once_per_batch(client, pushed_bf16):
    """Two versions, each with one planes blob: pull_many batches them
    across versions, with exactly one merge entry."""
    t, _ = pushed_bf16
    t2 = _randn(70_001, torch.bfloat16, seed=5)
    client.push_from_gpu("planes/bf16", "v2", {"w.bf16": t2}, compress="zstd", planes="auto")
    client.last_stats.clear()
    got = client.pull_many("planes/bf16", ["v1", "v2"])
    assert torch.equal(got["v1"]["w.bf16"], t.view(torch.uint8))
    assert torch.equal(got["v2"]["w.bf16"], t2.view(torch.uint8))
    merges = _phases(client, "pull-byte-planes-merge")
    assert len(merges) == 1 and merges[0]["blobs"] == 2


def test_gpu_pulls_cpu_pushed_planes(stack, client, tmp_path):
    from modelx_amd.client import Client
    from modelx_amd.config import ModelConfig
    from modelx_amd.wire import types

    mdx, _ = stack
    d = tmp_path / "model"
    d.mkdir()
    (d / "modelx.yaml").write_text(ModelConfig(description="cpu planes").to_yaml())
    payload = _raw(_randn((4 * FRAME + 4 * 999 + 4) // 4, torch.float32, seed=9)) + b"\x01\x02\x03"
    (d / "w.f32").write_bytes(payload)
    manifest = Client(mdx.url).push("planes/cpu", "v1", str(d), quiet=True, compress="zstd",
                                    planes=4)
    assert _blob(manifest, "w.f32").annotations[types.ANNOTATION_BYTE_PLANES] == \
        f"4:{4 * FRAME}"
    back = client.pull_to_gpu("planes/cpu", "v1")
    assert _raw(back["w.f32"]) == payload


def _republish(client, repo, manifest, version, name, key, value):
    from modelx_amd.wire import types

    m = types.Manifest.from_dict(manifest.to_dict())
    _blob(m, name).annotations[key] = value
    client.remote.put_manifest(repo, version, m)


def test_wrong_raw_digest_fails_after_the_merge(client, pushed_bf16, pushed_auto):
    """The raw digest describes the interleaved bytes and is checked on the
    merged output: a wrong one is DIGEST_INVALID on both pull paths."""
    from modelx_amd.wire import errors as er
    from modelx_amd.wire import types

    def flipped(desc):
        rd = desc.annotations[types.ANNOTATION_RAW_DIGEST]
        return rd[:-1] + ("0" if rd[-1] != "0" else "1")

    _, manifest = pushed_bf16
    _republish(client, "planes/bf16", manifest, "bad-digest", "w.bf16",
               types.ANNOTATION_RAW_DIGEST, flipped(_blob(manifest, "w.bf16")))
    with pytest.raises(er.ModelxError) as ei:
        client.pull_to_gpu("planes/bf16", "bad-digest")
    assert ei.value.code == er.ErrCode.DIGEST_INVALID

    _, _, manifest = pushed_auto
    _republish(client, "planes/auto", manifest, "bad-digest", "f.f32",
               types.ANNOTATION_RAW_DIGEST, flipped(_blob(manifest, "f.f32")))
    with pytest.raises(er.ModelxError) as ei:
        client.pull_to_gpu("planes/auto", "bad-digest")
    assert ei.value.code == er.ErrCode.DIGEST_INVALID


def test_planar_bytes_never_pass_for_the_tensor(client, pushed_bf16):
    """Dropping the annotation (what a client that predates it sees) fails the
    raw-digest check instead of returning planar bytes."""
    from modelx_amd.wire import errors as er
    from modelx_amd.wire import types

    _, manifest = pushed_bf16
    m = types.Manifest.from_dict(manifest.to_dict())
    del _blob(m, "w.bf16").annotations[types.ANNOTATION_BYTE_PLANES]
    client.remote.put_manifest("planes/bf16", "no-note", m)
    with pytest.raises(er.ModelxError) as ei:
        client.pull_to_gpu("planes/bf16", "no-note")
    assert ei.value.code == er.ErrCode.DIGEST_INVALID


def test_malformed_annotation_is_refused(client, pushed_bf16, pushed_auto):
    from modelx_amd.wire import errors as er
    from modelx_amd.wire import types

    _, manifest = pushed_bf16
    _republish(client, "planes/bf16", manifest, "bad-note", "w.bf16",
               types.ANNOTATION_BYTE_PLANES, "3:96")
    with pytest.raises(er.ModelxError) as ei:
        client.pull_to_gpu("planes/bf16", "bad-note")
    assert ei.value.code == er.ErrCode.UNSUPPORTED
    _, _, manifest = pushed_auto
    _republish(client, "planes/auto", manifest, "bad-note", "f.f32",
               types.ANNOTATION_BYTE_PLANES, "4:6")
    with pytest.raises(er.ModelxError) as ei:
        client.pull_to_gpu("planes/auto", "bad-note")
    assert ei.value.code == er.ErrCode.UNSUPPORTED


def test_planes_without_compress_is_unsupported(client):
    from modelx_amd.wire import errors as er

    t = torch.zeros(16, dtype=torch.bfloat16, device="cuda:0")
    for planes in (2, "auto"):
        with pytest.raises(er.ModelxError) as ei:
            client.push_from_gpu("planes/none", "v1", {"t": t}, planes=planes)
        assert ei.value.code == er.ErrCode.UNSUPPORTED
    with pytest.raises(er.ModelxError) as ei:
        client.push_from_gpu("planes/none", "v1", {"t": t}, compress="zstd", planes=3)
    assert ei.value.code == er.ErrCode.UNSUPPORTED
