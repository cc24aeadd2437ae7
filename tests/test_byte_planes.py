"""Byte-plane zstd on the CPU: the host transform (byteplane_host.hpp) against
an independent numpy model, the literals-only encode mode, the ratio it buys
on bf16 bytes, the annotation parser, and round trips through modelxd with
the CPU client."""
import ctypes
import os
import shutil
import subprocess

import pytest

np = pytest.importorskip("numpy")
# torch before the extension, as everywhere else in the suite: loaded in that
# order the two share torch's HIP runtime. The other way round the process
# holds two runtimes, and on a GPU machine the second one to initialise finds
# no device — for every GPU test that runs later in the same process.
torch = pytest.importorskip("torch")
_core = pytest.importorskip("modelx_amd._core")

from modelx_amd.client import Client  # noqa: E402
from modelx_amd.config import ModelConfig  # noqa: E402
from modelx_amd.wire import errors as er  # noqa: E402
from modelx_amd.wire import types  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = 128 << 10


# ------------------------------------------------------------ host model --

def np_split(raw: bytes, elem: int, group: int) -> bytes:
    """The transform written the numpy way: per group, reshape(-1, E).T,
    with the tail appended."""
    a = np.frombuffer(raw, dtype=np.uint8)
    out = []
    for base in range(0, len(a), group):
        g = a[base:base + group]
        whole = len(g) // elem * elem
        out.append(g[:whole].reshape(-1, elem).T.reshape(-1))
        out.append(g[whole:])
    return np.concatenate(out).tobytes() if out else b""


def _sizes(elem, group):
    return [0, 1, elem - 1, elem, group - 1, group, group + 1, group + elem + 1,
            3 * group + 5]


@pytest.mark.parametrize("elem", [2, 4, 8])
@pytest.mark.parametrize("frame", [16, FRAME], ids=["tiny-group", "real-group"])
def test_host_model_matches_numpy(elem, frame):
    group = elem * frame
    rng = np.random.default_rng(elem * 1000 + frame)
    for size in _sizes(elem, group):
        raw = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        planar = _core.byte_planes_cpu(raw, elem, group, False)
        assert planar == np_split(raw, elem, group), (elem, group, size)
        assert _core.byte_planes_cpu(planar, elem, group, True) == raw, (elem, group, size)


def test_host_model_separates_the_planes():
    """On a full group of E = 2 the first half is the low bytes."""
    raw = bytes([0x11, 0xAA] * 32)
    assert _core.byte_planes_cpu(raw, 2, 64, False) == bytes([0x11] * 32 + [0xAA] * 32)


@pytest.mark.parametrize("elem,group", [(3, 96), (0, 8), (1, 8), (16, 64), (2, 0), (2, 7),
                                        (8, 12)])
def test_host_model_rejects_bad_parameters(elem, group):
    for merge in (False, True):
        with pytest.raises(ValueError):
            _core.byte_planes_cpu(b"\0" * 16, elem, group, merge)


# --------------------------------------------------------- literals-only --

def _bf16_bytes(nbytes: int, seed: int = 0) -> bytes:
    """Little-endian bf16 bytes of seeded N(0, 0.02) values."""
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(nbytes // 2, generator=g) * 0.02).to(torch.bfloat16)
    return t.view(torch.uint8).numpy().tobytes()


def _codec_inputs():
    """The kinds of payload tests/test_zstd.py::TestCpuCodec runs, plus bf16
    bytes as they are and as planes."""
    import random

    rng = random.Random(4321)
    reps = bytearray()
    while len(reps) < 300_000:
        if rng.random() < 0.6 and len(reps) > 64:
            start = len(reps) - rng.randrange(1, min(len(reps), 60_000))
            for k in range(rng.randrange(4, 300)):
                reps.append(reps[start + k])
        else:
            reps.extend(rng.randbytes(rng.randrange(1, 50)))
    inputs = {
        "empty": b"",
        "tiny": b"a",
        "text": b"the quick brown fox jumps over the lazy dog " * 4000,
        "random": rng.randbytes(200_000),
        "zeros": bytes(150_000),
        "repeats": bytes(reps),
        "low-entropy": bytes(rng.choice(b"aab") for _ in range(140_000)),
        "entropy-only": bytes(rng.randrange(64) for _ in range(300_000)),
    }
    inputs["bf16"] = _bf16_bytes(600_000, seed=3)
    inputs["bf16-planes"] = _core.byte_planes_cpu(inputs["bf16"], 2, 2 * FRAME, False)
    return inputs


@pytest.fixture(scope="module")
def codec_inputs():
    return _codec_inputs()


def test_literals_only_roundtrips_with_our_decoder(codec_inputs):
    for name, data in codec_inputs.items():
        blob = _core.zstd_compress_cpu(data, FRAME, literals_only=True)
        assert _core.zstd_decompress_cpu(blob) == data, name
        assert _core.zstd_content_size(blob) == len(data), name


def test_literals_only_decodes_with_libzstd(codec_inputs):
    try:
        z = ctypes.CDLL("libzstd.so.1")
    except OSError:
        pytest.skip("libzstd.so.1 not available")
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_isError.restype = ctypes.c_uint
    for name, data in codec_inputs.items():
        blob = _core.zstd_compress_cpu(data, FRAME, literals_only=True)
        out = ctypes.create_string_buffer(max(len(data), 1))
        n = z.ZSTD_decompress(out, len(data), blob, len(blob))
        assert not z.ZSTD_isError(n), (name, n)
        assert out.raw[:n] == data, name


def test_literals_only_is_off_by_default():
    """The default encode is the unchanged one: LZ still finds the repeats."""
    data = b"modelx " * 100_000
    assert len(_core.zstd_compress_cpu(data, FRAME)) < len(data) // 20
    assert _core.zstd_compress_cpu(data, FRAME) == _core.zstd_compress_cpu(
        data, FRAME, literals_only=False)
    # without LZ a 7-symbol text cannot go below ~2.8 bits per byte
    assert len(_core.zstd_compress_cpu(data, FRAME, literals_only=True)) > len(data) // 4


# ----------------------------------------------------------------- ratio --

def test_planes_ratio_on_bf16():
    """2 MiB of N(0, 0.02) bf16 bytes: planes + literals-only against the
    unchanged path, and against the per-plane entropy bound."""
    raw = _bf16_bytes(2 << 20, seed=0)
    assert len(raw) == 2 << 20
    group = 2 * FRAME
    plain = len(_core.zstd_compress_cpu(raw, FRAME))
    planar = _core.byte_planes_cpu(raw, 2, group, False)
    blob = _core.zstd_compress_cpu(planar, FRAME, literals_only=True)
    assert _core.byte_planes_cpu(_core.zstd_decompress_cpu(blob), 2, group, True) == raw
    got = len(blob)

    a = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 2)
    ideal = 0.0
    for p in range(2):
        counts = np.bincount(a[:, p], minlength=256).astype(np.float64)
        n_p = counts.sum()
        prob = counts[counts > 0] / n_p
        h_p = float(-(prob * np.log2(prob)).sum())  # bits per byte
        ideal += min(n_p, h_p * n_p / 8)
    print(f"plain={plain} planes={got} ratio={got / plain:.4f} "
          f"ideal={ideal:.0f} over-ideal={got / ideal:.4f}")
    assert got <= 0.90 * plain
    assert got <= 1.05 * ideal


# ------------------------------------------------------------- self-test --

def test_selftest_under_sanitizers(tmp_path):
    """tools/byteplane_selftest.cpp: the header-only transform in its own
    process under ASan + UBSan."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = tmp_path / "byteplane_selftest"
    build = subprocess.run(
        [gxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined",
         # static runtimes: the dynamic ASan runtime refuses to start unless
         # it is the first library loaded
         "-static-libasan", "-static-libubsan",
         "-I" + os.path.join(REPO, "core", "include"),
         os.path.join(REPO, "tools", "byteplane_selftest.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stderr == ""


# ----------------------------------------------------- annotation parser --

def test_annotation_accepts_well_formed():
    assert types.parse_byte_planes("2:262144") == (2, 262144)
    assert types.parse_byte_planes("4:524288") == (4, 524288)
    assert types.parse_byte_planes("8:64") == (8, 64)
    assert types.format_byte_planes(2, 262144) == "2:262144"


def test_annotation_absent_is_none():
    assert types.parse_byte_planes("") is None
    assert types.parse_byte_planes(None) is None


@pytest.mark.parametrize("note", ["3:96", "2:0", "2:7", "2", "2:x", "٢:4", True,
                                  "2:4:8", " 2:4", "2:-4", "+2:4", 2, ["2:4"], "2:4\n"])
def test_annotation_refuses_malformed(note):
    with pytest.raises(er.ModelxError) as ei:
        types.parse_byte_planes(note)
    assert ei.value.code == er.ErrCode.UNSUPPORTED


# ------------------------------------------------- round trip via modelxd --

@pytest.fixture(scope="module")
def server(tmp_path_factory):
    from util_servers import start_modelxd_local

    p = start_modelxd_local(str(tmp_path_factory.mktemp("planes-registry")))
    yield p
    p.stop()


@pytest.fixture(scope="module")
def pushed(server, tmp_path_factory):
    """One CPU push with planes=2 of a file of 2G+7 bytes."""
    group = 2 * FRAME
    d = tmp_path_factory.mktemp("planes-model")
    (d / "modelx.yaml").write_text(ModelConfig(description="planes").to_yaml())
    payload = _bf16_bytes(2 * group + 8, seed=11)[:2 * group + 7]
    (d / "weights.bin").write_bytes(payload)
    c = Client(server.url)
    manifest = c.push("lib/planes", "v1", str(d), quiet=True, compress="zstd", planes=2)
    return c, manifest, payload, d


def _weights(manifest):
    (desc,) = [b for b in manifest.blobs if b.name == "weights.bin"]
    return desc


def test_cpu_push_pull_roundtrip(pushed, tmp_path):
    c, manifest, payload, _ = pushed
    desc = _weights(manifest)
    assert desc.media_type == types.MEDIA_TYPE_MODEL_FILE_ZSTD
    assert desc.annotations[types.ANNOTATION_BYTE_PLANES] == f"2:{2 * FRAME}"
    assert desc.annotations[types.ANNOTATION_RAW_SIZE] == str(len(payload))
    # the annotation survives the registry
    stored = _weights(c.get_manifest("lib/planes", "v1"))
    assert stored.annotations[types.ANNOTATION_BYTE_PLANES] == f"2:{2 * FRAME}"
    out = tmp_path / "out"
    c.pull("lib/planes", "v1", str(out), quiet=True)
    assert (out / "weights.bin").read_bytes() == payload


def test_stored_blob_is_the_host_split(pushed):
    c, manifest, payload, _ = pushed
    desc = _weights(manifest)
    blob = b"".join(c.remote.get_blob_content("lib/planes", desc.digest))
    assert len(blob) == desc.size
    assert _core.zstd_decompress_cpu(blob) == _core.byte_planes_cpu(
        payload, 2, 2 * FRAME, False)
    # every frame of a full group holds one plane
    frames = _core.zstd_frames(blob)
    assert [f[3] for f in frames] == [FRAME] * 4 + [7]


def test_planes_zero_keeps_the_plain_zstd_path(server, pushed, tmp_path):
    """planes=0 is the unchanged push: no annotation, the same stored bytes
    as before the option existed."""
    _, _, payload, d = pushed
    from modelx_amd.client.push import parse_manifest

    manifest = parse_manifest(str(d), compress="zstd")
    desc = _weights(manifest)
    assert types.ANNOTATION_BYTE_PLANES not in desc.annotations
    with open(d / ".modelx" / "weights.bin.zst", "rb") as f:
        assert f.read() == _core.zstd_compress_cpu(payload, FRAME)


def test_malformed_annotation_is_refused_on_pull(pushed, tmp_path):
    c, manifest, _, _ = pushed
    bad = types.Manifest.from_dict(manifest.to_dict())
    _weights(bad).annotations[types.ANNOTATION_BYTE_PLANES] = "3:96"
    c.remote.put_manifest("lib/planes", "bad", bad)
    out = tmp_path / "out-bad"
    with pytest.raises(er.ModelxError) as ei:
        c.pull("lib/planes", "bad", str(out), quiet=True)
    assert ei.value.code == er.ErrCode.UNSUPPORTED
    assert not (out / "weights.bin").exists()
    assert not (out / "weights.bin.part").exists()


def test_planes_without_zstd_is_unsupported(pushed):
    c, _, _, d = pushed
    with pytest.raises(er.ModelxError) as ei:
        c.push("lib/planes", "v2", str(d), quiet=True, planes=2)
    assert ei.value.code == er.ErrCode.UNSUPPORTED
    with pytest.raises(er.ModelxError) as ei:
        c.push("lib/planes", "v2", str(d), quiet=True, compress="zstd", planes=3)
    assert ei.value.code == er.ErrCode.UNSUPPORTED


def test_cli_planes_needs_compress(server, pushed, tmp_path, capsys):
    from modelx_amd.cli.main import main as cli_main

    _, _, payload, d = pushed
    ref = f"{server.url}/lib/planes-cli@v1"
    assert cli_main(["push", ref, str(d), "--planes", "2"]) != 0
    assert "UNSUPPORTED" in capsys.readouterr().err
    assert cli_main(["push", ref, str(d), "--compress", "zstd", "--planes", "2"]) == 0
    out = tmp_path / "cli-out"
    assert cli_main(["pull", ref, str(out)]) == 0
    assert (out / "weights.bin").read_bytes() == payload
