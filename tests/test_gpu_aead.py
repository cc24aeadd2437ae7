"""ChaCha20-Poly1305 on the GPU: ``GpuEngine.aead_seal`` / ``aead_open``
(core/hip/aead.hip) against the reference of test_aead at the quad, block,
row, segment and last-flag boundaries, and ``encrypt=True`` end to end against
modelx-s3d + modelxd."""
import functools
import gc
import os

import pytest

torch = pytest.importorskip("torch")

from modelx_amd import _core
from modelx_amd.client import gpu_rules as rules
from modelx_amd.wire import errors as er
from modelx_amd.wire import paths as pm

from test_aead import DATA, KEY, LENGTHS, S, ref_seal, seeded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    return _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=2)


def to_dev(data: bytes):
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


def to_host(t) -> bytes:
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def dev():
    """DATA in HBM, 16 B aligned: an offset into it is the misalignment."""
    return to_dev(DATA)


@functools.lru_cache(maxsize=None)
def ref(offset: int, n: int, seg: int = S) -> bytes:
    return ref_seal(KEY, DATA[offset:offset + n], seg)


@pytest.mark.parametrize("offset", [0, 1, 5, 15])
@pytest.mark.parametrize("n", LENGTHS)
def test_seal_matches_reference(engine, dev, n, offset):
    out = torch.zeros(rules.sealed_size(n, S) + 16, dtype=torch.uint8, device="cuda:0")
    engine.aead_seal(KEY, dev.data_ptr() + offset, n, out.data_ptr(), S)
    got = to_host(out)
    assert got[:-16] == ref(offset, n)
    assert got[-16:] == bytes(16)  # nothing written past the last tag


@pytest.mark.parametrize("n", LENGTHS)
def test_open_matches_reference(engine, n):
    stored = to_dev(ref(0, n) + b"\xaa" * 16)
    assert engine.aead_open(KEY, stored.data_ptr(), rules.sealed_size(n, S), n, S) == -1
    got = to_host(stored)
    assert got[:n] == DATA[:n]
    assert got[n:] == ref(0, n)[n:] + b"\xaa" * 16  # tags and what follows untouched


def test_more_segments_than_the_grid(engine):
    """8192 + 300 one-row segments of distinct content: the capped grid has
    8192 waves, so the last 300 are reached by its stride."""
    n = (8192 + 300) * 1024
    data = seeded(n, 23)
    want = ref_seal(KEY, data, 1024)
    src = to_dev(data)
    out = torch.empty(len(want), dtype=torch.uint8, device="cuda:0")
    engine.aead_seal(KEY, src.data_ptr(), n, out.data_ptr(), 1024)
    assert to_host(out) == want
    assert engine.aead_open(KEY, out.data_ptr(), len(want), n, 1024) == -1
    assert torch.equal(out[:n], src)


TAMPER_N = 5 * 1024 + 100  # six segments at 1024, the last one short


def _flip_ciphertext(b, k):
    b[k * 1024 + 37] ^= 0x20
    return b, TAMPER_N, k


def _flip_tag(b, k):
    b[TAMPER_N + 16 * k + 9] ^= 0x01
    return b, TAMPER_N, k


def _swap_segments(b, k):
    """Segments k and k + 1 (both whole), ciphertext and tag: the nonce
    carries the index."""
    for base, ln in ((0, 1024), (TAMPER_N, 16)):
        lo, hi = base + k * ln, base + (k + 1) * ln
        b[lo:lo + ln], b[hi:hi + ln] = b[hi:hi + ln], b[lo:lo + ln]
    return b, TAMPER_N, k


def _drop_last_segment(b, k):
    """Truncated to five whole segments: the fifth was not sealed as last."""
    return b[:5 * 1024] + b[TAMPER_N:TAMPER_N + 16 * 5], 5 * 1024, 4


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("tamper", [_flip_ciphertext, _flip_tag, _swap_segments,
                                    _drop_last_segment])
def test_open_names_the_first_bad_segment(engine, tamper, k):
    stored, n, want = tamper(bytearray(ref(0, TAMPER_N, 1024)), k)
    t = to_dev(bytes(stored))
    assert engine.aead_open(KEY, t.data_ptr(), len(stored), n, 1024) == want


def test_engine_refuses_bad_arguments(engine, dev):
    out = torch.empty(4096, dtype=torch.uint8, device="cuda:0")
    for args in ((KEY[:31], dev.data_ptr(), 100, out.data_ptr(), S),
                 (KEY, dev.data_ptr(), 100, out.data_ptr(), 1000),
                 (KEY, dev.data_ptr(), 100, out.data_ptr() + 4, S)):
        with pytest.raises((ValueError, RuntimeError)):
            engine.aead_seal(*args)
    with pytest.raises((ValueError, RuntimeError)):
        engine.aead_open(KEY, out.data_ptr(), 100 + 15, 100, S)


# ------------------------------------------------------------ end to end --

@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    from util_servers import start_modelxd_s3, start_s3d

    s3d = start_s3d(str(tmp_path_factory.mktemp("s3-aead")))
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    yield mdx, s3d
    mdx.stop()
    s3d.stop()


@pytest.fixture(scope="module")
def clients(stack):
    """GpuClients with the key, without one and with another."""
    from modelx_amd.client.gpu import GpuClient

    made = [GpuClient(stack[0].url, device=0, num_slots=4, slot_bytes=1 << 20, key=k)
            for k in (KEY, None, KEY[::-1])]
    yield made
    # their pooled connections go before the servers are asked to stop
    made.clear()
    gc.collect()


def stored_object(path: str) -> bytes:
    """An object as modelx-s3d keeps it: one file, or after a multipart upload
    a list "S3DPARTS\\n<size> <name>\\n..." of the files under <path>.parts/."""
    with open(path, "rb") as f:
        data = f.read()
    if not data.startswith(b"S3DPARTS\n"):
        return data
    parts = []
    for line in data.decode().splitlines()[1:]:
        with open(os.path.join(path + ".parts", line.split()[1]), "rb") as f:
            parts.append(f.read())
    return b"".join(parts)


@pytest.mark.parametrize("options", [{}, {"compress": "zstd", "planes": 2}],
                         ids=["plain", "zstd-planes"])
def test_encrypted_push_round_trips(clients, stack, dev, tmp_path, options):
    from modelx_amd.client import Client

    keyed, keyless, other = clients
    src = dev[5:5 + 3 * 65536 + 778]  # four parts, the last one ragged, source unaligned
    plain = DATA[5:5 + src.numel()]
    repo = "aead/" + "-".join(["m"] + sorted(options))
    keyed.last_stats.clear()
    manifest = keyed.push_from_gpu(repo, "v1", {"w.bin": src}, part_bytes=65536, encrypt=True,
                                   **options)
    desc, = [d for d in manifest.blobs if d.name == "w.bin"]
    seg, n, salt = rules.encryption(desc)
    assert seg == S and desc.size == rules.sealed_size(n, seg)

    # the store holds the sealed bytes, which the derived key opens
    root = stack[1].proc.args[stack[1].proc.args.index("--root") + 1]
    stored = stored_object(os.path.join(root, "modelx", "registry",
                                        pm.blob_digest_path(repo, desc.digest)))
    assert len(stored) == desc.size and stored[:n] != plain[:n]
    opened = _core.aead_open_host(rules.blob_key(KEY, salt, seg, n), stored, n, seg)
    assert (opened == plain) == (not options)

    back = keyed.pull_to_gpu(repo, "v1")
    assert torch.equal(back["w.bin"], src)
    phases = {s["phase"]: s for s in keyed.last_stats}
    assert phases["push-seal"]["bytes"] == n and phases["pull-open"]["bytes"] == n
    assert phases["push-seal"]["segments"] == (n + seg - 1) // seg

    for client, code in ((keyless, er.ErrCode.UNSUPPORTED), (other, er.ErrCode.DIGEST_INVALID)):
        with pytest.raises(er.ModelxError) as e:
            client.pull_to_gpu(repo, "v1")
        assert e.value.code == code

    cpu = Client(stack[0].url)
    cpu.pull(repo, "v1", str(tmp_path), quiet=True, key=KEY)
    with open(tmp_path / "w.bin", "rb") as f:
        assert f.read() == plain
    with pytest.raises(er.ModelxError) as e:
        cpu.pull(repo, "v1", str(tmp_path / "nokey"), quiet=True)
    assert e.value.code == er.ErrCode.UNSUPPORTED


@pytest.mark.parametrize("options", [{"cdc": True}, {"dirs": {"d": {}}}, {"encrypt_segment": 1000}],
                         ids=["cdc", "dirs", "segment"])
def test_encrypt_bad_combinations_are_unsupported(clients, dev, options):
    for client in clients[:2]:  # with a key: the combination; without: the missing key
        with pytest.raises(er.ModelxError) as e:
            client.push_from_gpu("aead/bad", "v1", {"w.bin": dev[:64]}, encrypt=True, **options)
        assert e.value.code == er.ErrCode.UNSUPPORTED
