"""The pinned ring under its new rules: a pulled slot returns when its H2D
copy ends and the blob is hashed by ONE launch after landing; a D2H drain
leases ONE slot and double-buffers between its halves; every ring user takes
one slot at a time, so an oversubscribed ring stays live.

All shapes are small (1 MiB slots, 2 of them): the geometry under test is in
the boundaries (chunk, half slot, slot, super-range of 4 slots), not in the
byte count."""
import hashlib
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CS = 128 << 10  # chunk size
SLOT = 1 << 20
HALF = SLOT // 2
HOST = np.random.default_rng(20240607).integers(0, 256, 20 << 20, dtype=np.uint8).tobytes()


def chunk_leaves(data: bytes, cs: int) -> bytes:
    """Per-chunk sha256 of data; the one leaf of the empty string for b""."""
    return b"".join(hashlib.sha256(data[off:off + cs]).digest()
                    for off in range(0, max(len(data), 1), cs))


@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    from util_servers import start_modelxd_s3, start_s3d

    root = tmp_path_factory.mktemp("ring")
    s3d = start_s3d(str(root / "s3"))
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    yield mdx
    mdx.stop()
    s3d.stop()


@pytest.fixture(scope="module")
def dev():
    t = torch.frombuffer(bytearray(HOST), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def client(stack):
    from modelx_amd.client.gpu import GpuClient

    return GpuClient(stack.url, device=0, num_slots=2, slot_bytes=SLOT, num_conns=8)


def _push(g, repo, version, src, **kw):
    m = g.push_from_gpu(repo, version, {"w.bin": src}, **kw)
    (desc,) = [b for b in m.blobs if b.name == "w.bin"]
    return desc


def _hashed_pull(g, repo, desc, cs):
    """engine.pull_to_device_hashed of a pushed blob -> (stats, leaves, bytes)."""
    url, headers = g._download_url(repo, desc)
    dst = torch.zeros(max(desc.size, 1), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    stats, leaves = g.engine.pull_to_device_hashed(url, headers, desc.size, dst.data_ptr(),
                                                   g.num_conns, cs)
    return stats, leaves, dst[:desc.size].cpu().numpy().tobytes()


# ------------------------------------------------------ hashed pull geometry --

HASHED_SIZES = [1, CS - 1, CS, CS + 1, SLOT - 1, SLOT, SLOT + 1, 4 * SLOT, 4 * SLOT + 17]


@pytest.mark.parametrize("n", HASHED_SIZES)
def test_hashed_pull_geometry(client, dev, n):
    repo = f"ring/hashed{n}"
    desc = _push(client, repo, "v1", dev[:n], chunk_size=CS)
    back = client.pull_to_gpu(repo, "v1")
    assert back["w.bin"].cpu().numpy().tobytes() == HOST[:n]
    hashed = [s for s in client.last_stats if s.get("phase") == "pull-transfer-hashed"]
    assert hashed and hashed[-1]["bytes"] == n, "the pull did not take the hashed path"
    stats, leaves, got = _hashed_pull(client, repo, desc, CS)
    assert got == HOST[:n]
    assert leaves == chunk_leaves(HOST[:n], CS)
    assert stats["slot_wait_seconds"] >= 0


def test_hashed_pull_slot_equals_chunk(stack, dev):
    from modelx_amd.client.gpu import GpuClient

    g = GpuClient(stack.url, device=0, num_slots=2, slot_bytes=CS, num_conns=8)
    n = 9 * CS + 3  # three super-ranges of 4 one-chunk slots, ragged end
    desc = _push(g, "ring/slot-is-chunk", "v1", dev[7:7 + n], chunk_size=CS)
    back = g.pull_to_gpu("ring/slot-is-chunk", "v1")
    assert back["w.bin"].cpu().numpy().tobytes() == HOST[7:7 + n]
    _, leaves, got = _hashed_pull(g, "ring/slot-is-chunk", desc, CS)
    assert got == HOST[7:7 + n]
    assert leaves == chunk_leaves(HOST[7:7 + n], CS)


def test_hashed_pull_of_nothing_is_the_empty_leaf(client, dev):
    # no byte is fetched for size 0; the URL only has to parse
    desc = _push(client, "ring/empty", "v1", dev[:CS], chunk_size=CS)
    url, headers = client._download_url("ring/empty", desc)
    dst = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    stats, leaves = client.engine.pull_to_device_hashed(url, headers, 0, dst.data_ptr(), 8, CS)
    assert leaves == hashlib.sha256(b"").digest()
    assert stats["bytes"] == 0 and stats["slot_wait_seconds"] >= 0


def test_hashed_pull_keeps_its_slot_multiple_check(client, dev):
    with pytest.raises(RuntimeError, match="multiple of chunk_size"):
        client.engine.pull_to_device_hashed("http://127.0.0.1:1/x", {}, 16, dev.data_ptr(), 1,
                                            CS - 1)


# --------------------------------------------------------- drain boundaries --

DRAIN_SIZES = [1, HALF - 1, HALF, HALF + 1, SLOT - 1, SLOT, SLOT + 1, 3 * HALF + 5]


@pytest.mark.parametrize("n", DRAIN_SIZES)
def test_drain_boundaries_push(client, dev, n):
    # one part, so one drain carries the whole blob; the source is off the
    # 16 B grid
    src = dev[3:3 + n]
    _push(client, f"ring/drain{n}", "v1", src, part_bytes=4 * SLOT)
    back = client.pull_to_gpu(f"ring/drain{n}", "v1")
    assert back["w.bin"].cpu().numpy().tobytes() == HOST[3:3 + n]


@pytest.mark.parametrize("n", DRAIN_SIZES)
def test_drain_boundaries_canonical(client, dev, n):
    got = client.engine.sha256_canonical_device(dev.data_ptr() + 3, n)
    assert got == hashlib.sha256(HOST[3:3 + n]).digest()


@pytest.mark.parametrize("slot_bytes", [4096, 8192, 13288],
                         ids=["single-buffered", "smallest-halves", "ragged-halves"])
def test_drain_small_slots(stack, dev, slot_bytes):
    """4096: below 8 KiB the whole slot is one buffer. 8192: the smallest
    slot with halves. 13288: the second half starts at 4096 (half rounded
    down to 4 KiB) and the bytes behind 8192 stay unused."""
    from modelx_amd.client.gpu import GpuClient

    g = GpuClient(stack.url, device=0, num_slots=2, slot_bytes=slot_bytes, num_conns=4)
    half = slot_bytes if slot_bytes < 8192 else (slot_bytes // 2) & ~4095
    for n in [1, half - 1, half, half + 1, 2 * half, 2 * half + 1, 3 * half + 5]:
        got = g.engine.sha256_canonical_device(dev.data_ptr() + 1, n)
        assert got == hashlib.sha256(HOST[1:1 + n]).digest(), n
    n = 5 * half + 5
    _push(g, f"ring/small{slot_bytes}", "v1", dev[1:1 + n])
    back = g.pull_to_gpu(f"ring/small{slot_bytes}", "v1")
    assert back["w.bin"].cpu().numpy().tobytes() == HOST[1:1 + n]


# ------------------------------------------------ oversubscribed ring stays live --

def test_oversubscribed_ring_stays_live(client, dev):
    """6 pushes (6 part uploads each) and 3 pulls (8 connections each) on a
    ring of 2 slots: 60 takers at the most. Every one of them needs ONE slot
    and gives it back after a bounded piece of work, so all of them finish;
    a taker that needs two free slots at once would wait behind the rest."""
    blob = 8 * SLOT
    errors = []
    pulled = {}

    def src_of(i):
        return dev[i * SLOT + i: i * SLOT + i + blob]

    def ref_of(i):
        return HOST[i * SLOT + i: i * SLOT + i + blob]

    for i in range(3):
        _push(client, "ring/live", f"old{i}", src_of(i), part_bytes=SLOT)

    def push(i):
        try:
            _push(client, "ring/live", f"new{i}", src_of(i), part_bytes=SLOT)
        except Exception as e:  # surfaced by the assertion below
            errors.append(("push", i, repr(e)))

    def pull(i):
        try:
            pulled[f"old{i}"] = client.pull_to_gpu("ring/live", f"old{i}")["w.bin"]
        except Exception as e:
            errors.append(("pull", i, repr(e)))

    threads = [threading.Thread(target=push, args=(i,), daemon=True) for i in range(3, 9)]
    threads += [threading.Thread(target=pull, args=(i,), daemon=True) for i in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not [t.name for t in threads if t.is_alive()], "a ring user never got its slot"
    assert not errors, errors
    for i in range(3):
        assert pulled[f"old{i}"].cpu().numpy().tobytes() == ref_of(i), i
    for i in range(3, 9):
        back = client.pull_to_gpu("ring/live", f"new{i}")["w.bin"]
        assert back.cpu().numpy().tobytes() == ref_of(i), i


# -------------------------------------------------------------------- stats --

def test_stats_carry_slot_wait(client, dev):
    from modelx_amd.client.gpu import _signed_headers
    from modelx_amd.wire import digest as dg
    from modelx_amd.wire import types

    n = SLOT + 5
    desc = types.Descriptor(name="p.bin", media_type=types.MEDIA_TYPE_MODEL_FILE,
                            digest=dg.sha256_digest(HOST[:n]), size=n)
    part = client.remote.get_blob_location("ring/stats", desc, "upload").properties["parts"][0]
    pushed = client.engine.push_part_from_device(part["url"], part.get("method") or "PUT",
                                                 _signed_headers(part), dev.data_ptr(), n)
    assert pushed["bytes"] == n and pushed["slot_wait_seconds"] >= 0

    desc = _push(client, "ring/stats2", "v1", dev[:n], chunk_size=CS)
    url, headers = client._download_url("ring/stats2", desc)
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    plain = client.engine.pull_to_device(url, headers, n, dst.data_ptr(), 8)
    assert plain["bytes"] == n and plain["slot_wait_seconds"] >= 0
    assert dst.cpu().numpy().tobytes() == HOST[:n]
