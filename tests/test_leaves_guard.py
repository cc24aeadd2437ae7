"""Host-side guard between remote leaves / chunk-size annotations and the
device engine (modelx_amd.client.gpu.leaves_usable). Pure Python: no GPU."""
import hashlib
import itertools

import pytest

from modelx_amd.client import gpu
from modelx_amd.wire import digest as dg
from modelx_amd.wire import types


def _leaves(n):
    return b"".join(hashlib.sha256(bytes([i % 256, i // 256])).digest() for i in range(n))


@pytest.mark.parametrize("size,cs,n", [
    (1, 4096, 1), (4095, 4096, 1), (4096, 4096, 1), (4097, 4096, 2),
    (10 * 4096, 4096, 10), (10 * 4096 + 1, 4096, 11), (39 * 17 + 3, 17, 40),
    (5, 1, 5), (1 << 40, 1 << 20, 1 << 20),
])
def test_exact_short_and_long_leaves(size, cs, n):
    if n > 4096:  # count only: do not build a 32 MiB array
        assert (size - 1) // cs + 1 == n
        return
    assert gpu.leaves_usable(_leaves(n), size, cs)
    assert not gpu.leaves_usable(_leaves(n + 1), size, cs)
    assert not gpu.leaves_usable(_leaves(n - 1), size, cs)
    assert not gpu.leaves_usable(_leaves(n) + b"\0", size, cs)
    assert not gpu.leaves_usable(_leaves(n)[:-1], size, cs)


def test_empty_blob_has_one_leaf():
    assert gpu.leaves_usable(_leaves(1), 0, 4096)
    assert gpu.leaves_usable(bytearray(_leaves(1)), 0, 1)
    assert not gpu.leaves_usable(b"", 0, 4096)
    assert not gpu.leaves_usable(_leaves(2), 0, 4096)


def test_agrees_with_the_digest_reference():
    for size, cs in itertools.product([0, 1, 63, 64, 65, 1000, 4097], [1, 7, 64, 1000]):
        lv = b"".join(dg.chunk_leaves(bytes(size), cs))
        assert gpu.leaves_usable(lv, size, cs), (size, cs)
        assert not gpu.leaves_usable(lv + lv[:32], size, cs), (size, cs)


@pytest.mark.parametrize("cs", [0, -1, -4096, 4096.0, 0.5, "4096", None, True, b"1"])
def test_bad_chunk_sizes(cs):
    assert not gpu.leaves_usable(_leaves(1), 100, cs)
    assert not gpu.leaves_usable(_leaves(1), 0, cs)


def test_bad_leaves_and_sizes():
    assert not gpu.leaves_usable(None, 100, 4096)
    assert not gpu.leaves_usable("x" * 32, 100, 4096)
    assert not gpu.leaves_usable(_leaves(1), -1, 4096)
    assert not gpu.leaves_usable(_leaves(1), 1.0, 4096)


@pytest.mark.parametrize("note,want", [
    ("131072", 131072), ("1", 1), (4096, 4096),
    ("", 0), ("0", 0), ("-4096", 0), ("4096.0", 0), ("1e6", 0), ("4k", 0),
    (" 4096", 0), ("0x1000", 0), ("١٢", 0), (0, 0), (-5, 0), (4096.0, 0), (True, 0),
    (None, 0),
])
def test_chunk_size_annotation(note, want):
    """Anything but a positive integer falls back like an absent annotation."""
    d = types.Descriptor(name="w", digest="sha256:" + "0" * 64, size=10)
    if note is not None:
        d.annotations[types.ANNOTATION_CHUNK_SIZE] = note
    assert gpu._annotated_chunk_size(d) == want


class _Tensor:
    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n

    def element_size(self):
        return 1

    def data_ptr(self):
        return 0x1000


class _Engine:
    """Records which engine entry points a pull reaches."""

    def __init__(self, leaves):
        self.calls = []
        self.leaves = leaves

    def sha256_chunk_leaves(self, ptr, size, cs):
        self.calls.append(("sha256_chunk_leaves", size, cs))
        return self.leaves

    def dedup_pull(self, expect, ptr, cs, size):
        self.calls.append(("dedup_pull", len(expect), cs, size))
        return [], size

    def dedup_register(self, leaves, ptr, cs, size):
        self.calls.append(("dedup_register", len(leaves), cs, size))
        return 0

    def pull_to_device(self, url, headers, size, ptr, conns):
        self.calls.append(("pull_to_device", size))
        return {"seconds": 1.0, "bytes": size}


class _Remote:
    def __init__(self, sidecar):
        self.sidecar = sidecar

    def get_blob_location(self, repository, desc, purpose, extra=None):
        return types.BlobLocation(provider="s3", purpose=purpose,
                                  properties={"parts": [{"url": "http://store/blob"}]})

    def get_blob_content(self, repository, digest):
        yield self.sidecar


def _client(sidecar, engine_leaves):
    c = object.__new__(gpu.GpuClient)  # no device: the engine is the stub above
    c.remote, c.engine = _Remote(sidecar), _Engine(engine_leaves)
    c.device, c.num_conns, c.slot_bytes = 0, 1, 1 << 20
    c.last_stats, c.dedup, c._dedup_tensors, c._dedup_registered = [], True, [], True
    return c


def _desc(size, sidecar, chunk_note):
    return types.Descriptor(
        name="w.bin", digest="sha256:" + "0" * 64, size=size,
        annotations={types.ANNOTATION_CHUNK_SIZE: chunk_note,
                     types.ANNOTATION_LEAVES_BLOB: dg.sha256_digest(sidecar)})


def test_pull_with_fitting_sidecar_uses_it():
    size, cs = 10 * 4096 + 5, 4096
    sidecar = _leaves(11)
    c = _client(sidecar, sidecar)
    c.pull_blob_to_device("r", _desc(size, sidecar, str(cs)), tensor=_Tensor(size),
                          verify=False, resume=True)
    assert c.engine.calls == [("sha256_chunk_leaves", size, cs)]
    c = _client(sidecar, sidecar)
    c.pull_blob_to_device("r", _desc(size, sidecar, str(cs)), tensor=_Tensor(size),
                          verify=False)
    assert c.engine.calls == [("dedup_pull", 11 * 32, cs, size),
                              ("dedup_register", 11 * 32, cs, size)]


@pytest.mark.parametrize("nleaves,chunk_note", [
    (12, "4096"), (10, "4096"), (40, "4096"), (0, "4096"),  # sidecar of the wrong length
    (11, "2048"), (11, "8192"),  # chunk size that does not go with the sidecar
])
@pytest.mark.parametrize("resume", [True, False])
def test_pull_with_unusable_sidecar_is_a_full_fetch(nleaves, chunk_note, resume):
    """The sidecar passes its own digest check and still does not describe
    the blob: it never reaches the engine, the blob is fetched whole."""
    size = 10 * 4096 + 5
    sidecar = _leaves(nleaves) or b"\0"
    c = _client(sidecar, _leaves(11))
    c.pull_blob_to_device("r", _desc(size, sidecar, chunk_note), tensor=_Tensor(size),
                          verify=False, resume=resume)
    assert c.engine.calls == [("pull_to_device", size)]


@pytest.mark.parametrize("chunk_note", ["0", "-4096", "4096.5", "abc", ""])
def test_pull_with_bad_chunk_size_annotation_falls_back(chunk_note):
    """As with no annotation: the default chunk size, which this sidecar
    does not fit, so the blob is fetched whole and nothing raises."""
    size = 10 * 4096 + 5
    sidecar = _leaves(11)
    c = _client(sidecar, sidecar)
    c.pull_blob_to_device("r", _desc(size, sidecar, chunk_note), tensor=_Tensor(size),
                          verify=False, resume=True)
    assert c.engine.calls == [("pull_to_device", size)]


def test_register_chunks_refuses_leaves_that_do_not_fit():
    c = _client(b"", b"")
    t = _Tensor(3 * 4096)
    c.register_chunks(t, _leaves(4), 4096)  # one leaf too many
    c.register_chunks(t, _leaves(2), 4096)  # one too few
    c.register_chunks(t, _leaves(3), 0)
    c.register_chunks(t, _leaves(4), 4096, size=4 * 4096)  # blob larger than the tensor
    assert c.engine.calls == [] and c._dedup_tensors == []
    c.register_chunks(t, _leaves(3), 4096)
    c.register_chunks(t, _leaves(2), 4096, size=4096 + 1)  # blob shorter than the tensor
    assert c.engine.calls == [("dedup_register", 96, 4096, 3 * 4096),
                              ("dedup_register", 64, 4096, 4097)]


def _inside(ranges, size):
    end = 0
    for off, ln in ranges:
        assert ln > 0 and off >= end and off + ln <= size, (ranges, size)
        end = off + ln


def test_bad_chunk_ranges_stay_inside_the_blob():
    ranges = gpu.GpuClient._bad_chunk_ranges
    cs, size = 100, 950  # 10 chunks, 50-byte tail
    good = _leaves(10)
    flipped = bytearray(good)
    for i in (0, 4, 5, 9):
        flipped[i * 32] ^= 1
    assert ranges(good, good, cs, size) == []
    assert ranges(bytes(flipped), good, cs, size) == [(0, 100), (400, 200), (900, 50)]
    # leaves that do not fit the blob locate nothing: all of it is bad, and
    # no range leaves [0, size)
    for expect in (_leaves(11), _leaves(9), _leaves(40), good + b"\0", b""):
        for got in (good, expect):
            r = ranges(got, expect, cs, size)
            assert r == [(0, size)]
            _inside(r, size)
    for bad_cs in (0, -100, 100.0, None):
        r = ranges(good, good, bad_cs, size)
        assert r == [(0, size)]
    assert ranges(_leaves(9), good, cs, size) == [(0, size)]
    # every subset of mismatching chunks, a chunk size that does not divide
    for mask in range(1 << 5):
        size, cs = 4 * 7 + 3, 7
        expect = _leaves(5)
        got = bytearray(expect)
        for i in range(5):
            if mask >> i & 1:
                got[i * 32 + 31] ^= 0x80
        r = ranges(bytes(got), expect, cs, size)
        _inside(r, size)
        assert sum(ln for _, ln in r) == sum(
            min(cs, size - i * cs) for i in range(5) if mask >> i & 1)
    # an empty blob has no bytes to refetch, whatever the leaves say
    assert ranges(_leaves(1), _leaves(1), cs, 0) == []
    assert ranges(_leaves(1), _leaves(2), cs, 0) == []
