"""The gzip host model (modelx/deflate_core.hpp, ``_core.gzip_compress_host``)
against zlib: every payload and length round-trips, the trailer and the bound
hold, the bytes are deterministic, and the sizes show that matches, Huffman
coding and the stored fallback each took effect. The ``dir_format`` rules."""
import functools
import gzip
import random
import zlib

import pytest

torch = pytest.importorskip("torch")  # before _core (engineering note 16)

from modelx_amd import _core
from modelx_amd.client import gpu_rules as rules
from modelx_amd.wire import errors as er

C = _core.GZIP_CHUNK_BYTES
LENGTHS = [0, 1, 3, 4, 5, 11, 12, 258, 259, 262, 32768, 32769, C - 1, C, C + 1, 2 * C + 1041]
TOTAL = max(LENGTHS) + 16  # room for the GPU test's source offsets


def zeros(seed):
    return bytes(TOTAL)


def rand(seed):
    return random.Random(seed).randbytes(TOTAL)


def words(seed, total=TOTAL):
    r = random.Random(seed)
    vocab = [bytes(r.randrange(97, 123) for _ in range(r.randrange(2, 9))) for _ in range(200)]
    out = bytearray()
    while len(out) < total:
        out += r.choice(vocab) + b" "
    return bytes(out[:total])


def onebyte_runs(seed):
    r = random.Random(seed)
    out = bytearray()
    while len(out) < TOTAL:
        out += bytes([r.randrange(256)]) * r.randrange(1, 601)
    return bytes(out[:TOTAL])


def far(seed):
    """A 300-byte motif again 32768 + k bytes on, k = -1, 0, +1, from starts
    inside a chunk and across a chunk edge, over a four-letter background."""
    r = random.Random(seed)
    out = bytearray(r.choice(b"acgt") for _ in range(TOTAL))
    motif = r.randbytes(300)
    for start, k in ((100, -1), (700, 0), (1300, 1), (C - 150, 0), (C - 600, 1), (C + 2000, -1)):
        out[start:start + 300] = motif
        out[start + 32768 + k:start + 32768 + k + 300] = motif
    return bytes(out[:TOTAL])


PAYLOADS = {"zeros": zeros, "random": rand, "words": words, "onebyte_runs": onebyte_runs,
            "far": far}


@functools.lru_cache(maxsize=None)
def payload(name):
    return PAYLOADS[name](sorted(PAYLOADS).index(name) + 11)


@functools.lru_cache(maxsize=None)
def model(name, offset, n):
    return _core.gzip_compress_host(payload(name)[offset:offset + n])


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_host_model_round_trips(name, n):
    x = payload(name)[:n]
    out = model(name, 0, n)
    assert zlib.decompress(out, 31) == x
    assert out[-8:] == zlib.crc32(x).to_bytes(4, "little") + (n % 2**32).to_bytes(4, "little")
    assert len(out) <= _core.gzip_compress_bound(n)
    assert _core.gzip_compress_host(x) == out
    if name == "zeros" and n >= 4096:
        assert len(out) < n // 16
    if name == "words" and n >= C:
        assert len(out) < n
    if name == "random":
        assert len(out) <= n + (_core.gzip_compress_bound(n) - n)


def test_gzip_module_reads_it():
    assert gzip.decompress(model("words", 0, 2 * C + 1041)) == payload("words")[:2 * C + 1041]


def test_header_is_the_documented_one():
    assert model("zeros", 0, 0)[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])
    assert model("zeros", 0, 0)[10:15] == bytes([1, 0, 0, 0xff, 0xff])  # one final empty block


@pytest.mark.parametrize("dir_format, dirs, cdc", [
    ("tgz", {"d": {}}, None), ("", {"d": {}}, None), ("tar+gz", None, None),
    ("tar+gz", {}, None), ("tar+gz", {"d": {}}, (32768, 16, 262144))])
def test_bad_dir_format_is_unsupported(dir_format, dirs, cdc):
    with pytest.raises(er.ModelxError) as e:
        rules.check_dir_format(dir_format, dirs, cdc)
    assert e.value.code == er.ErrCode.UNSUPPORTED


def test_good_dir_formats_pass():
    rules.check_dir_format("tar", None, None)
    rules.check_dir_format("tar", {"d": {}}, (32768, 16, 262144))
    rules.check_dir_format("tar+gz", {"d": {}}, None)
