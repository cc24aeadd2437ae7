"""The span-parallel inflate host model (modelx/inflate_core.hpp,
``_core.gzip_inflate_spans_host``) against zlib and the source bytes: members
of this project's own format, foreign streams flushed with ``Z_FULL_FLUSH``
(fixed blocks, code length symbols 16 to 18, distances up to 32768, spans above
64 KiB, a last block that ends inside a byte, a header with FEXTRA and FNAME),
a false marker inside stored data, and every kind of ineligible member with
its status. test_gpu_gunzip runs the same members through the kernels."""
import functools
import gzip
import random
import struct
import zlib

import pytest

torch = pytest.importorskip("torch")  # before _core (engineering note 16)

from modelx_amd import _core

from test_deflate import C, PAYLOADS, payload, words

OWN_LENGTHS = [0, 1, 258, C - 1, C, C + 1, 2 * C + 1041]


def flushed(data, level, every, mode=zlib.Z_FULL_FLUSH):
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    out = b"".join(co.compress(data[i:i + every]) + co.flush(mode)
                   for i in range(0, len(data), every))
    return out + co.flush()


def rewrap(member, header):
    """The same deflate bytes and trailer behind another gzip header."""
    return header + member[10:]


EXTRA_NAME = (b"\x1f\x8b\x08\x0c" + bytes(6) + struct.pack("<H", 6) + b"\x00\x00\xff\xff\x00\x01" +
              b"a name\x00")


def runs(total):
    r = random.Random(5)
    out = bytearray()
    while len(out) < total:
        out += bytes([r.randrange(4)]) * r.randrange(1, 900)
    return bytes(out[:total])


def far_words(total):
    """Words whose second half repeats the first 32768 bytes on: distances up
    to the window."""
    w = words(21, total)
    return w[:32768] + w[:total - 32768]


def false_marker():
    data = bytearray(payload("random")[:2 * C] + words(3, C))
    data[5000:5004] = data[C + 7:C + 11] = b"\x00\x00\xff\xff"
    return bytes(data)


@functools.lru_cache(maxsize=None)
def good_members():
    """name -> (member, source) of every eligible member the GPU test shares."""
    out = {}
    for every in (1000, 40000, 70000):
        for name, data in (("words", words(2, 150000)), ("runs", runs(150000))):
            for level in (1, 9):
                out["full-%s-%d-l%d" % (name, every, level)] = (flushed(data, level, every), data)
    out["full-far"] = (flushed(far_words(100000), 9, 70000), far_words(100000))
    out["header"] = (rewrap(flushed(words(4, 5000), 6, 1000), EXTRA_NAME), words(4, 5000))
    out["false-marker"] = (_core.gzip_compress_host(false_marker()), false_marker())
    return out


@functools.lru_cache(maxsize=None)
def bad_members():
    """name -> (member, status)."""
    data = words(2, 150000)
    own = _core.gzip_compress_host(payload("words")[:2 * C + 1041])
    flipped = bytearray(own)
    flipped[12] ^= 0xFF  # inside the first block's code lengths
    crc_only = bytearray(_core.gzip_compress_host(payload("random")[:1000]))
    crc_only[500] ^= 1  # a stored byte: only the CRC-32 can tell
    return {"sync-flush": (flushed(data, 6, 40000, zlib.Z_SYNC_FLUSH), "dependent"),
            "stock": (gzip.compress(words(6, 1 << 20)), "too-long"),
            "two-members": (own + own, "trailing"),
            "flipped": (bytes(flipped), "corrupt"),
            "flipped-stored": (bytes(crc_only), "corrupt"),
            "isize": (own[:-4] + struct.pack("<I", 2 * C + 1040), "corrupt"),
            "truncated": (own[:len(own) // 2], "corrupt"),
            "no-header": (own[:12], "header"),
            "not-gzip": (b"PK" + own[2:], "header")}


@pytest.mark.parametrize("n", OWN_LENGTHS)
@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_own_format(name, n):
    x = payload(name)[:n]
    member = _core.gzip_compress_host(x)
    assert _core.gzip_inflate_spans_host(member) == ("ok", x)
    plan = _core.gzip_inflate_plan_host(member)
    assert plan["out_bytes"] == n
    assert plan["spans"] == max(1, -(-n // C)) or name == "random"  # stored chunks share a span


@pytest.mark.parametrize("name", sorted(good_members()))
def test_foreign_and_marked_members(name):
    member, x = good_members()[name]
    assert zlib.decompress(member, 31) == x
    assert _core.gzip_inflate_spans_host(member) == ("ok", x)


def test_the_foreign_members_reach_their_edges():
    """What the list above is there for, read off the streams themselves."""
    members = good_members()
    first_types = {(m[0][10] >> 1) & 3 for name, m in members.items() if name.startswith("full-")}
    assert first_types == {1, 2}  # fixed and dynamic first blocks
    assert _core.gzip_inflate_plan_host(members["full-words-70000-l9"][0])["spans"] == 4  # 3 flushes, the end
    assert _core.gzip_inflate_plan_host(members["full-words-1000-l1"][0])["spans"] == 151
    assert _core.gzip_inflate_plan_host(members["header"][0])["spans"] == 6  # 5 flushes, the end
    # a final block that ends inside a byte: zlib's last flush() is no sync marker
    assert members["full-runs-40000-l9"][0][-12:-8] != b"\x00\x00\xff\xff"


@pytest.mark.parametrize("name", sorted(bad_members()))
def test_ineligible_members(name):
    member, status = bad_members()[name]
    assert _core.gzip_inflate_spans_host(member) == (status, b"")
    assert _core.gzip_inflate_plan_host(member) == {"status": status, "out_bytes": 0, "spans": 0}
