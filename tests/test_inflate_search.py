"""The host model of the block-search gunzip (modelx/inflate_core.hpp,
``_core.gzip_inflate_spans_host(member, search=True)``) against
``zlib.decompress`` on stock, unflushed streams: Huffman blocks cut at found
dynamic headers, distances of a whole window across the cuts, stored blocks cut
at found LEN fields, both kinds in one stream, a false candidate, members below
one stride, and the ineligible members with the statuses they have without
search. test_gpu_gunzip_search runs the same members through the kernels."""
import functools
import gzip
import random
import zlib

import pytest

torch = pytest.importorskip("torch")  # before _core (engineering note 16)

from modelx_amd import _core

from test_deflate import words
from test_inflate import bad_members, far_words

STRIDE = 64 << 10
KEPT_STATUSES = ["two-members", "flipped", "truncated", "isize", "not-gzip"]


def noise(n):
    return random.Random(7).randbytes(n)


def planted():
    """Random bytes (stored blocks) with the first dynamic block header of the
    words member copied in, byte-aligned, just after the first stride
    boundary: a header that confirms and a block that does not decode."""
    member = gzip.compress(words(6, 1 << 20))
    assert (member[10] >> 1) & 3 == 2  # a dynamic first block
    data = bytearray(noise(200000))
    data[STRIDE + 40:STRIDE + 340] = member[10:310]
    return bytes(data)


@functools.lru_cache(maxsize=None)
def search_members():
    """name -> (member, source) of every member a search makes eligible."""
    w, r = words(6, 1 << 20), noise(300000)
    mix = r[:150000] + words(11, 150000) + r[150000:300000] + words(12, 150000)
    out = {"words-l9": (gzip.compress(w), w), "words-l1": (gzip.compress(w, 1), w),
           "far": (gzip.compress(far_words(400000)), far_words(400000)),
           "random": (gzip.compress(r), r),
           "mix": (gzip.compress(mix), mix),
           "sync-flush": (bad_members()["sync-flush"][0], words(2, 150000)),
           "planted": (gzip.compress(planted()), planted())}
    for n in (0, 1, 40000):
        out["short-%d" % n] = (gzip.compress(w[:n]), w[:n])
    return out


@pytest.mark.parametrize("name", sorted(search_members()))
def test_search_equals_zlib(name):
    member, x = search_members()[name]
    assert zlib.decompress(member, 31) == x
    assert _core.gzip_inflate_spans_host(member, search=True) == ("ok", x)
    plan = _core.gzip_inflate_plan_host(member, search=True)
    assert (plan["status"], plan["out_bytes"]) == ("ok", len(x))
    if len(member) < STRIDE:
        assert plan["spans"] == 1  # the short ones and sync-flush: below one stride
    else:  # a block starts after every stride boundary
        assert plan["spans"] >= (3 if name == "words-l9" else 2)


@pytest.mark.parametrize("name", KEPT_STATUSES)
def test_search_keeps_the_status_of_ineligible_members(name):
    member, status = bad_members()[name]
    assert _core.gzip_inflate_spans_host(member, search=True) == (status, b"")
    assert _core.gzip_inflate_plan_host(member, search=True) == {"status": status, "out_bytes": 0,
                                                                 "spans": 0}
