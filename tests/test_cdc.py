"""Content-defined chunking on the host: the arithmetic of
core/include/modelx/cdc_core.hpp as exposed through _core, and the CDC
sidecar rules of gpu_rules.py. Runs without a GPU."""
import hashlib

import numpy as np
import pytest

from modelx_amd import _core
from modelx_amd.client import gpu_rules as rules
from modelx_amd.wire import errors as er

PARAMS = (64, 6, 1024)


def _rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def shifted_pair():
    """(A, B): 256 KiB of random bytes, and the same with 37 bytes inserted at
    offset 5000. Shared with tests/test_gpu_cdc.py."""
    a = _rand(20, 256 << 10)
    return a, a[:5000] + _rand(21, 37) + a[5000:]


def test_defaults():
    assert _core.CDC_DEFAULTS == rules.CDC_DEFAULTS == (32 << 10, 16, 256 << 10)
    assert rules.cdc_params(True) == rules.CDC_DEFAULTS and rules.cdc_params(False) is None


@pytest.mark.parametrize("value", range(256))
def test_constant_run_is_never_a_candidate(value):
    buf = bytes([value]) * 96
    for bits in range(1, 21):
        assert [i for i in _core.cdc_candidates_host(buf, bits) if i >= 31] == []


def test_rolling_form_equals_the_closed_form():
    data, bits = _rand(1, 4096), 4
    gear = [_closed_gear(v) for v in range(256)]
    want = []
    for i in range(len(data)):
        h = sum(gear[data[i - k]] << k for k in range(32) if i - k >= 0) & 0xFFFFFFFF
        if h >> (32 - bits) == 0:
            want.append(i)
    assert len(want) > 100 and _core.cdc_candidates_host(data, bits) == want


def _closed_gear(v):
    """cdc_core.hpp's gear(): murmur3's finaliser over a Weyl sequence, >> 1."""
    m = 0xFFFFFFFF
    x = (0x4D58C0DE + v * 0x9E3779B9) & m
    x ^= x >> 16
    x = x * 0x85EBCA6B & m
    x ^= x >> 13
    x = x * 0xC2B2AE35 & m
    return (x ^ (x >> 16)) >> 1


def test_chunks_tile_the_buffer_within_min_and_max():
    data = _rand(2, 300_000)
    lo, bits, hi = PARAMS
    chunks = _core.cdc_chunks_host(data, lo, bits, hi)
    assert [o for o, _ in chunks] == [sum(l for _, l in chunks[:i]) for i in range(len(chunks))]
    assert sum(l for _, l in chunks) == len(data)
    assert all(lo <= l <= hi for _, l in chunks[:-1]) and 0 < chunks[-1][1] <= hi
    cand = set(_core.cdc_candidates_host(data, bits))
    for o, l in chunks[:-1]:  # cut at the first eligible candidate, else at max
        eligible = [i for i in range(o + lo - 1, o + hi) if i in cand]
        assert o + l == (eligible[0] + 1 if eligible else o + hi)


def test_chunks_of_edge_sizes():
    lo, bits, hi = 64, 6, 1024
    zeros = bytes(hi + 1)  # constant data has no candidates: cut by max alone
    assert _core.cdc_chunks_host(b"", lo, bits, hi) == []
    assert _core.cdc_chunks_host(b"x", lo, bits, hi) == [(0, 1)]
    assert _core.cdc_chunks_host(zeros[:lo], lo, bits, hi) == [(0, lo)]
    assert _core.cdc_chunks_host(zeros, lo, bits, hi) == [(0, hi), (hi, 1)]


@pytest.mark.parametrize("params", [(63, 6, 1024), (64, 0, 1024), (64, 25, 1024), (2048, 6, 1024),
                                    (64, 6, (16 << 20) + 1), (64, 6), "on", (64.0, 6, 1024)])
def test_invalid_parameters_are_unsupported(params):
    with pytest.raises(er.ModelxError) as e:
        rules.cdc_params(params)
    assert e.value.code == er.ErrCode.UNSUPPORTED
    if isinstance(params, tuple) and len(params) == 3 and isinstance(params[0], int):
        with pytest.raises(ValueError, match="UNSUPPORTED"):
            _core.cdc_chunks_host(b"abc", *params)


def test_chunks_resynchronise_after_an_insertion():
    a, b = shifted_pair()
    have = {hashlib.sha256(a[o:o + l]).digest() for o, l in _core.cdc_chunks_host(a, *PARAMS)}
    covered = sum(l for o, l in _core.cdc_chunks_host(b, *PARAMS)
                  if hashlib.sha256(b[o:o + l]).digest() in have)
    assert covered >= len(b) // 2


def _sidecar(data, params=PARAMS):
    ranges = _core.cdc_chunks_host(data, *params)
    body = rules.cdc_sidecar(params, ranges,
                             b"".join(hashlib.sha256(data[o:o + l]).digest() for o, l in ranges))
    return body, ranges


def test_sidecar_round_trip():
    data = _rand(3, 10_000)
    body, ranges = _sidecar(data)
    assert body[:8] == b"MXCDC1\0\0" and len(body) == 24 + 36 * len(ranges)
    params, got, digests = rules.cdc_usable(body, "sha256:" + hashlib.sha256(body).hexdigest(),
                                            len(data))
    assert params == PARAMS and got == ranges
    assert digests[:32] == hashlib.sha256(data[:ranges[0][1]]).digest()


def _patched(body, at, value):
    return body[:at] + value + body[at + len(value):]


@pytest.mark.parametrize("damage", [
    lambda b: (b, "sha256:" + "0" * 64, 10_000),                # digest does not match
    lambda b: (_patched(b, 0, b"MXCDC2"), None, 10_000),        # magic
    lambda b: (_patched(b, 8, (32).to_bytes(4, "little")), None, 10_000),   # min < 64
    lambda b: (_patched(b, 16, (25).to_bytes(4, "little")), None, 10_000),  # bits > 24
    lambda b: (_patched(b, 24, (0).to_bytes(4, "little")), None, 10_000),   # a zero length
    lambda b: (_patched(b, 24, (1025).to_bytes(4, "little")), None, 10_000),  # length > max
    lambda b: (b, None, 10_001),                                # lengths do not sum to the size
    lambda b: (b[:-1], None, 10_000),                           # truncated record
], ids=["digest", "magic", "min", "bits", "zero-length", "over-max", "sum", "truncated"])
def test_unusable_sidecar_counts_as_absent(damage):
    body, digest, size = damage(_sidecar(_rand(3, 10_000))[0])
    digest = digest or "sha256:" + hashlib.sha256(body).hexdigest()
    assert rules.cdc_usable(body, digest, size) is None
