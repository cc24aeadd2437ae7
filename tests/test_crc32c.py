"""CRC-32C host arithmetic (core/include/modelx/crc32c_core.hpp) against a
plain bytewise reference written here: the SSE4.2 path, the bytewise model
the kernel is tested against, mul_xn and combine."""
import random

import pytest

from modelx_amd import _core

_TABLE = []
for _b in range(256):
    for _ in range(8):
        _b = (_b >> 1) ^ (0x82F63B78 if _b & 1 else 0)
    _TABLE.append(_b)


def ref_crc32c(data: bytes, state: int = 0xFFFFFFFF, final: int = 0xFFFFFFFF) -> int:
    for x in data:
        state = _TABLE[(state ^ x) & 0xFF] ^ (state >> 8)
    return state ^ final


def seeded(n: int, seed: int = 7) -> bytes:
    return random.Random(seed).randbytes(n)


def test_check_value():
    assert ref_crc32c(b"123456789") == 0xE3069283
    assert _core.crc32c_host(b"123456789") == 0xE3069283
    assert _core.crc32c_host(b"123456789", model=True) == 0xE3069283


@pytest.mark.parametrize("model", [False, True])
@pytest.mark.parametrize("size", [0, 1, 3, 4, 7, 8, 9, (64 << 10) + 1])
def test_host_matches_reference(size, model):
    data = seeded(size)
    assert _core.crc32c_host(data, model=model) == ref_crc32c(data)


@pytest.mark.parametrize("len_a,len_b", [(0, 0), (0, 1), (1, 0), (1, 1), (5, 4099), (4099, 5)])
def test_combine(len_a, len_b):
    a, b = seeded(len_a, 1), seeded(len_b, 2)
    assert _core.crc32c_combine(ref_crc32c(a), ref_crc32c(b), len_b) == ref_crc32c(a + b)


@pytest.mark.parametrize("nbytes", [0, 1, 2, 255, 4099, 1 << 16])
def test_mul_xn_is_zero_bytes(nbytes):
    """A raw register advanced by mul_xn equals the same register fed that
    many zero bytes."""
    reg = 0x1234ABCD
    assert _core.crc32c_mul_xn(reg, nbytes) == ref_crc32c(bytes(nbytes), reg, 0)


def test_lengths_past_32_bits():
    """len(b) >= 2^32 with b all zeros. x^(8 * 2^32) is checked against 2^16
    steps of 2^16 bytes (each of which the test above pins to the
    reference), and combine against mul_xn composed twice."""
    reg = 0x1234ABCD
    step = reg
    for _ in range(1 << 16):
        step = _core.crc32c_mul_xn(step, 1 << 16)
    assert _core.crc32c_mul_xn(reg, 1 << 32) == step
    a = seeded(9, 3)
    len_b = (1 << 32) + 7
    # crc of len_b zero bytes: the initial value advanced, then the final xor
    crc_b = _core.crc32c_mul_xn(_core.crc32c_mul_xn(0xFFFFFFFF, 1 << 32), 7) ^ 0xFFFFFFFF
    want = _core.crc32c_mul_xn(_core.crc32c_mul_xn(ref_crc32c(a), 1 << 32), 7) ^ crc_b
    assert _core.crc32c_combine(ref_crc32c(a), crc_b, len_b) == want
