"""ChaCha20-Poly1305 sealed blobs: the host model
(core/include/modelx/aead_core.hpp, ``_core.aead_seal_host`` /
``aead_open_host``) against a plain reference written here (numpy keystream
over all blocks at once, Poly1305 in Python integers), which is pinned to
RFC 8439 section 2.8.2; and the annotation rules."""
import random
import struct

import numpy as np
import pytest

# torch before _core: this module sorts first, and the process must hold one
# HIP runtime for the GPU tests that follow (docs/engineering-notes.md, 16)
torch = pytest.importorskip("torch")

from modelx_amd import _core
from modelx_amd.client import gpu_rules as rules
from modelx_amd.wire import errors as er
from modelx_amd.wire import types

S = _core.AEAD_DEFAULT_SEGMENT_BYTES
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, S - 1, S, S + 1, 3 * S + 1041]
KEY = bytes(range(0x30, 0x50))


def seeded(n: int, seed: int = 11) -> bytes:
    return random.Random(seed).randbytes(n)


DATA = seeded(3 * S + 1041 + 16)


def _keystream(key: bytes, counters, nonces) -> bytes:
    """ChaCha20 blocks, all at once: block i has counter ``counters[i]`` and
    the nonce words ``nonces[:, i]``."""
    nblocks = len(counters)
    x = np.empty((16, nblocks), dtype=np.uint32)
    x[:4] = np.array(struct.unpack("<4I", b"expand 32-byte k"), dtype=np.uint32)[:, None]
    x[4:12] = np.array(struct.unpack("<8I", key), dtype=np.uint32)[:, None]
    x[12] = counters
    x[13:] = nonces
    init = x.copy()

    def qr(a, b, c, d):
        for p, q, r, n in ((a, b, d, 16), (c, d, b, 12), (a, b, d, 8), (c, d, b, 7)):
            x[p] += x[q]
            x[r] ^= x[p]
            x[r] = (x[r] << np.uint32(n)) | (x[r] >> np.uint32(32 - n))

    for _ in range(10):
        for quad in ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
                     (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14)):
            qr(*quad)
    return (x + init).T.astype("<u4").tobytes()


def _poly1305(key: bytes, msg: bytes) -> bytes:
    r = int.from_bytes(key[:16], "little") & 0x0ffffffc0ffffffc0ffffffc0fffffff
    s = int.from_bytes(key[16:], "little")
    h = 0
    for i in range(0, len(msg), 16):
        block = msg[i:i + 16]
        h = (h + int.from_bytes(block, "little") + (1 << (8 * len(block)))) * r % ((1 << 130) - 5)
    return ((h + s) % (1 << 128)).to_bytes(16, "little")


def _blocks(n: int) -> int:
    return 1 + (n + 63) // 64  # block 0 is the Poly1305 key


def _aead(ks: bytes, plain: bytes, aad: bytes = b""):
    """RFC 8439 section 2.8 from the keystream blocks 0.. of one nonce:
    (ciphertext, tag)."""
    ct = (np.frombuffer(plain, np.uint8)
          ^ np.frombuffer(ks, np.uint8)[64:64 + len(plain)]).tobytes()
    pad = lambda b: b + bytes(-len(b) % 16)  # noqa: E731
    return ct, _poly1305(ks[:32], pad(aad) + pad(ct) + struct.pack("<QQ", len(aad), len(ct)))


def ref_aead(key: bytes, nonce: bytes, plain: bytes, aad: bytes = b""):
    nb = _blocks(len(plain))
    words = np.array(struct.unpack("<3I", nonce), dtype=np.uint32)[:, None]
    return _aead(_keystream(key, np.arange(nb, dtype=np.uint32), np.repeat(words, nb, 1)),
                 plain, aad)


def ref_seal(blob_key: bytes, data: bytes, seg: int) -> bytes:
    """The stored layout: segment i sealed under the nonce LE32(last) +
    LE64(i) with empty AAD, ciphertext at the plaintext's offsets, then one
    tag per segment. The keystream of all segments is one numpy pass."""
    nseg = (len(data) + seg - 1) // seg
    pieces = [data[i * seg:(i + 1) * seg] for i in range(nseg)]
    nb = np.array([_blocks(len(p)) for p in pieces])
    index = np.repeat(np.arange(nseg, dtype=np.uint64), nb)
    ends = np.cumsum(nb)
    counters = np.arange(ends[-1]) - np.repeat(ends - nb, nb)
    nonces = np.stack([index == nseg - 1, index & 0xFFFFFFFF, index >> 32]).astype(np.uint32)
    ks = _keystream(blob_key, counters.astype(np.uint32), nonces)
    sealed = [_aead(ks[64 * (e - b):64 * e], p) for p, b, e in zip(pieces, nb, ends)]
    return b"".join([ct for ct, _ in sealed] + [tag for _, tag in sealed])


def test_reference_is_rfc8439():
    key = bytes(range(0x80, 0xa0))
    nonce = bytes.fromhex("070000004041424344454647")
    text = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip "
            b"for the future, sunscreen would be it.")
    assert len(text) == 114
    ct, tag = ref_aead(key, nonce, text, bytes.fromhex("50515253c0c1c2c3c4c5c6c7"))
    assert ct[:16].hex() == "d31a8d34648e60db7b86afbc53ef7ec2"
    assert tag.hex() == "1ae10b594f09e26a7e902ecbd0600691"
    assert ref_aead(key, nonce, text)[1].hex() == "6a23a4681fd59456aea1d29f82477216"


@pytest.mark.parametrize("seg", [S, 2048])
@pytest.mark.parametrize("n", LENGTHS)
def test_host_seal_matches_reference_and_opens(n, seg):
    sealed = _core.aead_seal_host(KEY, DATA[:n], seg)
    assert len(sealed) == rules.sealed_size(n, seg)
    assert sealed == ref_seal(KEY, DATA[:n], seg)
    assert _core.aead_open_host(KEY, sealed, n, seg) == DATA[:n]


@pytest.mark.parametrize("where", ["ciphertext", "tag", "n"])
@pytest.mark.parametrize("n", [1, 2048, 2049, 5000])
def test_host_open_refuses_one_flipped_bit(n, where):
    sealed = bytearray(ref_seal(KEY, DATA[:n], 2048))
    if where == "ciphertext":
        sealed[n // 2] ^= 0x04
    elif where == "tag":
        sealed[-7] ^= 0x80
    with pytest.raises((ValueError, RuntimeError)):
        _core.aead_open_host(KEY, bytes(sealed), n ^ (where == "n"), 2048)


def test_blob_key_binds_salt_segment_and_length():
    salt = bytes(16)
    keys = {rules.blob_key(KEY, salt, 2048, 100), rules.blob_key(KEY, b"\1" + salt[1:], 2048, 100),
            rules.blob_key(KEY, salt, 4096, 100), rules.blob_key(KEY, salt, 2048, 101),
            rules.blob_key(KEY[::-1], salt, 2048, 100)}
    assert len(keys) == 5 and all(len(k) == 32 for k in keys)


SALT = "00112233445566778899aabbccddeeff"


def _desc(note, size):
    return types.Descriptor(name="w", size=size, annotations={types.ANNOTATION_ENCRYPTION: note})


def test_annotation_round_trips():
    note = rules.encryption_note(2048, 5000, bytes.fromhex(SALT))[types.ANNOTATION_ENCRYPTION]
    assert note == f"chacha20-poly1305;seg=2048;size=5000;salt={SALT}"
    assert rules.sealed_size(5000, 2048) == 5000 + 16 * 3
    assert rules.encryption(_desc(note, 5048)) == (2048, 5000, bytes.fromhex(SALT))
    assert rules.encryption(types.Descriptor(name="w", size=5)) is None


@pytest.mark.parametrize("note,size", [
    (f"chacha20-poly1305;seg=2048;size=5000;salt={SALT}", 5047),  # not the sealed size
    (f"chacha20-poly1305;seg=2048;size=5000;salt={SALT}", 5032),  # a tag short
    (f"aes-256-gcm;seg=2048;size=5000;salt={SALT}", 5048),
    (f"chacha20-poly1305;seg=1000;size=5000;salt={SALT}", 5080),
    (f"chacha20-poly1305;seg=512;size=5000;salt={SALT}", 5160),
    (f"chacha20-poly1305;seg={32 << 20};size=5000;salt={SALT}", 5016),
    (f"chacha20-poly1305;seg=2048;size=0;salt={SALT}", 0),
    (f"chacha20-poly1305;seg=2048;size=5000;salt={SALT[:-2]}", 5048),
    (f"chacha20-poly1305;seg=2048;size=5000;salt={SALT.upper()}", 5048),
    (f"chacha20-poly1305;size=5000;seg=2048;salt={SALT}", 5048),
    (f"chacha20-poly1305;seg=2048;size=5000;salt={SALT};x=1", 5048),
    ("chacha20-poly1305", 5048),
    (7, 5048),
])
def test_malformed_annotation_is_unsupported(note, size):
    with pytest.raises(er.ModelxError) as e:
        rules.encryption(_desc(note, size))
    assert e.value.code == er.ErrCode.UNSUPPORTED


def test_key_and_segment_options():
    rules.check_encrypt_key(None)
    rules.check_encrypt_key(KEY)
    assert rules.encrypt_segment(None) == S and rules.encrypt_segment(4096) == 4096
    for bad in (lambda: rules.check_encrypt_key(KEY[:31]), lambda: rules.check_encrypt_key("k" * 32),
                lambda: rules.encrypt_segment(1000), lambda: rules.encrypt_segment(True),
                lambda: rules.opening_key(_desc(f"chacha20-poly1305;seg=2048;size=5000;salt={SALT}",
                                                5048), None)):
        with pytest.raises(er.ModelxError) as e:
            bad()
        assert e.value.code == er.ErrCode.UNSUPPORTED
