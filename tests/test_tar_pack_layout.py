"""Host-side tar writer layout (core/include/modelx/tar_host.hpp) through
``_core.tar_pack_layout``: the header bytes and offsets the GPU pack kernel
fills in. No GPU needed — Python's ``tarfile`` is the independent reader (it
verifies every header checksum), and a stand-alone C++ self-test runs the
same builder under ASan/UBSan.
"""
import io
import os
import shutil
import subprocess
import tarfile

import pytest

_core = pytest.importorskip("modelx_amd._core")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pad(n: int) -> int:
    return (n + 511) & ~511


def assemble(members, payloads):
    """Archive bytes from the layout's headers + the given payloads."""
    lay = _core.tar_pack_layout([(n, len(payloads[n])) for n in members])
    out = bytearray()
    hoff = 0
    for name, e in zip(members, lay["entries"]):
        assert e["header_off"] == len(out)
        out += lay["headers"][hoff:hoff + e["header_len"]]
        hoff += e["header_len"]
        assert e["payload_off"] == len(out)
        assert e["size"] == len(payloads[name])
        out += payloads[name]
        out += bytes(_pad(e["size"]) - e["size"])
    assert hoff == len(lay["headers"])
    out += bytes(1024)
    assert lay["total"] == len(out)
    return bytes(out), lay


# one name per rule: plain name field (1, 99, 100 bytes), 101 bytes without
# a slash (PAX), 101 bytes with a usable split (prefix field), 256 bytes
# without a slash (PAX), and a name whose only slash leaves a 160-byte
# prefix (> 155, so PAX again)
NAMES = [
    "a",
    "b" * 99,
    "c" * 100,
    "d" * 101,
    "dir/" + "e" * 97,
    "f" * 256,
    "g" * 160 + "/" + "h" * 20,
]


def test_layout_readable_by_tarfile():
    assert [len(n) for n in NAMES] == [1, 99, 100, 101, 101, 256, 181]
    payloads = {n: os.urandom(37 * (i + 1) + i) for i, n in enumerate(NAMES)}
    blob, lay = assemble(NAMES, payloads)
    # header_len says which rule was used
    lens = [e["header_len"] for e in lay["entries"]]
    assert lens == [512, 512, 512, 1024 + 512, 512, 1024 + 512, 1024 + 512]
    with tarfile.open(fileobj=io.BytesIO(blob), mode="r:") as tf:
        infos = tf.getmembers()
        assert [ti.name for ti in infos] == NAMES
        for ti in infos:
            assert ti.isreg()
            assert ti.size == len(payloads[ti.name])
            assert tf.extractfile(ti).read() == payloads[ti.name]
            assert ti.mode == 0o644
            assert ti.mtime == 0
            assert ti.uid == 0 and ti.gid == 0
            assert ti.uname == "" and ti.gname == "" and ti.linkname == ""


def test_header_fields():
    lay = _core.tar_pack_layout([("dir/" + "e" * 97, 0o1234567), ("f" * 256, 5)])
    h = lay["headers"]
    assert len(h) == 512 + 1024 + 512
    # prefix-field member
    assert h[0:97] == b"e" * 97 and h[97:100] == bytes(3)
    assert h[345:348] == b"dir" and h[348] == 0
    assert h[100:108] == b"0000644\0"
    assert h[108:116] == b"0000000\0" and h[116:124] == b"0000000\0"
    assert h[124:136] == b"00001234567\0"
    assert h[136:148] == b"00000000000\0"
    assert h[156:157] == b"0"
    assert h[157:257] == bytes(100)
    assert h[257:265] == b"ustar\x0000"
    assert h[265:329] == bytes(64)
    # PAX member: 'x' header, one self-consistent path= record, truncated name
    x = h[512:1024]
    assert x[156:157] == b"x"
    rec = b"266 path=" + b"f" * 256 + b"\n"
    assert len(rec) == 266
    assert int(x[124:135], 8) == 266
    assert h[1024:1024 + 266] == rec and h[1024 + 266:1536] == bytes(512 - 266)
    m = h[1536:2048]
    assert m[0:100] == b"f" * 100 and m[156:157] == b"0"


@pytest.mark.parametrize("dir_len", [1, 50, 886, 887, 888, 889])
def test_pax_record_length_is_self_consistent(dir_len):
    """The record length counts its own digits; 887/888 straddle the step
    from a 999-byte to a 1001-byte record (1000 cannot exist)."""
    name = "n" * dir_len + "/" + "m" * 101  # no usable split: PAX
    lay = _core.tar_pack_layout([(name, 0)])
    h = lay["headers"]
    size = int(h[124:135], 8)
    rec = h[512:512 + size]
    num, rest = rec.split(b" ", 1)
    assert int(num) == len(rec) == size
    assert rest == b"path=" + name.encode() + b"\n"
    assert lay["entries"][0]["header_len"] == 1024 + _pad(size)


def test_sizes_and_total():
    sizes = [0, 1, 511, 512, 513]
    members = [f"m{s}" for s in sizes]
    lay = _core.tar_pack_layout(list(zip(members, sizes)))
    off = 0
    for e, s in zip(lay["entries"], sizes):
        assert e["header_off"] == off
        assert e["header_len"] == 512
        assert e["payload_off"] == off + 512
        assert e["size"] == s
        off += 512 + _pad(s)
    assert off == 512 * 5 + 0 + 512 + 512 + 512 + 1024
    assert lay["total"] == off + 1024
    assert lay["total"] % 512 == 0
    blob, _ = assemble(members, {m: b"\xff" * s for m, s in zip(members, sizes)})
    assert blob[-1024:] == bytes(1024)
    # an empty member list is just the end marker
    assert _core.tar_pack_layout([])["total"] == 1024


@pytest.mark.parametrize("members", [
    [("", 1)],
    [("/abs", 1)],
    [("a/../b", 1)],
    [("..", 1)],
    [("a/..", 1)],
    [("dir/", 1)],
    [("a//b", 1)],
    [("./a", 1)],
    [("a/./b", 1)],
    [("nul\0name", 1)],
    [("dup", 1), ("other", 2), ("dup", 3)],
    [("big", 8 << 30)],
])
def test_rejections(members):
    with pytest.raises(ValueError):
        _core.tar_pack_layout(members)


def test_accepts_edge_names_and_sizes():
    # '..' only as a whole component; the largest size the octal field holds
    lay = _core.tar_pack_layout([("a..b/..c/d..", 1), ("big", (8 << 30) - 1)])
    assert lay["headers"][512 + 124:512 + 136] == b"77777777777\0"


def test_member_count_limit():
    """tar_index reads back at most 65536 header entries; a PAX member costs
    two. The pack side refuses what the pull side could not index."""
    assert _core.tar_pack_layout([(f"m{i}", 0) for i in range(65536)])["total"] == \
        65536 * 512 + 1024
    with pytest.raises(ValueError):
        _core.tar_pack_layout([(f"m{i}", 0) for i in range(65537)])
    long_names = ["L" * 200 + str(i) for i in range(32769)]
    _core.tar_pack_layout([(n, 0) for n in long_names[:32768]])
    with pytest.raises(ValueError):
        _core.tar_pack_layout([(n, 0) for n in long_names])


def test_deterministic():
    members = [(n, i * 1000) for i, n in enumerate(NAMES)]
    a = _core.tar_pack_layout(members)
    b = _core.tar_pack_layout(members)
    assert a["headers"] == b["headers"]
    assert a["entries"] == b["entries"] and a["total"] == b["total"]


def test_selftest_under_sanitizers(tmp_path):
    """tools/tar_pack_selftest.cpp: the header-only builder in its own
    process under ASan + UBSan."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = tmp_path / "tar_pack_selftest"
    build = subprocess.run(
        [gxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined",
         # static runtimes: the dynamic ASan runtime refuses to start
         # unless it is the first library loaded, which the program cannot
         # promise when the caller's environment preloads another one
         "-static-libasan", "-static-libubsan",
         "-I" + os.path.join(REPO, "core", "include"),
         os.path.join(REPO, "tools", "tar_pack_selftest.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stderr == ""
