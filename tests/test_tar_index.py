"""The tar index on host bytes: ``_core.tar_index_host`` runs the header walk
that ``tar_index_kernel`` runs (core/include/modelx/tar_core.hpp) and the name
resolution of ``GpuEngine::tar_index`` (tar_host.hpp). No GPU needed.

Python's ``tarfile`` is the reference on every well-formed archive of
util_tarcorpus.py. On damaged ones the contract is stricter than ``tarfile``,
which quietly ends its listing at a bad header past offset 0: every such
archive must raise, and the tests that cover these say what ``tarfile`` does
instead. A stand-alone C++ self-test walks archives in buffers of exactly
``tar_len`` bytes under ASan/UBSan.
"""
import os
import shutil
import subprocess
import tarfile

import pytest
import util_tarcorpus as tc

_core = pytest.importorskip("modelx_amd._core")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOOD = sorted(tc.good_archives())
RAGGED = sorted(tc.ragged_archives())
BAD = sorted(tc.bad_archives())


# ------------------------------------------------------------ the corpus ---

def _typeflags(blob):
    """Typeflags of the headers, by a plain walk over a well-formed archive
    (octal or base-256 size; links, directories and devices store nothing)."""
    flags, off = [], 0
    while off + 512 <= len(blob) and any(blob[off:off + 512]):
        field = blob[off + 124:off + 136]
        if field[0] == 0x80:
            size = int.from_bytes(field[1:], "big")
        else:
            size = int(field.split(b"\0")[0].strip() or b"0", 8)
        flag = blob[off + 156:off + 157]
        flags.append(flag)
        off += 512 + (0 if flag in b"123456" else tc.pad(size))
    return flags


def test_corpus_holds_what_it_claims():
    """The installed tarfile wrote the constructs the corpus is named for."""
    good = tc.good_archives()
    ustar, gnu, pax = (_typeflags(good[k]) for k in ("tarfile-ustar", "tarfile-gnu",
                                                      "tarfile-pax"))
    assert set(ustar) == {b"0", b"1", b"2", b"5"}
    assert good["tarfile-ustar"][345:346] == b"\0"  # 'dir' itself: no prefix
    assert any(good["tarfile-ustar"][o + 345:o + 346] != b"\0"
               for o in range(0, len(good["tarfile-ustar"]), 512)
               if good["tarfile-ustar"][o + 257:o + 262] == b"ustar")
    assert set(gnu) == {b"0", b"1", b"2", b"5", b"L", b"K"}
    # 'L' directly before a directory, which is directly before a file
    assert any(gnu[i:i + 3] == [b"L", b"5", b"0"] for i in range(len(gnu)))
    # 'K' then 'L' then the symlink, then a file
    assert any(gnu[i:i + 4] == [b"K", b"L", b"2", b"0"] for i in range(len(gnu)))
    assert pax[0] == b"g" and set(pax) == {b"0", b"1", b"2", b"5", b"g", b"x"}
    assert b" mtime=" in good["tarfile-pax"] and b" uname=" in good["tarfile-pax"]
    sizes = {e["size"] for k in ("tarfile-ustar", "tarfile-gnu", "tarfile-pax")
             for e in tc.listing(good[k])}
    assert sizes >= set(tc.SIZES)
    for k in ("tarfile-gnu", "tarfile-pax"):
        lens = {len(e["name"].encode()) for e in tc.listing(good[k])}
        assert lens >= {1, 99, 100, 101, 256}
    assert {len(e["name"].encode()) for e in tc.listing(good["tarfile-ustar"])} >= \
        {1, 99, 100, 101, 256}
    # the hand-built headers are what they say
    assert good["base256-700"][124:136] == b"\x80" + bytes(9) + b"\x02\xbc"
    h = good["signed-checksum"][:512]
    unsigned = sum(h[:148]) + 256 + sum(h[156:])
    assert int(h[148:154], 8) != unsigned  # only the signed sum matches
    assert good["v7"][257:265] == bytes(8) and good["v7"][156] == 0


# ------------------------------------------------------------- well-formed --

@pytest.mark.parametrize("name", GOOD)
def test_matches_tarfile(name):
    blob = tc.good_archives()[name]
    ref = tc.listing(blob)
    assert _core.tar_index_host(blob) == ref
    # and the offsets point at the bytes tarfile extracts
    data = tc.payloads(blob)
    assert len(data) == len(ref)
    for e, (name, payload) in zip(ref, data):
        assert name == e["name"] and blob[e["offset"]:e["offset"] + e["size"]] == payload


def test_listing_is_not_trivial():
    """Guards the reference itself: the listings the comparisons rest on hold
    the members the corpus wrote."""
    good = tc.good_archives()
    assert len(tc.listing(good["tarfile-ustar"])) == 6
    assert len(tc.listing(good["tarfile-gnu"])) == 11
    assert len(tc.listing(good["tarfile-pax"])) == 13
    names = [e["name"] for e in tc.listing(good["tarfile-gnu"])]
    assert "D" * 120 not in names and "after-long-dir" in names and "after-long-link" in names
    assert [e["name"] for e in tc.listing(good["longname-then-longlink"])] == ["the-name", "m2"]
    assert [e["name"] for e in tc.listing(good["longname-then-pax"])] == ["outer", "m2"]
    assert [e["name"] for e in tc.listing(good["pax-then-longname"])] == ["outer", "m2"]
    assert [e["name"] for e in tc.listing(good["pax-global-path"])] == \
        ["everyone", "own", "everyone"]
    assert [e["name"] for e in tc.listing(good["v7"])] == ["old", "olddir/f"]
    assert [e["size"] for e in tc.listing(good["base256-70001"])] == [70001, 513]
    assert [e["name"] for e in tc.listing(good["contiguous-7"])] == ["cont", "m2"]


def test_own_pack_layout_indexes():
    """The archive the pack side lays out, through the host index."""
    names = ["a", "c" * 100, "d" * 101, "dir/" + "e" * 97, "f" * 256]
    sizes = [0, 1, 513, 70001, 512]
    lay = _core.tar_pack_layout(list(zip(names, sizes)))
    blob, hoff = bytearray(), 0
    for e in lay["entries"]:
        blob += lay["headers"][hoff:hoff + e["header_len"]] + bytes(tc.pad(e["size"]))
        hoff += e["header_len"]
    blob += bytes(1024)
    got = _core.tar_index_host(bytes(blob))
    assert got == tc.listing(bytes(blob))
    assert [(g["name"], g["size"], g["offset"]) for g in got] == \
        [(n, s, e["payload_off"]) for n, s, e in zip(names, sizes, lay["entries"])]


@pytest.mark.parametrize("name", RAGGED)
def test_ragged_lengths(name):
    """tar_len of 0, below 512 and no multiple of 512: the entries before the
    ragged end. tarfile agrees wherever it reads the file at all (it calls an
    empty file and a lone partial header errors)."""
    blob, expect = tc.ragged_archives()[name]
    assert len(blob) == 0 or len(blob) % 512
    assert _core.tar_index_host(blob) == expect
    try:
        ref = tc.listing(blob)
    except tarfile.ReadError:
        assert expect == [] and len(blob) < 512
    else:
        assert ref == expect


def test_entry_count_limit_is_inclusive():
    got = _core.tar_index_host(tc.many_members(tc.MAX_INDEX_ENTRIES))
    assert len(got) == tc.MAX_INDEX_ENTRIES
    assert got[-1] == {"name": "m", "offset": tc.MAX_INDEX_ENTRIES * 512, "size": 0,
                       "mode": 0o644}


# --------------------------------------------------------------- malformed --

@pytest.mark.parametrize("name", BAD)
def test_rejected(name):
    with pytest.raises(RuntimeError) as exc:
        _core.tar_index_host(tc.bad_archives()[name])
    assert str(exc.value).startswith("tar_index: ")
    assert "header offset" in str(exc.value)


def test_too_many_members_rejected():
    """65537 headers: one more than the index holds (32 MiB, host only)."""
    with pytest.raises(RuntimeError, match="too many entries"):
        _core.tar_index_host(tc.many_members())


@pytest.mark.parametrize("name, cause, offset", [
    ("payload-truncated", "extends past the end", 1536),
    ("padding-missing", "extends past the end", 1536),
    ("size-overruns-by-1", "extends past the end", 1536),
    ("size-overruns-by-1MiB", "extends past the end", 1536),
    ("x-truncated", "extends past the end", 0),
    ("L-truncated", "extends past the end", 0),
    ("g-truncated", "extends past the end", 0),
    ("name-byte-flipped", "checksum", 1536),
    ("garbage-block", "checksum", 1536),
    ("base256-negative", "negative base-256", 1536),
    ("base256-above-2^63", "does not fit 63 bits", 1536),
    ("size-not-octal", "neither octal nor base-256", 1536),
    ("pax-size", "size= record", 0),
    ("pax-record-length-0", "malformed PAX record", 0),
    ("pax-record-length-past-payload", "malformed PAX record", 0),
])
def test_error_names_cause_and_offset(name, cause, offset):
    with pytest.raises(RuntimeError) as exc:
        _core.tar_index_host(tc.bad_archives()[name])
    assert cause in str(exc.value)
    assert str(exc.value).endswith(f"at header offset {offset}")


def test_stricter_than_tarfile():
    """tarfile ends its listing without a word at a bad header past offset
    0 and returns what came before; the same archives raise here. (At offset
    0 tarfile raises too.)"""
    bad = tc.bad_archives()
    for name in ("name-byte-flipped", "garbage-block", "checksum-field-junk",
                 "base256-negative", "size-not-octal"):
        assert [e["name"] for e in tc.listing(bad[name])] == ["m1"], name
        with pytest.raises(RuntimeError):
            _core.tar_index_host(bad[name])
    # tarfile honours size=; the index refuses it and does not half-support it
    assert [e["name"] for e in tc.listing(bad["pax-size"])] == ["renamed"]
    # the same bad block first: both refuse
    first = bad["garbage-block"][1536:]
    with pytest.raises(tarfile.ReadError):
        tc.listing(first)
    with pytest.raises(RuntimeError):
        _core.tar_index_host(first)


def test_every_prefix_of_an_archive_is_safe():
    """Cut a two-member archive at every length around each boundary: the
    result is the listing of the members that are whole, or an error when
    the cut falls inside a member. Never anything else."""
    blob = tc.good_archives()["no-end-marker"]  # header, 700 B, header, 513 B
    full = tc.listing(blob)
    ends = [0, 512 + 1024, len(blob)]  # where 0, 1 and 2 members are complete
    cuts = {c + d for c in (0, 512, 512 + 700, 1536, 2048, 2048 + 513, len(blob))
            for d in (-1, 0, 1, 511) if 0 <= c + d <= len(blob)}
    for cut in sorted(cuts):
        whole = max(i for i, e in enumerate(ends) if e <= cut)
        inside_header = cut - ends[whole] < 512
        if inside_header:
            assert _core.tar_index_host(blob[:cut]) == full[:whole], cut
        else:
            with pytest.raises(RuntimeError, match="extends past the end"):
                _core.tar_index_host(blob[:cut])


# --------------------------------------------------------------- sanitizers --

def test_selftest_under_sanitizers(tmp_path):
    """tools/tar_index_selftest.cpp: the walk and the name resolution in
    their own process under ASan + UBSan, every archive in a heap buffer of
    exactly tar_len bytes."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = tmp_path / "tar_index_selftest"
    build = subprocess.run(
        [gxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined",
         # static runtimes: the dynamic ASan runtime refuses to start
         # unless it is the first library loaded, which the program cannot
         # promise when the caller's environment preloads another one
         "-static-libasan", "-static-libubsan",
         "-I" + os.path.join(REPO, "core", "include"),
         os.path.join(REPO, "tools", "tar_index_selftest.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stderr == ""
