"""Tar archives for the index tests: foreign ones written by Python's
``tarfile`` in its three formats, hand-built headers for the constructs
``tarfile`` reads but never writes, and damaged archives derived from good
ones. Everything is generated at run time from fixed seeds; apart from
``many_members`` every archive is below 256 KiB.

``listing`` is the reference: ``tarfile``'s regular-file members. Our own
writer (tar_host.hpp) emits only ustar headers with octal sizes, the prefix
field and one PAX ``path=`` record, so an index fed only its output never runs
GNU long names, base-256 sizes, V7 headers or any rejection.

Needs neither torch nor the extension.
"""
import functools
import io
import random
import tarfile

BLOCK = 512
MIB = 1 << 20
MAX_INDEX_ENTRIES = 65536  # tarhost::kMaxIndexEntries


def pad(n: int) -> int:
    return (n + BLOCK - 1) & ~(BLOCK - 1)


def listing(blob: bytes):
    """tarfile's view: what tar_index must return for a well-formed archive."""
    with tarfile.open(fileobj=io.BytesIO(blob), mode="r:") as tf:
        return [{"name": ti.name, "offset": ti.offset_data, "size": ti.size, "mode": ti.mode}
                for ti in tf.getmembers() if ti.isfile()]


def payloads(blob: bytes):
    """[(name, bytes)] of the regular files in `listing` order, read by
    tarfile (a list: an archive may repeat a name)."""
    with tarfile.open(fileobj=io.BytesIO(blob), mode="r:") as tf:
        return [(ti.name, tf.extractfile(ti).read()) for ti in tf.getmembers() if ti.isfile()]


# ---------------------------------------------------------- tarfile-written --

SIZES = [0, 1, 511, 512, 513, 70001]


def _info(name, size=0, type_=tarfile.REGTYPE, mode=0o644, linkname=""):
    ti = tarfile.TarInfo(name)
    ti.size = size
    ti.type = type_
    ti.mode = mode
    ti.linkname = linkname
    ti.mtime = 1_600_000_000
    ti.uid = ti.gid = 1000
    ti.uname = ti.gname = "corpus"
    return ti


def _written(fmt, seed):
    rng = random.Random(seed)
    names = [
        "a",                          # 1 byte
        "b" * 99,
        "c" * 100,                    # fills the name field, no NUL
        "dir/" + "e" * 97,            # 101 bytes with a usable prefix split
        "p" * 155 + "/" + "q" * 100,  # 256 bytes, both fields full
        "naïve/日本語.bin",  # UTF-8
    ]
    if fmt != tarfile.USTAR_FORMAT:  # ustar cannot carry these at all
        names += [
            "d" * 101,                   # no slash: GNU 'L' / PAX path=
            "f" * 256,
            "g" * 160 + "/" + "h" * 20,  # the only slash leaves a 160-byte prefix
        ]
    assert {len(n) for n in names} >= {1, 99, 100, 101, 256}
    pax_global = {"comment": "tar index corpus"} if fmt == tarfile.PAX_FORMAT else None
    bio = io.BytesIO()
    with tarfile.open(fileobj=bio, mode="w", format=fmt, pax_headers=pax_global) as tf:
        tf.addfile(_info("dir", type_=tarfile.DIRTYPE, mode=0o755))
        for i, name in enumerate(names):
            size = SIZES[i % len(SIZES)]
            tf.addfile(_info(name, size, mode=0o600 + i), io.BytesIO(rng.randbytes(size)))
            if i == 0:
                tf.addfile(_info("sym", type_=tarfile.SYMTYPE, linkname="a", mode=0o777))
                tf.addfile(_info("hard", type_=tarfile.LNKTYPE, linkname="a"))
        if fmt != tarfile.USTAR_FORMAT:
            # a long-named directory directly before a file: the directory
            # consumes the long name, the file keeps its own
            tf.addfile(_info("D" * 120, type_=tarfile.DIRTYPE, mode=0o755))
            tf.addfile(_info("after-long-dir", 513), io.BytesIO(rng.randbytes(513)))
            # long target and long name: GNU writes 'K' then 'L'
            tf.addfile(_info("s" * 120, type_=tarfile.SYMTYPE, linkname="t" * 150))
            tf.addfile(_info("after-long-link", 1), io.BytesIO(rng.randbytes(1)))
        if fmt == tarfile.PAX_FORMAT:
            # records beside path=: a fractional mtime and a non-ASCII uname
            ti = _info("x" * 130, 511)
            ti.mtime = 1_600_000_000.25
            ti.uname = "üser"
            tf.addfile(ti, io.BytesIO(rng.randbytes(511)))
            # records without path=
            ti = _info("short-with-pax", 512)
            ti.pax_headers = {"comment": "no path here"}
            tf.addfile(ti, io.BytesIO(rng.randbytes(512)))
    return bio.getvalue()


# --------------------------------------------------------------- hand-built --

def octal(v: int, width: int) -> bytes:
    """`width`-byte field: width-1 zero-padded octal digits and a NUL."""
    return b"%0*o\0" % (width - 1, v)


def base256(v: int) -> bytes:
    """12-byte GNU base-256 size field (two's complement when negative)."""
    if v >= 0:
        return b"\x80" + v.to_bytes(11, "big")
    return b"\xff" + (v + (1 << 88)).to_bytes(11, "big")


def header(name: bytes, size=0, typeflag=b"0", *, mode=octal(0o644, 8), magic=b"ustar\x0000",
           prefix=b"", linkname=b"", signed_sum=False) -> bytes:
    """One 512 B header. `size` and `mode` may be raw field bytes."""
    size_field = size if isinstance(size, bytes) else octal(size, 12)
    assert len(name) <= 100 and len(size_field) == 12 and len(mode) == 8 and len(magic) == 8
    h = bytearray(BLOCK)
    h[0:len(name)] = name
    h[100:108] = mode
    h[108:116] = octal(0, 8)
    h[116:124] = octal(0, 8)
    h[124:136] = size_field
    h[136:148] = octal(0, 12)
    h[148:156] = b" " * 8
    h[156:157] = typeflag
    h[157:157 + len(linkname)] = linkname
    h[257:265] = magic
    h[345:345 + len(prefix)] = prefix
    return fix_checksum(h, signed_sum)


def fix_checksum(h, signed_sum=False) -> bytes:
    h = bytearray(h)
    h[148:156] = b" " * 8
    total = sum(b - 256 if signed_sum and b >= 128 else b for b in h)
    h[148:156] = b"%06o\0 " % total
    return bytes(h)


def member(name: bytes, data: bytes, **kw) -> bytes:
    kw.setdefault("size", len(data))
    return header(name, **kw) + data + bytes(pad(len(data)) - len(data))


END = bytes(2 * BLOCK)


def pax_record(key: str, value: str) -> bytes:
    body = f" {key}={value}\n".encode()
    n = len(body) + 1
    while len(str(n)) + len(body) != n:
        n = len(str(n)) + len(body)
    return str(n).encode() + body


def _hand_built():
    rng = random.Random(77)
    d700, d513, d70001 = rng.randbytes(700), rng.randbytes(513), rng.randbytes(70001)
    two = member(b"m1", d700) + member(b"m2", d513)
    out = {
        "size-space-terminated": member(b"sp", d700, size=b"00000001274 ") + END,
        "size-leading-spaces": member(b"lead", d700, size=b"       1274\0") + END,
        "size-all-spaces": member(b"blank", b"", size=b" " * 12) + member(b"next", d513) + END,
        # old V7: no magic, typeflag NUL; a name ending in '/' is a directory
        "v7": (member(b"old", d700, typeflag=b"\0", magic=bytes(8))
               + header(b"olddir/", typeflag=b"\0", magic=bytes(8))
               + member(b"olddir/f", d513, typeflag=b"\0", magic=bytes(8)) + END),
        "gnu-magic": member(b"gnu", d700, magic=b"ustar  \0") + END,
        "contiguous-7": member(b"cont", d700, typeflag=b"7") + member(b"m2", d513) + END,
        "base256-700": member(b"b700", d700, size=base256(700)) + member(b"m2", d513) + END,
        "base256-70001": member(b"b70001", d70001, size=base256(70001)) + member(b"m2", d513) + END,
        "signed-checksum": member("éèê.bin".encode(), d700, signed_sum=True) + END,
        "no-end-marker": two,
        "one-end-block": two + bytes(BLOCK),
        "data-after-end": two + END + b"\xff" * 1500,
        "end-marker-only": END,
        # non-regular entries with a size field: nothing is stored after them
        "sized-directory": header(b"d", size=700, typeflag=b"5") + member(b"m2", d513) + END,
        # a name in the prefix field under another magic still counts
        "prefix": member(b"leaf", d700, prefix=b"some/dir") + END,
        # hand-written long names: 'L' with and without the trailing NUL
        "gnu-longname": (member(b"././@LongLink", b"L" * 150 + b"\0", typeflag=b"L")
                         + member(b"L" * 100, d700)
                         + member(b"././@LongLink", b"M" * 512, typeflag=b"L")
                         + member(b"M" * 100, d513) + END),
        # 'L' before 'x': tarfile lets the outer one win
        "longname-then-pax": (member(b"././@LongLink", b"outer\0", typeflag=b"L")
                              + member(b"PaxHeader", pax_record("path", "inner"), typeflag=b"x")
                              + member(b"field", d700) + member(b"m2", d513) + END),
        "pax-then-longname": (member(b"PaxHeader", pax_record("path", "outer"), typeflag=b"x")
                              + member(b"././@LongLink", b"inner\0", typeflag=b"L")
                              + member(b"field", d700) + member(b"m2", d513) + END),
        # 'L' then 'K': the link target must not eat the name
        "longname-then-longlink": (member(b"././@LongLink", b"the-name\0", typeflag=b"L")
                                   + member(b"././@LongLink", b"the-target\0", typeflag=b"K")
                                   + member(b"field", d700) + member(b"m2", d513) + END),
        "pax-global-path": (member(b"GlobalHead", pax_record("path", "everyone"), typeflag=b"g")
                            + member(b"m1", d700)
                            + member(b"PaxHeader", pax_record("path", "own"), typeflag=b"x")
                            + member(b"m2", d513) + member(b"m3", b"z") + END),
        "pax-path-trailing-slash": (member(b"PaxHeader", pax_record("path", "p/q/"),
                                           typeflag=b"x")
                                    + member(b"field", d700) + END),
        # the last payload ends exactly at tar_len
        "exact-fit": member(b"m1", d700) + member(b"full", d513 + d513[:511]),
    }
    return out


@functools.lru_cache(maxsize=None)
def good_archives():
    """{name: archive}: well-formed, tar_index must equal `listing`."""
    out = {
        "tarfile-ustar": _written(tarfile.USTAR_FORMAT, 1),
        "tarfile-gnu": _written(tarfile.GNU_FORMAT, 2),
        "tarfile-pax": _written(tarfile.PAX_FORMAT, 3),
    }
    out.update(_hand_built())
    assert all(len(a) < 256 << 10 for a in out.values())
    return out


@functools.lru_cache(maxsize=None)
def ragged_archives():
    """{name: (archive, expected listing)}: lengths that are 0, below 512 or
    no multiple of 512. The listing is the entries before the ragged end;
    tarfile agrees except that it calls an empty or sub-header file an
    error."""
    rng = random.Random(5)
    m1, m2 = member(b"m1", rng.randbytes(700)), member(b"m2", rng.randbytes(513))
    first = listing(m1 + END)
    return {
        "empty": (b"", []),
        "below-512": (m1[:100], []),
        "511": (m1[:511], []),
        "header-cut": (m1 + m2[:300], first),
        "end-block-cut": (m1 + bytes(100), first),
        "second-end-block-cut": (m1 + bytes(BLOCK + 7), first),
        "junk-tail": (m1 + b"\xff" * 511, first),
    }


def _set_size(archive: bytes, header_off: int, size_field: bytes) -> bytes:
    a = bytearray(archive)
    a[header_off + 124:header_off + 136] = size_field
    a[header_off:header_off + BLOCK] = fix_checksum(a[header_off:header_off + BLOCK])
    return bytes(a)


@functools.lru_cache(maxsize=None)
def bad_archives():
    """{name: archive}: each must raise. Every one is a good archive with one
    thing wrong; none claims more than 1 MiB beyond its length."""
    rng = random.Random(99)
    d700, d513 = rng.randbytes(700), rng.randbytes(513)
    m1, m2 = member(b"m1", d700), member(b"m2", d513)
    h2 = len(m1)  # offset of the 2nd header
    two = m1 + m2  # no end marker: tar_len is where the last padding ends
    assert listing(two + END) == listing(two) and len(listing(two)) == 2
    long_name = "n" * 200
    x = member(b"PaxHeader", pax_record("path", long_name), typeflag=b"x")
    g = member(b"GlobalHead", pax_record("comment", "c" * 600), typeflag=b"g")
    lname = member(b"././@LongLink", long_name.encode() + b"\0", typeflag=b"L")
    body = member(long_name[:100].encode(), d513)
    for good in (x + body + END, lname + body + END, g + m1 + END):
        assert [e["size"] for e in listing(good)] in ([513], [700])

    def flipped():
        a = bytearray(two + END)
        a[h2 + 1] ^= 0x01
        return bytes(a)

    def pax(payload: bytes, typeflag=b"x"):
        return member(b"PaxHeader", payload, typeflag=typeflag) + m1 + END

    out = {
        "payload-truncated": two[:h2 + BLOCK + 100],
        "padding-missing": two[:h2 + BLOCK + 513],
        "padding-one-short": two[:-1],
        "size-overruns-by-1": _set_size(two, h2, octal(1024 + 1, 12)),
        "size-overruns-by-1MiB": _set_size(two, h2, octal(1024 + MIB, 12)),
        "base256-size-overruns-by-1": _set_size(two, h2, base256(1024 + 1)),
        "x-truncated": (x + body)[:BLOCK + 100],
        "x-header-only": (x + body)[:BLOCK],
        "L-truncated": (lname + body)[:BLOCK + 100],
        "g-truncated": (g + m1)[:BLOCK + 512],
        "name-byte-flipped": flipped(),
        "garbage-block": m1 + rng.randbytes(BLOCK) + m2 + END,
        "checksum-field-junk": m1 + m2[:148] + b"zzzzzz\0 " + m2[156:] + END,
        "base256-negative": _set_size(two + END, h2, base256(-513)),
        "base256-sign-bit": _set_size(two + END, h2, b"\xc0" + bytes(9) + b"\x02\x01"),
        "base256-2^63": _set_size(two + END, h2, base256(1 << 63)),
        "base256-above-2^63": _set_size(two + END, h2, base256((1 << 63) + 513)),
        "base256-2^87": _set_size(two + END, h2, base256(1 << 87)),
        "size-not-octal": _set_size(two + END, h2, b"0000000z001\0"),
        "size-digit-8": _set_size(two + END, h2, b"00000001008\0"),
        "size-high-byte": _set_size(two + END, h2, b"\x81" + bytes(9) + b"\x02\x01"),
        "pax-size": pax(pax_record("path", "renamed") + pax_record("size", "700")),
        "pax-global-size": pax(pax_record("size", "700"), typeflag=b"g"),
        "pax-record-length-0": pax(b"0 path=abc\n"),
        "pax-record-length-past-payload": pax(b"99 path=abc\n"),
        "pax-record-no-length": pax(b"path=abc\n"),
        "pax-record-no-newline": pax(b"11 path=abc"),
        "pax-record-no-equals": pax(b"11 pathabc\n"),
        "pax-record-trailing-junk": pax(pax_record("path", "abc") + b"\0\0\0"),
    }
    for name, a in out.items():
        assert len(a) < 256 << 10, name
    return out


def many_members(n=MAX_INDEX_ENTRIES + 1) -> bytes:
    """`n` empty members: 512 B per header. 65537 is one more than the index
    holds; the one large archive (32 MiB), for the host model only."""
    return header(b"m") * n + END
