"""The gzip host model (modelx/deflate_core.hpp, ``_core.gzip_compress_host``)
against zlib: every payload and length round-trips, the trailer and the bound
hold, the bytes are deterministic, and the sizes show that matches, Huffman
coding and the stored fallback each took effect. Payload families built for one
edge each (largest distance, longest codes, widest tokens, fewest symbols) with
the proof, from ``_core.gzip_chunk_stats_host``, that the model reaches it. The
Huffman builder alone (``_core.deflate_code_lengths_host``) on a list of
histograms, against the Kraft sum, zlib and package-merge; test_gpu_gzip runs
the same payloads and histograms through the kernels. The ``dir_format``
rules."""
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


# ---- payloads built for one edge each; the tests after the round trip prove it

MAXDIST_MOTIF = bytes(random.Random(3).sample(range(1, 256), 19))


def maxdist(seed):
    """Nineteen distinct non-zero bytes at 0 and again at C - 4, zeros between:
    from every source offset up to 15 the chunk starts with four bytes that it
    holds again as its last four, and the zero run between them lives in one
    hash bucket, so the first entry survives: one match of C - 4."""
    out = bytearray(TOTAL)
    out[0:19] = MAXDIST_MOTIF
    out[C - 4:C + 15] = MAXDIST_MOTIF
    return bytes(out)


def maxdist_next(seed):
    """The same motif, its repeat at the first position of the next chunk: no
    chunk may reach it."""
    out = bytearray(TOTAL)
    out[0:19] = MAXDIST_MOTIF
    out[C:C + 19] = MAXDIST_MOTIF
    return bytes(out)


def longcodes(seed):
    """Chunk 0: 48 equally likely literals and twelve bytes that occur once, so
    that the lit/len tree keeps a 15-bit code. Chunk 1: 21 byte values with
    Fibonacci counts, shuffled: thousands of short matches whose distance codes
    are as skewed, for the longest distance code."""
    r = random.Random(seed)
    first = bytearray(r.randrange(48) for _ in range(C))
    for i in range(12):
        first[1000 + 777 * i] = 200 + i
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    second = [40 + i for i, c in enumerate(fib) for _ in range(c)]
    r.shuffle(second)
    second += [r.randrange(40, 61) for _ in range(TOTAL - C - len(second))]
    return bytes(first) + bytes(second)


def _wide_chunk(r, nseg, lo, hi, letters, tail=0):
    """`nseg` random segments of lo..hi bytes near the start of a chunk and
    again near its end, over a background of few letters: the background's many
    short matches make every far, long match a rare symbol twice over. `tail`
    moves the copies forward, to set the distance and with it the extra bits,
    which are a wide token's topmost."""
    out = bytearray(r.choice(letters) for _ in range(C))
    segs = [r.randbytes(r.randrange(lo, hi + 1)) for _ in range(nseg)]
    p, q = 20, C - 20 - tail
    for s in segs:
        out[p:p + len(s)] = s
        p += len(s) + 6
    for s in reversed(segs):
        q -= len(s)
        out[q:q + len(s)] = s
        q -= 6
    assert p < q
    return out


def widetokens(seed):
    """Chunk 0: 48 far matches of 67..257 bytes (length codes with 4 and 5
    extra bits, distance codes with 13), enough of them to meet the bit phases
    at which a token spills into a third word, at a distance whose extra bits,
    the token's topmost, are not zero there. Chunk 1: two of them, as rare
    as they get, for the widest token. The two seeds are the best of a few
    dozen tried on the host model."""
    out = _wide_chunk(random.Random(26), 48, 67, 257, b"acgtxy", tail=600)
    out += _wide_chunk(random.Random(48), 2, 131, 257, b"acgtxy")
    r = random.Random(seed)
    out += bytes(r.choice(b"acgt") for _ in range(TOTAL - len(out)))
    return bytes(out)


def onesymbol(seed):
    return b"\xa7" * TOTAL


def twosymbols(seed):
    return b"\x00\xff" * (TOTAL // 2) + b"\x00" * (TOTAL % 2)


# the seeds of the first five are the ones they have always had
PAYLOADS = {"far": far, "onebyte_runs": onebyte_runs, "random": rand, "words": words,
            "zeros": zeros, "maxdist": maxdist, "maxdist_next": maxdist_next,
            "longcodes": longcodes, "widetokens": widetokens, "onesymbol": onesymbol,
            "twosymbols": twosymbols}
SEEDS = {name: 11 + i for i, name in enumerate(PAYLOADS)}


@functools.lru_cache(maxsize=None)
def payload(name):
    return PAYLOADS[name](SEEDS[name])


@functools.lru_cache(maxsize=None)
def model(name, offset, n):
    return _core.gzip_compress_host(payload(name)[offset:offset + n])


def check_member(out, x):
    """zlib reads the member `out` as `x`, as a gzip file and as a raw stream
    that ends (BFINAL on the last block and on no other) exactly where the
    trailer starts, and the trailer is x's."""
    assert zlib.decompress(out, 31) == x
    raw = zlib.decompressobj(-15)
    assert raw.decompress(out[10:]) == x
    assert raw.eof and raw.unused_data == out[-8:] and len(out) >= 18
    assert out[-8:] == zlib.crc32(x).to_bytes(4, "little") + (len(x) % 2**32).to_bytes(4, "little")


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_host_model_round_trips(name, n):
    x = payload(name)[:n]
    out = model(name, 0, n)
    check_member(out, x)
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


# ------------------------------------------- the payloads reach their edges --

OFFSETS = [0, 1, 5, 15]  # the GPU test's source phases


@functools.lru_cache(maxsize=None)
def stats(name, offset, chunk, n=C):
    """``gzip_chunk_stats_host`` of chunk `chunk` of the payload read from
    `offset`, as the host model and the kernel see it."""
    at = offset + chunk * C
    return _core.gzip_chunk_stats_host(payload(name)[at:at + n])


def test_stats_count_what_they_say():
    s = _core.gzip_chunk_stats_host(b"abcdefgh" + bytes(600) + b"abcdefgh")
    # a..h, one zero, 258 + 258 + 83 zeros at distance 1, abcdefgh from 608 back
    assert (s["tokens"], s["matches"], s["len258"], s["max_dist"]) == (13, 4, 2, 608)
    assert s["max_dist_code"] == 18 and not s["stored"] and s["trees_ok"]
    assert (s["used_ll"], s["used_d"], s["nd"]) == (13, 2, 19)
    assert set(s["builder_steps"]) == set(s["builder_shrink_steps"]) == {"ll", "d", "cl"}
    assert s["builder_steps_max"] == max(s["builder_steps"].values())
    with pytest.raises(ValueError):
        _core.gzip_chunk_stats_host(b"")
    with pytest.raises(ValueError):
        _core.gzip_chunk_stats_host(bytes(C + 1))


@pytest.mark.parametrize("offset", OFFSETS)
def test_maxdist_reaches_the_largest_distance(offset):
    s = stats("maxdist", offset, 0)
    assert s["max_dist"] == C - 4 == 32764 and s["max_dist_code"] == 29
    assert not s["stored"] and s["nd"] == 30 and s["used_d"] == 2
    # the next chunk starts inside the motif and may not look back
    assert stats("maxdist", offset, 1)["max_dist"] == 1


@pytest.mark.parametrize("offset", OFFSETS)
def test_a_repeat_in_the_next_chunk_is_no_match(offset):
    """Nothing but the zero run matches: the motif's repeat is C away, past the
    chunk's end, and the chunk that holds it starts with an empty table."""
    for chunk in (0, 1):
        s = stats("maxdist_next", offset, chunk)
        assert s["matches"] > 100 and s["max_dist"] == 1 and s["used_d"] == 1


@pytest.mark.parametrize("offset", OFFSETS)
def test_longcodes_reach_the_length_limit(offset):
    """max_d_len: a distance code of L bits needs a symbol with less than
    2^-(L-1) of the matches (the builder starts from ceil(log2(total / count))
    and only ever shortens below the limit), and a 32 KiB chunk has at most
    8192 matches of four bytes, so 13 bits is the most this parse can give and
    14 cannot occur. This payload reaches 13 from one source phase and 11 to
    12 from the others."""
    s = stats("longcodes", offset, 0)
    assert s["max_ll_len"] == 15 and not s["stored"]
    assert s["tokens"] > 32000 and s["builder_steps"]["ll"] > 17  # 17: the old corpus's most
    s = stats("longcodes", offset, 1)
    assert s["max_d_len"] >= {0: 12, 1: 13, 5: 12, 15: 11}[offset]
    assert not s["stored"] and s["matches"] > 4096


def test_widetokens_reach_the_third_word():
    """The corpus before this family: widest token 40 bits, 6 third-word tokens
    in all of it. Here 44 bits in one chunk and 7 third-word tokens in another,
    every one with bits set in that word (a third word of zeros tests nothing)
    (46 bits is the most the parse allows: 15 + 5 and 13 + 13, see above)."""
    s = stats("widetokens", 0, 0)
    assert s["three_word_nonzero"] >= 7 and s["max_token_bits"] >= 37 and not s["stored"]
    s = stats("widetokens", 0, 1)
    assert s["max_token_bits"] >= 44 and s["three_word_nonzero"] >= 2 and not s["stored"]
    for offset in OFFSETS:  # every source phase of the GPU test meets the third word
        assert stats("widetokens", offset, 0)["three_word_nonzero"] >= 5
        assert stats("widetokens", offset, 1)["max_token_bits"] >= 44


@pytest.mark.parametrize("name", ["onesymbol", "twosymbols"])
def test_few_symbols_trim_the_header(name):
    for n in (1, 3):  # nothing can match: no distance is used, the filler code is declared
        s = stats(name, 0, 0, n)
        assert (s["matches"], s["used_d"], s["nd"], s["nll"]) == (0, 0, 1, 257)
        assert s["used_ll"] == (2 if name == "onesymbol" or n == 1 else 3) and s["trees_ok"]
    for n in (258, 259, C):  # the whole chunk is one run
        s = stats(name, 0, 0, n)
        period = 1 if name == "onesymbol" else 2
        # literals: the first round of the alternation (it looks up before it
        # inserts), and a tail too short to match
        assert s["tokens"] - s["matches"] <= (1 if period == 1 else 64) + 3
        assert s["matches"] >= 1 and not s["stored"]
        if period == 1:  # one used distance symbol: the one-bit code, no Kraft step
            assert (s["max_dist"], s["used_d"], s["nd"], s["builder_steps"]["d"]) == (1, 1, 1, 0)
        else:  # a round sees the table of the rounds before it: 2, 4, ... up to a round back
            assert s["max_dist"] % 2 == 0 and s["max_dist"] <= 64


# ------------------------------------------------- the builder on histograms --

def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def random_hist(r, nsym):
    """2..nsym used symbols, a total up to 32769, from flat to very skewed."""
    used = r.randrange(2, nsym + 1)
    total = r.randrange(used, 32770)
    power = r.choice([0.0, 1.0, 3.0, 8.0])
    w = [r.random() ** power + 1e-9 for _ in range(used)]
    scale = (total - used) / sum(w)
    counts = [1 + int(x * scale) for x in w]
    hist = counts + [0] * (nsym - used)
    r.shuffle(hist)
    return hist


@functools.lru_cache(maxsize=None)
def histograms():
    """(id, counts, maxbits, complete) of every builder case, host and GPU."""
    out = [("shrink", [67, 67, 67, 34, 22] + [1] * 11 + [0] * 3, 7, True),
           ("fib21-15", fib(21) + [0] * 265, 15, True),
           ("fib24-15", fib(24) + [0] * 6, 15, False),  # total 75024 > 2^15: the clip
           ("fib19-7", fib(19), 7, True),
           ("two", [0, 5, 0, 9] + [0] * 26, 15, False),
           ("two-7", [1, 32768] + [0] * 17, 7, True),
           ("one-complete", [0, 0, 7] + [0] * 283, 15, True),
           ("one-at-zero", [7] + [0] * 18, 7, True),
           ("one-incomplete", [0, 0, 7] + [0] * 27, 15, False),
           ("none-complete", [0] * 286, 15, True),
           ("none-incomplete", [0] * 30, 15, False)]
    for n in range(2, 287):
        out.append(("ones-%d" % n, [1] * n, 15, True))
        if n <= 19:
            out.append(("ones-%d-7" % n, [1] * n, 7, True))
    for k in range(1, 286):
        out.append(("big-%d" % k, [32768] + [1] * k + [0] * (285 - k), 15, True))
    # Kraft sum above one: `big` counts of total/2, total/4, ... are exact, and
    # more rare symbols than the rest has room for are clipped to the limit
    for tid, total, big, rare, nsym, maxbits in (("7", 4096, 4, range(9, 16), 19, 7),
                                                 ("15", 65536, 8, range(140, 271, 10), 286, 15),
                                                 ("d", 65536, 11, range(17, 20), 30, 15)):
        for u in rare:
            left = total >> big
            small = [left // u + (i < left % u) for i in range(u)]
            hist = [total >> j for j in range(1, big + 1)] + small
            out.append(("tight-%s-%d" % (tid, u), hist + [0] * (nsym - len(hist)), maxbits,
                        nsym != 30))
    r = random.Random(1951)
    for nsym, maxbits, complete in ((286, 15, True), (30, 15, False), (19, 7, True)):
        for i in range(300):
            out.append(("random-%d-%d" % (nsym, i), random_hist(r, nsym), maxbits, complete))
    return out


def package_merge(counts, maxbits):
    """Optimal code lengths of at most `maxbits` for the non-zero counts
    (Larmore and Hirschberg's package-merge, in its plainest form)."""
    leaves = sorted((c, (s,)) for s, c in enumerate(counts) if c)
    assert 2 <= len(leaves) <= 1 << maxbits
    level = leaves
    for _ in range(maxbits - 1):
        pairs = [(level[i][0] + level[i + 1][0], level[i][1] + level[i + 1][1])
                 for i in range(0, len(level) - 1, 2)]
        level = sorted(leaves + pairs, key=lambda x: x[0])
    lens = [0] * len(counts)
    for _, syms in level[:2 * len(leaves) - 2]:
        for s in syms:
            lens[s] += 1
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2: symbol -> (code, MSB first), written independently of
    assign_codes."""
    code, codes = 0, {}
    for bits in range(1, 16):
        for s, l in enumerate(lens):
            if l == bits:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, nb):  # LSB first, as header fields go
        self.acc |= v << self.n
        self.n += nb

    def code(self, v, nb):  # Huffman codes go MSB first
        self.put(int(format(v, "0%db" % nb)[::-1], 2), nb)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def inflate_with(lens):
    """One final dynamic block whose lit/len code is `lens` (as many as 286),
    moved so that a coded symbol is the end-of-block: every coded literal once,
    then the end. zlib accepts the code only if it is neither over-subscribed
    nor incomplete (but for a single one-bit code), and must give the literals
    back. Code lengths travel one by one through a flat 4-bit code."""
    ll = list(lens) + [0] * (286 - len(lens))
    if not ll[256]:
        s = max(range(286), key=lambda i: ll[i] > 0)  # the first coded symbol
        ll[s], ll[256] = ll[256], ll[s]
    codes = canonical_codes(ll)
    w = BitWriter()
    w.put(1, 1), w.put(2, 2), w.put(286 - 257, 5), w.put(0, 5), w.put(19 - 4, 4)
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        w.put(4 if sym < 16 else 0, 3)
    for l in ll + [1]:  # and one distance code of one bit
        w.code(l, 4)  # flat code: the code of length l is l
    literals = [s for s in range(256) if ll[s]]
    for s in literals + [256]:
        w.code(codes[s], ll[s])
    assert zlib.decompress(w.bytes(), -15) == bytes(literals)


def check_lengths(hist, maxbits, complete, ok, lens):
    assert ok and len(lens) == len(hist)
    used = [s for s, c in enumerate(hist) if c]
    kraft = sum(1 << (maxbits - l) for l in lens if l)
    assert max(lens) <= maxbits
    if len(used) >= 2:
        assert kraft == 1 << maxbits
        assert all((l > 0) == (c > 0) for l, c in zip(lens, hist))
    else:  # the documented fillers: one bit on the used symbol (or symbol 0) ...
        one = used[0] if used else 0
        want = [0] * len(hist)
        want[one] = 1
        if complete:  # ... and the other one-bit code on an unused symbol
            want[0 if one else 1] = 1
        assert lens == want
    inflate_with(lens)


# Worst total cost of the builder over package-merge's optimum on histograms():
# the figure of profiles/deflate_kernel.md, a regression guard and not a claim
# about the method.
WORST_COST_RATIO = 1.157143  # "ones-17": 17 equal counts, 81 bits against 70


def test_builder_on_histograms():
    worst, worst_id = 1.0, None
    for hid, hist, maxbits, complete in histograms():
        ok, lens, steps = _core.deflate_code_lengths_host(hist, maxbits, complete)
        check_lengths(hist, maxbits, complete, ok, lens)
        assert steps["steps"] <= 16 * len(hist)
        if sum(1 for c in hist if c) >= 2:
            best = package_merge(hist, maxbits)
            assert sum(1 << (maxbits - l) for l in best if l) == 1 << maxbits
            ratio = (sum(c * l for c, l in zip(hist, lens)) /
                     sum(c * l for c, l in zip(hist, best)))
            assert ratio >= 1.0, hid  # nothing beats the optimum: the reference holds
            if ratio > worst:
                worst, worst_id = ratio, hid
    print("worst cost ratio %.6f at %s" % (worst, worst_id))
    assert worst <= WORST_COST_RATIO * 1.01


def test_builder_takes_the_shrink_branch():
    hist = [67, 67, 67, 34, 22] + [1] * 11 + [0] * 3
    ok, lens, steps = _core.deflate_code_lengths_host(hist, 7, True)
    assert ok and lens == [2, 2, 2, 3, 5] + [7] * 10 + [6] + [0] * 3
    assert steps == {"steps": 2, "shrink": 1}
    shrinks = sum(_core.deflate_code_lengths_host(h, m, c)[2]["shrink"] > 0
                  for _, h, m, c in histograms())
    assert shrinks >= 10  # the clipped random histograms reach it too


@pytest.mark.parametrize("hist, maxbits", [([1], 15), ([1] * 287, 15), ([1, 1], 0), ([1, 1], 16),
                                           ([65536, 1], 15)])
def test_builder_refuses_what_it_cannot_hold(hist, maxbits):
    with pytest.raises(ValueError):
        _core.deflate_code_lengths_host(hist, maxbits, True)


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
