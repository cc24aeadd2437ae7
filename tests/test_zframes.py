"""The foreign-frame corpus (util_zframes.py) on the CPU: it reaches every
decoder construct it is there for, libzstd agrees with it, and the CPU
decoder reads it through the seek-table path. The device half is
test_gpu_zstd_interop.py."""
import pytest

# torch before the extension (docs/engineering-notes.md #16): this module
# runs in the same process as the GPU modules
torch = pytest.importorskip("torch")
_core = pytest.importorskip("modelx_amd._core")

import util_seek  # noqa: E402
import util_zframes as uz  # noqa: E402


def _id(it):
    return "%s-%s" % (it.name, it.variant)


def test_corpus_reaches_every_required_construct():
    cov = uz.coverage()
    print("libzstd", uz.libzstd_version(), "constructs:",
          ", ".join("%s=%d" % kv for kv in sorted(cov.items())))
    missing = [name for name in uz.REQUIRED if cov[name] == 0]
    assert not missing, "libzstd %s emitted no %s" % (uz.libzstd_version(), missing)


def test_walker_reads_our_own_dialect():
    # the walker against frames whose make-up is known from the encoder:
    # single-segment, no checksum, one block per 128 KiB, predefined tables
    data = uz.payloads()["text"]
    blob = _core.zstd_compress_cpu(data, 128 << 10)
    total = uz.collections.Counter()
    for c_off, c_size, _, _ in _core.zstd_seek_table(blob):
        total += uz.walk(blob[c_off:c_off + c_size])
    assert total["hdr:single-segment"] == 3 and total["hdr:checksum"] == 0
    assert total["block:compressed"] == 3 and total["frame:>=4-blocks"] == 0
    assert total["ll:predefined"] == total["of:predefined"] == total["ml:predefined"] == 3
    assert not [k for k in total if k.endswith((":fse", ":repeat", ":rle"))]


def test_walker_rejects_a_cut_frame():
    frame = uz.compress(uz.payloads()["shrdlu-900"], 3)
    with pytest.raises((AssertionError, IndexError)):
        uz.walk(frame[:-1])
    with pytest.raises(AssertionError):
        uz.walk(frame + b"\0")


def test_libzstd_decodes_every_frame():
    for it in uz.corpus():
        assert uz.decompress(it.frame, len(it.payload)) == it.payload, _id(it)


def test_empty_frames_sit_between_non_empty_ones():
    items = uz.corpus()
    empties = [i for i, it in enumerate(items) if not it.payload]
    assert len(empties) == len(uz.LEVELS)
    for i in empties:
        assert 0 < i < len(items) - 1 and items[i - 1].payload and items[i + 1].payload


def test_seek_table_of_wrapped_frames_tiles():
    items = uz.corpus()
    frames = [it.frame for it in items]
    sizes = [len(it.payload) for it in items]
    blob, _ = uz.corpus_blob()
    assert _core.zstd_seek_table(blob) == uz.tiling(frames, sizes)
    assert _core.zstd_frames(blob) == uz.tiling(frames, sizes)
    wide = util_seek.with_checksum_flag(blob)
    assert len(wide) == len(blob) + 4 * len(items)
    assert _core.zstd_seek_table(wide) == uz.tiling(frames, sizes)
    # one frame and no frame at all
    one = uz.wrap_seekable(frames[:1], sizes[:1])
    assert _core.zstd_seek_table(one) == [(0, len(frames[0]), 0, sizes[0])]
    assert _core.zstd_seek_table(uz.wrap_seekable([], [])) == []


def test_cpu_decoder_through_the_seek_table():
    blob, payload = uz.corpus_blob()
    assert _core.zstd_content_size(blob) == len(payload)
    assert _core.zstd_decompress_cpu(blob) == payload
    assert _core.zstd_decompress_cpu(util_seek.with_checksum_flag(blob)) == payload


@pytest.mark.parametrize("index", range(len(uz.corpus_keys())),
                         ids=["%s-%s" % k for k in uz.corpus_keys()])
def test_cpu_decoder_per_frame(index):
    # one blob per frame, so a failure names the payload and the variant
    it = uz.corpus()[index]
    assert (it.name, it.variant) == uz.corpus_keys()[index]
    blob = uz.wrap_seekable([it.frame], [len(it.payload)])
    assert _core.zstd_decompress_cpu(blob) == it.payload


def test_cpu_decoder_refuses_a_lying_d_size():
    # frame 1 understated by one and frame 2 overstated by one: the envelope,
    # the c_size sum and the total all stay valid, the frames do not fit
    items = [it for it in uz.corpus() if it.variant == "L3"
             and it.name in ("shrdlu-900", "aab", "random-63")]
    assert len(items) == 3
    frames = [it.frame for it in items]
    sizes = [len(it.payload) for it in items]
    good = uz.wrap_seekable(frames, sizes)
    assert _core.zstd_decompress_cpu(good) == b"".join(it.payload for it in items)
    bad = uz.wrap_seekable(frames, [sizes[0], sizes[1] - 1, sizes[2] + 1])
    assert [e[3] for e in _core.zstd_seek_table(bad)] == [sizes[0], sizes[1] - 1, sizes[2] + 1]
    with pytest.raises(RuntimeError):
        _core.zstd_decompress_cpu(bad)
