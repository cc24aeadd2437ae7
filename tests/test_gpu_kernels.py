"""GPU numerics + engine tests (run on MI355X via gpurun).

Kernel results are compared against plain CPU references (hashlib) —
SURVEY.md §4 kernel-unit strategy."""
import hashlib
import os

import pytest

torch = pytest.importorskip("torch")

from modelx_amd.wire import digest as dg

pytestmark = pytest.mark.gpu


def _engine(device=0):
    from modelx_amd import _core

    assert _core.hip_available(), "native extension loaded but no HIP device"
    return _core.GpuEngine(device=device, num_slots=8, slot_bytes=32 << 20, num_streams=4)


@pytest.fixture(scope="module")
def engine():
    return _engine()


class TestSha256Kernels:
    @pytest.mark.parametrize("size", [1, 55, 56, 63, 64, 65, 127, 128, 1000,
                                      (1 << 20) - 1, 1 << 20, (1 << 20) + 1,
                                      (5 << 20) + 12345])
    def test_chunk_leaves_match_hashlib(self, engine, size):
        data = torch.randint(0, 256, (size,), dtype=torch.uint8)
        dev = data.cuda()
        cs = 1 << 20
        leaves = engine.sha256_chunk_leaves(dev.data_ptr(), size, cs)
        raw = data.numpy().tobytes()
        expect = b"".join(
            hashlib.sha256(raw[o : o + cs]).digest() for o in range(0, size, cs)
        )
        assert leaves == expect

    def test_chunk_leaves_small_chunksize(self, engine):
        # many chunks per block → exercises multi-block grids
        size = 256 * 1024 + 7
        cs = 4096
        data = torch.randint(0, 256, (size,), dtype=torch.uint8)
        dev = data.cuda()
        leaves = engine.sha256_chunk_leaves(dev.data_ptr(), size, cs)
        raw = data.numpy().tobytes()
        expect = b"".join(hashlib.sha256(raw[o : o + cs]).digest() for o in range(0, size, cs))
        assert leaves == expect

    def test_root_matches_python_reference(self, engine):
        size = (3 << 20) + 17
        cs = 1 << 20
        data = torch.randint(0, 256, (size,), dtype=torch.uint8)
        dev = data.cuda()
        leaves = engine.sha256_chunk_leaves(dev.data_ptr(), size, cs)
        got = dg.root_from_leaf_bytes(leaves, cs, size)
        assert got == dg.chunked_digest(data.numpy().tobytes(), cs)

    def test_multibuf_canonical_sha256(self, engine):
        bufs = []
        raws = []
        for size in [1, 100, 4096, 1 << 18, (1 << 20) + 3]:
            t = torch.randint(0, 256, (size,), dtype=torch.uint8)
            raws.append(t.numpy().tobytes())
            bufs.append(t.cuda())
        digests = engine.sha256_multibuf([(t.data_ptr(), t.numel()) for t in bufs])
        for i, raw in enumerate(raws):
            assert digests[i * 32 : (i + 1) * 32] == hashlib.sha256(raw).digest()

    # The kernels load 16 bytes at a time only from a 16-byte-aligned chunk;
    # any other base or chunk size takes the exact-width branch. A view may
    # start at any byte of an allocation and a chunk size may be any integer.
    UNALIGNED_SIZE = 200 * 1024 + 37  # 37-byte tail behind the last 64 B block

    @pytest.fixture(scope="class")
    def unaligned(self):
        """(host bytes, device tensor) shared by the unaligned cases."""
        g = torch.Generator().manual_seed(11)
        data = torch.randint(0, 256, (self.UNALIGNED_SIZE + 16,), dtype=torch.uint8,
                             generator=g)
        dev = data.cuda()
        torch.cuda.synchronize()
        return data.numpy().tobytes(), dev

    @pytest.mark.parametrize("cs", [64, 65, 1000, 4100, 65536])
    def test_chunk_leaves_any_base_phase(self, engine, unaligned, cs):
        raw, dev = unaligned
        size = self.UNALIGNED_SIZE
        expect = [b"".join(dg.chunk_leaves(raw[off : off + size], cs)) for off in range(16)]
        for off in range(16):
            got = engine.sha256_chunk_leaves(dev.data_ptr() + off, size, cs)
            assert got == expect[off], f"base phase {off}"
        many = engine.sha256_chunk_leaves_many(
            [(dev.data_ptr() + off, size, cs) for off in range(16)])
        for off in range(16):
            assert many[off] == expect[off], f"base phase {off} (batched)"

    def test_leaves_many_mixed_buffers(self, engine, unaligned):
        """One batched call over different chunk sizes and base phases, with
        an empty buffer in the middle and another one last; more than 256
        chunks, so the per-lane buffer search crosses a workgroup."""
        raw, dev = unaligned
        shapes = [(0, 70000, 1000), (3, 4100, 4100), (7, 0, 64), (1, 20000, 65),
                  (16, 64, 64), (9, 100000, 65536), (5, 12345, 4096), (2, 0, 1000)]
        assert sum(max(1, -(-size // cs)) for _, size, cs in shapes) > 256
        got = engine.sha256_chunk_leaves_many(
            [(dev.data_ptr() + off, size, cs) for off, size, cs in shapes])
        assert len(got) == len(shapes)
        for (off, size, cs), leaves in zip(shapes, got):
            assert leaves == b"".join(dg.chunk_leaves(raw[off : off + size], cs)), \
                (off, size, cs)

    def test_multibuf_any_base_phase(self, engine, unaligned):
        raw, dev = unaligned
        lengths = [0, 55, 56, 64, 119, 120, 4099]
        cases = [(off, n) for off in range(16) for n in lengths]
        # other content per buffer: each starts `stride` (a multiple of 16,
        # so `off` stays the base phase) after the last
        stride = 1616
        bufs = [(dev.data_ptr() + k * stride + off, n) for k, (off, n) in enumerate(cases)]
        assert (len(cases) - 1) * stride + 15 + 4099 <= self.UNALIGNED_SIZE
        digests = engine.sha256_multibuf(bufs)
        for k, (off, n) in enumerate(cases):
            start = k * stride + off
            assert digests[k * 32 : (k + 1) * 32] == \
                hashlib.sha256(raw[start : start + n]).digest(), (off, n)


class TestEngineTransfers:
    @pytest.fixture(scope="class")
    def stack(self, tmp_path_factory):
        from util_servers import start_modelxd_s3, start_s3d

        s3_root = tmp_path_factory.mktemp("s3-gpu")
        s3d = start_s3d(str(s3_root))
        mdx = start_modelxd_s3(s3d.url, redirect=True)
        yield mdx, s3d
        mdx.stop()
        s3d.stop()

    def test_pull_to_device_lands_exact_bytes(self, engine, stack, tmp_path):
        from modelx_amd.client import Client
        from modelx_amd.client.extension import ContentSource, get as get_ext
        from modelx_amd.client.push import parse_manifest
        from modelx_amd.config import ModelConfig

        mdx, _ = stack
        d = tmp_path / "m"
        d.mkdir()
        (d / "modelx.yaml").write_text(ModelConfig(description="gpu").to_yaml())
        payload = os.urandom(48 * 1024 * 1024 + 12345)
        (d / "weights.bin").write_bytes(payload)
        c = Client(mdx.url)
        c.push("gpu/pull", "v1", str(d), quiet=True)

        from modelx_amd.client.gpu import GpuClient

        g = GpuClient(mdx.url, device=0)
        tensors = g.pull_to_gpu("gpu/pull", "v1")  # digest-verified on GPU
        got = tensors["weights.bin"].cpu().numpy().tobytes()
        assert got == payload

    def test_pull_detects_corruption(self, engine, stack, tmp_path):
        from modelx_amd.client import Client
        from modelx_amd.config import ModelConfig
        from modelx_amd.wire import errors as er
        from modelx_amd.wire import paths as pm

        mdx, s3d = stack
        d = tmp_path / "mc"
        d.mkdir()
        (d / "modelx.yaml").write_text(ModelConfig(description="corrupt").to_yaml())
        (d / "weights.bin").write_bytes(os.urandom(8 * 1024 * 1024))
        c = Client(mdx.url)
        manifest = c.push("gpu/corrupt", "v1", str(d), quiet=True)
        blob = next(b for b in manifest.blobs if b.name == "weights.bin")
        # flip one byte in the stored object
        root = s3d.proc.args[s3d.proc.args.index("--root") + 1]
        obj = os.path.join(root, "modelx", "registry",
                           pm.blob_digest_path("gpu/corrupt", blob.digest))
        with open(obj, "r+b") as f:
            f.seek(4 * 1024 * 1024)
            b0 = f.read(1)
            f.seek(4 * 1024 * 1024)
            f.write(bytes([b0[0] ^ 1]))
        from modelx_amd.client.gpu import GpuClient

        g = GpuClient(mdx.url, device=0)
        with pytest.raises(er.ModelxError) as exc:
            g.pull_to_gpu("gpu/corrupt", "v1")
        assert exc.value.code == er.ErrCode.DIGEST_INVALID

    def test_push_from_gpu_roundtrip(self, engine, stack):
        from modelx_amd.client.gpu import GpuClient

        mdx, _ = stack
        g = GpuClient(mdx.url, device=0)
        src = torch.randint(0, 256, (24 * 1024 * 1024 + 999,), dtype=torch.uint8,
                            device="cuda:0")
        manifest = g.push_from_gpu("gpu/pushed", "v1", {"w.bin": src},
                                   part_bytes=8 << 20)
        blob = next(b for b in manifest.blobs if b.name == "w.bin")
        assert blob.digest.startswith("sha256c")
        back = g.pull_to_gpu("gpu/pushed", "v1")
        assert torch.equal(back["w.bin"], src)

    def test_push_dedup_skips_existing(self, engine, stack):
        from modelx_amd.client.gpu import GpuClient

        mdx, _ = stack
        g = GpuClient(mdx.url, device=0)
        src = torch.randint(0, 256, (1 << 20,), dtype=torch.uint8, device="cuda:0")
        g.push_from_gpu("gpu/dedup", "v1", {"a.bin": src})
        # same content again: HEAD-dedup path (no error, blob reused)
        g.push_from_gpu("gpu/dedup", "v2", {"a.bin": src})
        m = g.remote.get_manifest("gpu/dedup", "v2")
        assert m.blobs[0].size == 1 << 20


class TestZstdKernels:
    """GPU zstd kernels (core/hip/zstd.hip) vs the CPU path of the SAME
    shared codec core; libzstd decodes what the compress kernel wrote. The
    libzstd interop oracle for the decoder (frames libzstd wrote) is
    test_gpu_zstd_interop.py."""

    def _payloads(self):
        import random

        rng = random.Random(77)
        reps = bytearray()
        while len(reps) < 3_000_000:
            if rng.random() < 0.6 and len(reps) > 64:
                off = rng.randrange(1, min(len(reps), 100_000))
                ln = rng.randrange(4, 400)
                start = len(reps) - off
                for k in range(ln):
                    reps.append(reps[start + k])
            else:
                reps.extend(rng.randbytes(rng.randrange(1, 60)))
        return {
            "text": b"the quick brown fox jumps over the lazy dog " * 60_000,
            "random": rng.randbytes(2_000_000),
            "zeros": bytes(1_500_000),
            "repeats": bytes(reps),
            "tiny": b"x",
        }

    def test_compress_device_roundtrip(self, engine):
        from modelx_amd import _core

        for name, data in self._payloads().items():
            src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            bound = _core.zstd_compress_bound(len(data))
            dst = torch.empty(bound, dtype=torch.uint8, device="cuda")
            n = engine.zstd_compress_device(src.data_ptr(), len(data), 128 << 10,
                                            dst.data_ptr(), bound)
            blob = bytes(dst[:n].cpu().numpy().tobytes())
            # CPU decode of the GPU-compressed blob
            assert _core.zstd_decompress_cpu(blob) == data, name
            # libzstd decodes it too (standard frames)
            import ctypes

            z = ctypes.CDLL("libzstd.so.1")
            z.ZSTD_decompress.restype = ctypes.c_size_t
            z.ZSTD_isError.restype = ctypes.c_uint
            out = ctypes.create_string_buffer(max(len(data), 1))
            m = z.ZSTD_decompress(out, len(data), blob, len(blob))
            assert not z.ZSTD_isError(m) and out.raw[:m] == data, name

    def test_decompress_device_of_cpu_blob(self, engine):
        from modelx_amd import _core

        for name, data in self._payloads().items():
            blob = _core.zstd_compress_cpu(data, 128 << 10)
            src = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
            dst = torch.empty(max(len(data), 1), dtype=torch.uint8, device="cuda")
            n = engine.zstd_decompress_device(src.data_ptr(), len(blob),
                                              dst.data_ptr(), dst.numel())
            assert n == len(data), name
            assert bytes(dst[:n].cpu().numpy().tobytes()) == data, name

    def test_gpu_compress_gpu_decompress(self, engine):
        from modelx_amd import _core

        data = b"modelx gpu roundtrip " * 500_000  # ~10 MiB compressible
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        bound = _core.zstd_compress_bound(len(data))
        comp = torch.empty(bound, dtype=torch.uint8, device="cuda")
        n = engine.zstd_compress_device(src.data_ptr(), len(data), 128 << 10,
                                        comp.data_ptr(), bound)
        assert n < len(data) // 10
        back = torch.empty(len(data), dtype=torch.uint8, device="cuda")
        m = engine.zstd_decompress_device(comp.data_ptr(), n, back.data_ptr(), len(data))
        assert m == len(data)
        assert torch.equal(back, src)

    def test_corrupt_seek_table_rejected_on_host(self, engine):
        """A damaged blob tail is refused by the host-side seek-table
        validation of both device entry points — before any decode kernel
        is launched — and the engine's scratch and locks survive the
        throws: the same engine still decodes the good blob."""
        import util_seek

        data, blob = util_seek.three_frame_blob()
        good = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        dst = [torch.empty(len(data), dtype=torch.uint8, device="cuda") for _ in range(3)]
        for name, bad_bytes in util_seek.corruptions(blob).items():
            bad = torch.frombuffer(bytearray(bad_bytes), dtype=torch.uint8).cuda()
            with pytest.raises(RuntimeError):
                engine.zstd_decompress_device(bad.data_ptr(), len(bad_bytes),
                                              dst[0].data_ptr(), len(data))
            with pytest.raises(RuntimeError):
                engine.zstd_decompress_many(
                    [(good.data_ptr(), len(blob), dst[0].data_ptr(), len(data)),
                     (bad.data_ptr(), len(bad_bytes), dst[1].data_ptr(), len(data)),
                     (good.data_ptr(), len(blob), dst[2].data_ptr(), len(data))])
        for d in dst:
            d.zero_()
        torch.cuda.synchronize()
        n = engine.zstd_decompress_device(good.data_ptr(), len(blob),
                                          dst[0].data_ptr(), len(data))
        sizes = engine.zstd_decompress_many(
            [(good.data_ptr(), len(blob), d.data_ptr(), len(data)) for d in dst[1:]])
        assert n == len(data) and sizes == [len(data)] * 2
        for d in dst:
            assert bytes(d.cpu().numpy().tobytes()) == data


class TestZstdGpuClient:
    def test_push_pull_compressed(self, tmp_path):
        from util_servers import start_modelxd_s3, start_s3d

        from modelx_amd.client.gpu import GpuClient

        s3d = start_s3d(str(tmp_path / "s3"))
        mdx = start_modelxd_s3(s3d.url, redirect=True)
        try:
            g = GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20)
            data = (b"w" * 1000 + os.urandom(24)) * 4096  # compressible, 4 MiB
            src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            manifest = g.push_from_gpu("gpu/zstd", "v1", {"weights.bin": src},
                                       compress="zstd")
            (desc,) = [b for b in manifest.blobs if b.name == "weights.bin"]
            from modelx_amd.wire import types as t

            assert desc.media_type == t.MEDIA_TYPE_MODEL_FILE_ZSTD
            assert desc.size < len(data) // 2
            back = g.pull_to_gpu("gpu/zstd", "v1")
            assert torch.equal(back["weights.bin"], src)
        finally:
            mdx.stop()
            s3d.stop()


class TestChunkDedup:
    def test_second_pull_dedups(self, tmp_path):
        """Pulling content whose chunks are already HBM-resident must gather
        D2D instead of re-fetching (config-5 dedup semantics)."""
        from util_servers import start_modelxd_s3, start_s3d

        from modelx_amd.client.gpu import GpuClient

        s3d = start_s3d(str(tmp_path / "s3"))
        mdx = start_modelxd_s3(s3d.url, redirect=True)
        try:
            g = GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20, dedup=True)
            base = torch.randint(0, 256, (4 << 20,), dtype=torch.uint8, device="cuda")
            g.push_from_gpu("gpu/dedup", "v1", {"a.bin": base})
            # v2 = same chunks under another name + a fresh tail
            tail = torch.randint(0, 256, (256 << 10,), dtype=torch.uint8, device="cuda")
            v2 = torch.cat([base, tail])
            g.push_from_gpu("gpu/dedup", "v2", {"b.bin": v2})
            g.clear_chunk_index()

            first = g.pull_to_gpu("gpu/dedup", "v1")
            assert torch.equal(first["a.bin"], base)
            stats_before = len(g.last_stats)
            second = g.pull_to_gpu("gpu/dedup", "v2")
            assert torch.equal(second["b.bin"], v2)
            dd = [s for s in g.last_stats[stats_before:] if s.get("phase") == "pull-dedup"]
            assert dd, "dedup path not taken"
            # all of v1's chunks must have been gathered, only the tail fetched
            assert dd[0]["dedup_bytes"] >= base.numel()
            assert dd[0]["bytes"] <= tail.numel() + (128 << 10)
        finally:
            mdx.stop()
            s3d.stop()


class TestZstdCrossPath:
    """GPU-pushed +zstd blobs pulled by the CPU client and vice versa —
    the format is one (seekable multi-frame zstd), whichever side codes."""

    def test_gpu_push_cpu_pull(self, tmp_path):
        from util_servers import start_modelxd_s3, start_s3d

        from modelx_amd.client import Client
        from modelx_amd.client.gpu import GpuClient

        s3d = start_s3d(str(tmp_path / "s3"))
        mdx = start_modelxd_s3(s3d.url, redirect=True)
        try:
            g = GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20)
            data = (b"interop " * 8192 + os.urandom(1024)) * 64  # ~4 MiB
            src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            g.push_from_gpu("xp/gpu2cpu", "v1", {"weights.bin": src}, compress="zstd")
            c = Client(mdx.url)
            out = tmp_path / "out"
            c.pull("xp/gpu2cpu", "v1", str(out), quiet=True)
            assert (out / "weights.bin").read_bytes() == data
        finally:
            mdx.stop()
            s3d.stop()

    def test_cpu_push_gpu_pull(self, tmp_path):
        from util_servers import start_modelxd_s3, start_s3d

        from modelx_amd.client import Client
        from modelx_amd.client.gpu import GpuClient
        from modelx_amd.config import ModelConfig

        s3d = start_s3d(str(tmp_path / "s3"))
        mdx = start_modelxd_s3(s3d.url, redirect=True)
        try:
            d = tmp_path / "model"
            d.mkdir()
            (d / "modelx.yaml").write_text(ModelConfig(description="xp").to_yaml())
            data = (b"cpu-coded " * 6553 + os.urandom(512)) * 48  # ~3 MiB
            (d / "weights.bin").write_bytes(data)
            Client(mdx.url).push("xp/cpu2gpu", "v1", str(d), quiet=True, compress="zstd")
            g = GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20)
            out = g.pull_to_gpu("xp/cpu2gpu", "v1")
            assert bytes(out["weights.bin"].cpu().numpy().tobytes()) == data
        finally:
            mdx.stop()
            s3d.stop()


class TestCanonicalDigest:
    """Wire-canonical sha256 on the GPU data path (reference
    push.go:149-161 semantics): D2H through the pinned ring onto the CPU's
    SHA-NI units (engine.sha256_canonical_device)."""

    @pytest.mark.parametrize("size", [0, 1, 63, 64, 65, 4096,
                                      (32 << 20) - 1, 32 << 20, (32 << 20) + 1,
                                      (70 << 20) + 12345])
    def test_canonical_device_matches_hashlib(self, engine, size):
        data = torch.randint(0, 256, (max(size, 1),), dtype=torch.uint8)[:size]
        dev = data.cuda()
        got = engine.sha256_canonical_device(dev.data_ptr(), size)
        assert got == hashlib.sha256(data.numpy().tobytes()).digest()

    def test_canonical_push_verified_by_cpu_client(self, tmp_path):
        """A digest_mode="sha256" GPU push round-trips through the CPU pull
        engine, which digest-verifies the blob from the MAIN descriptor
        digest alone — zero chunk annotations consumed (wire interop with a
        stock Go modelx client)."""
        from util_servers import start_modelxd_s3, start_s3d

        from modelx_amd.client.gpu import GpuClient
        from modelx_amd.client.pull import Puller, _verify_digest_of_file
        from modelx_amd.client.registry import RegistryClient
        from modelx_amd.wire import types as t

        s3d = start_s3d(str(tmp_path / "s3"))
        mdx = start_modelxd_s3(s3d.url, redirect=True)
        try:
            g = GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20)
            src = torch.randint(0, 256, ((12 << 20) + 777,), dtype=torch.uint8,
                                device="cuda:0")
            manifest = g.push_from_gpu("gpu/canon", "v1", {"w.bin": src},
                                       digest_mode="sha256")
            blob = next(b for b in manifest.blobs if b.name == "w.bin")
            assert blob.digest.startswith("sha256:")
            # the main digest IS the canonical hash of the bytes
            assert blob.digest == "sha256:" + hashlib.sha256(
                src.cpu().numpy().tobytes()).hexdigest()

            # CPU client pulls and verifies from desc.digest alone: strip
            # the chunk annotations to prove nothing else is consumed
            stripped = RegistryClient(mdx.url).get_manifest("gpu/canon", "v1")
            for b in stripped.blobs:
                b.annotations = {}
            dest = tmp_path / "out"
            p = Puller(RegistryClient(mdx.url))
            wb = next(b for b in stripped.blobs if b.name == "w.bin")
            p.pull_blob("gpu/canon", wb, str(dest / "w.bin"))
            assert _verify_digest_of_file(str(dest / "w.bin"), blob.digest)
            # GPU pull of the canonical-mode manifest still verifies (via
            # the chunk annotation at chunk rate)
            back = g.pull_to_gpu("gpu/canon", "v1")
            assert torch.equal(back["w.bin"], src)
        finally:
            mdx.stop()
            s3d.stop()

    def test_canonical_device_beats_gpu_single_chain(self, engine):
        """The D2H+SHA-NI canonical path must outrun the single-lane GPU
        chain (the design rationale for putting the sequential chain on the
        CPU)."""
        import time

        size = 256 << 20
        dev = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
        # raw engine calls never order against torch's stream — sync the
        # producer like GpuClient._sync_producers does, or the D2H reads
        # race the randint kernel (observed as a digest mismatch on HW)
        torch.cuda.synchronize()
        t0 = time.monotonic()
        got = engine.sha256_canonical_device(dev.data_ptr(), size)
        t_cpu = time.monotonic() - t0
        t0 = time.monotonic()
        gpu = engine.sha256_multibuf([(dev.data_ptr(), size)])
        t_gpu = time.monotonic() - t0
        assert got == gpu[:32]
        # informational rates land in the log either way
        print(f"canonical D2H+SHA-NI: {size / t_cpu / 2**30:.2f} GiB/s, "
              f"GPU single chain: {size / t_gpu / 2**30:.2f} GiB/s")
        assert t_cpu < t_gpu


class TestPushFaultInjection:
    def test_push_part_transport_fault_retries(self, tmp_path, monkeypatch):
        """A dropped connection mid-part must be retried with a fresh
        socket and the push must complete (reference per-part retry x3,
        extension_s3.go:133-148)."""
        from util_servers import start_modelxd_s3, start_s3d

        from modelx_amd.client.gpu import GpuClient

        s3d = start_s3d(str(tmp_path / "s3"))
        mdx = start_modelxd_s3(s3d.url, redirect=True)
        try:
            g = GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20)
            state = {"fails": 0}
            real_engine = g.engine

            class FlakyEngine:
                """pybind11 instances reject setattr — proxy the engine and
                fail the first two part uploads at the transport level."""

                def __getattr__(self, name):
                    return getattr(real_engine, name)

                def push_part_from_device(self, url, method, headers, ptr, length):
                    if state["fails"] < 2:
                        state["fails"] += 1
                        raise RuntimeError("push: send_body failed (injected)")
                    return real_engine.push_part_from_device(url, method, headers,
                                                             ptr, length)

            g.engine = FlakyEngine()
            src = torch.randint(0, 256, (20 << 20,), dtype=torch.uint8,
                                device="cuda:0")
            g.push_from_gpu("gpu/fault", "v1", {"w.bin": src}, part_bytes=4 << 20)
            g.engine = real_engine
            assert state["fails"] == 2
            back = g.pull_to_gpu("gpu/fault", "v1")
            assert torch.equal(back["w.bin"], src)
        finally:
            mdx.stop()
            s3d.stop()

    def test_drain_boundaries_on_minimum_pool(self, tmp_path):
        """Multi-slot parts plus a part ending a few bytes past a slot edge,
        pushed through the smallest pool a drain can run on (2 slots): the
        prefetch / swap / tail steps of the double-buffered D2H drain."""
        from util_servers import start_modelxd_s3, start_s3d

        from modelx_amd.client.gpu import GpuClient

        s3d = start_s3d(str(tmp_path / "s3"))
        mdx = start_modelxd_s3(s3d.url, redirect=True)
        try:
            g = GpuClient(mdx.url, device=0, num_slots=2, slot_bytes=1 << 20)
            src = torch.randint(0, 256, ((9 << 20) + 5,), dtype=torch.uint8,
                                device="cuda:0")
            g.push_from_gpu("gpu/drain", "v1", {"w.bin": src}, part_bytes=4 << 20)
            back = g.pull_to_gpu("gpu/drain", "v1")
            assert torch.equal(back["w.bin"], src)
        finally:
            mdx.stop()
            s3d.stop()

    def test_slots_return_after_failed_push(self, tmp_path):
        """Every failed push_part_from_device gives both pinned slots back:
        on a 2-slot engine a single lost slot would block the next drain
        forever (shown here as a failed assertion, not a hang)."""
        import threading

        from util_servers import BUCKET, start_s3d

        from modelx_amd import _core

        s3d = start_s3d(str(tmp_path / "s3"))
        try:
            eng = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=4)
            size = 3 << 20
            data = torch.randint(0, 256, (size,), dtype=torch.uint8)
            dev = data.cuda()
            torch.cuda.synchronize()
            for _ in range(3):
                # unsigned PUT: s3d answers 403
                with pytest.raises(RuntimeError):
                    eng.push_part_from_device(f"{s3d.url}/{BUCKET}/unsigned", "PUT", {},
                                              dev.data_ptr(), size)
            got = []
            t = threading.Thread(
                target=lambda: got.append(eng.sha256_canonical_device(dev.data_ptr(), size)),
                daemon=True)
            t.start()
            t.join(20)
            assert not t.is_alive(), "canonical digest blocked: a pinned slot was lost"
            assert got == [hashlib.sha256(data.numpy().tobytes()).digest()]
        finally:
            s3d.stop()


class TestRegistryStreamFallback:
    def test_gpu_pull_without_redirect(self, tmp_path):
        """Against a redirect-less registry the GPU pull must degrade to
        streaming through the registry (pull.go:206-215 semantics), not
        fail."""
        from util_servers import start_modelxd_s3, start_s3d

        from modelx_amd.client.gpu import GpuClient

        s3d = start_s3d(str(tmp_path / "s3"))
        mdx = start_modelxd_s3(s3d.url, redirect=False)
        try:
            g = GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20)
            src = torch.randint(0, 256, ((9 << 20) + 123,), dtype=torch.uint8,
                                device="cuda:0")
            g.push_from_gpu("gpu/noredir", "v1", {"w.bin": src})
            back = g.pull_to_gpu("gpu/noredir", "v1")
            assert torch.equal(back["w.bin"], src)
        finally:
            mdx.stop()
            s3d.stop()


class TestZstdBatchedPull:
    def test_many_zstd_blobs_batched_decode(self, tmp_path):
        """pull_to_gpu with several +zstd blobs runs the batched decode
        (one footer/table pass + one rc sync for the whole set) and the
        batched raw-digest verify; bytes must round-trip exactly."""
        from util_servers import start_modelxd_s3, start_s3d

        from modelx_amd.client.gpu import GpuClient

        s3d = start_s3d(str(tmp_path / "s3"))
        mdx = start_modelxd_s3(s3d.url, redirect=True)
        try:
            g = GpuClient(mdx.url, device=0, num_slots=4, slot_bytes=8 << 20)
            tensors = {}
            for i in range(6):
                data = (bytes([i]) * 997 + os.urandom(31)) * 4096  # compressible
                tensors[f"w{i}.bin"] = torch.frombuffer(bytearray(data),
                                                        dtype=torch.uint8).cuda()
            g.push_from_gpu("gpu/zmany", "v1", tensors, compress="zstd")
            back = g.pull_to_gpu("gpu/zmany", "v1", parallel=4)
            for name, t in tensors.items():
                assert torch.equal(back[name], t), name
            phases = [s["phase"] for s in g.last_stats]
            assert "pull-zstd-decompress-batched" in phases
            assert "pull-zstd-raw-verify-batched" in phases
            # corruption must still surface through the batched path
            import modelx_amd.wire.errors as er2

            store_root = s3d.proc.args[s3d.proc.args.index("--root") + 1]
            import glob as g2

            blobs = g2.glob(os.path.join(store_root, "modelx", "registry",
                                         "gpu/zmany/blobs/*/*"))
            big = max(blobs, key=os.path.getsize)
            with open(big, "r+b") as f:
                f.seek(os.path.getsize(big) // 3)
                b0 = f.read(1)
                f.seek(os.path.getsize(big) // 3)
                f.write(bytes([b0[0] ^ 0x40]))
            with pytest.raises(Exception):
                g.pull_to_gpu("gpu/zmany", "v1", parallel=4)
        finally:
            mdx.stop()
            s3d.stop()

    def test_leaves_many_matches_single(self, engine):
        datas = [torch.randint(0, 256, (s,), dtype=torch.uint8).cuda()
                 for s in (1, 4096, (1 << 20) + 17, 5 << 20)]
        items = [(t.data_ptr(), t.numel(), 1 << 20) for t in datas]
        many = engine.sha256_chunk_leaves_many(items)
        for t, leaves in zip(datas, many):
            assert leaves == engine.sha256_chunk_leaves(t.data_ptr(), t.numel(), 1 << 20)


class TestFseWeightsDevice:
    def test_device_compress_bf16_bytes(self, engine):
        """The CDNA4 compress kernel emits FSE-compressed huffman weight
        tables for full-byte alphabets (bf16 tensor bytes): ratio must beat
        raw and the blob must decode via our decoder AND libzstd."""
        import ctypes

        from modelx_amd import _core

        torch.manual_seed(5)
        data = ((torch.randn(4 << 20) * 0.02).to(torch.bfloat16)
                .view(torch.uint8).numpy().tobytes())
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        bound = _core.zstd_compress_bound(len(data))
        dst = torch.empty(bound, dtype=torch.uint8, device="cuda")
        n = engine.zstd_compress_device(src.data_ptr(), len(data), 128 << 10,
                                        dst.data_ptr(), bound)
        blob = bytes(dst[:n].cpu().numpy().tobytes())
        assert n / len(data) < 0.85, f"ratio {n / len(data):.3f}"
        assert _core.zstd_decompress_cpu(blob) == data
        back = torch.empty(len(data), dtype=torch.uint8, device="cuda")
        m = engine.zstd_decompress_device(dst.data_ptr(), n, back.data_ptr(),
                                          len(data))
        assert m == len(data)
        assert bytes(back.cpu().numpy().tobytes()) == data
        z = ctypes.CDLL("libzstd.so.1")
        z.ZSTD_decompress.restype = ctypes.c_size_t
        z.ZSTD_isError.restype = ctypes.c_uint
        out = ctypes.create_string_buffer(len(data))
        k = z.ZSTD_decompress(out, len(data), blob, len(blob))
        assert not z.ZSTD_isError(k) and out.raw[:k] == data


class TestTlsDataPlane:
    def test_gpu_pull_push_via_https_presigned(self, tmp_path, monkeypatch):
        """The pinned-ring engine speaks TLS: ranged GETs and multipart
        part PUTs against https presigned URLs from a TLS object store
        (production S3 endpoints are TLS; a plain-TCP-only engine would
        strand the GPU data plane)."""
        import subprocess
        import time

        from util_servers import (ACCESS_KEY, BUCKET, MODELXD, S3D, SECRET_KEY,
                                  ServerProc, _build_servers, free_port, wait_http)

        from modelx_amd import _core
        from modelx_amd.client.gpu import GpuClient

        _build_servers()
        d = tmp_path / "certs"
        d.mkdir()
        cert, key = str(d / "cert.pem"), str(d / "key.pem")
        r = subprocess.run(["openssl", "req", "-x509", "-newkey", "rsa:2048",
                            "-keyout", key, "-out", cert, "-days", "1", "-nodes",
                            "-subj", "/CN=127.0.0.1"], capture_output=True)
        if r.returncode != 0:
            pytest.skip("openssl cert generation failed")
        monkeypatch.setenv("MODELX_TLS_INSECURE", "1")
        s3_port = free_port()
        s3 = ServerProc([S3D, "--listen", f"127.0.0.1:{s3_port}", "--root",
                         str(tmp_path / "s3"), "--access-key", ACCESS_KEY,
                         "--secret-key", SECRET_KEY, "--tls-cert", cert,
                         "--tls-key", key], s3_port)
        os.makedirs(tmp_path / "s3" / BUCKET, exist_ok=True)
        deadline = time.time() + 10
        while time.time() < deadline:
            try:
                if _core.http_get(f"https://127.0.0.1:{s3_port}/healthz")[0] == 200:
                    break
            except RuntimeError:
                time.sleep(0.1)
        mdx_port = free_port()
        mdx = ServerProc([MODELXD, "--listen", f"127.0.0.1:{mdx_port}", "--s3-url",
                          f"https://127.0.0.1:{s3_port}", "--s3-bucket", BUCKET,
                          "--s3-access-key", ACCESS_KEY, "--s3-secret-key",
                          SECRET_KEY, "--enable-redirect"], mdx_port)
        wait_http(mdx_port)
        try:
            g = GpuClient(f"http://127.0.0.1:{mdx_port}", device=0,
                          num_slots=4, slot_bytes=8 << 20)
            src = torch.randint(0, 256, ((20 << 20) + 77,), dtype=torch.uint8,
                                device="cuda:0")
            # push parts go D2H -> https PUT; pull is https ranged GETs -> HBM
            g.push_from_gpu("tls/gpu", "v1", {"w.bin": src}, part_bytes=4 << 20)
            desc = next(b for b in g.remote.get_manifest("tls/gpu", "v1").blobs
                        if b.name == "w.bin")
            url, _ = g._download_url("tls/gpu", desc)
            assert url.startswith("https://")
            back = g.pull_to_gpu("tls/gpu", "v1")
            assert torch.equal(back["w.bin"], src)
        finally:
            mdx.stop()
            s3.stop()
