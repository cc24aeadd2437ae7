"""gunzip on the GPU: ``GpuEngine.gunzip_plan_device`` and
``gunzip_emit_device`` (core/hip/inflate.hip) against the host model of
test_inflate on every member of that file, at every source and destination
phase, with guard bytes around the output; what the emit call refuses; and
``GpuClient(gpu_gunzip=True)`` end to end against modelx-s3d + modelxd."""
import functools
import gc

import pytest

torch = pytest.importorskip("torch")

from modelx_amd import _core

from test_deflate import C, PAYLOADS, payload, words
from test_gpu_aead import to_dev, to_host
from test_inflate import OWN_LENGTHS, bad_members, good_members

pytestmark = pytest.mark.gpu

SRC_PHASES, DST_PHASES = [0, 1, 5, 15], [0, 3]
GUARD = 32


@pytest.fixture(scope="module")
def engine():
    return _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=2)


def mixed():
    """Seven chunks, stored (random) and Huffman (words) in turn, the last one
    short: test_gpu_gzip's fixture of that name."""
    return b"".join([payload("random")[:C], words(7, C), words(8, C), payload("random")[C:2 * C],
                     words(9, C), payload("random")[100:100 + C], words(10, 5000)])


@functools.lru_cache(maxsize=None)
def members():
    """name -> (member, source): own format, foreign, false marker, mixed."""
    out = {"own-%s-%d" % (name, n): (_core.gzip_compress_host(payload(name)[:n]), payload(name)[:n])
           for name in PAYLOADS for n in OWN_LENGTHS}
    out.update(good_members())
    out["mixed"] = (_core.gzip_compress_host(mixed()), mixed())
    return out


def gunzip(engine, src, member, sphase, dphase, cap=None):
    """Plan and emit the member that lies `sphase` bytes into `src`: the plan
    and the output, whose guard bytes are checked."""
    ptr = src.data_ptr() + sphase
    plan = engine.gunzip_plan_device(ptr, len(member))
    assert plan["status"] == "ok"
    n, at = plan["out_bytes"], GUARD + dphase
    out = torch.full((n + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    wrote = engine.gunzip_emit_device(ptr, len(member), plan["plan"], out.data_ptr() + at,
                                      n if cap is None else cap)
    got = to_host(out)
    assert wrote == n
    assert got[:at] == b"\xa5" * at and got[at + n:] == b"\xa5" * (len(got) - at - n)
    return plan, got[at:at + n]


@pytest.mark.parametrize("name", sorted(members()))
def test_device_equals_host_model(engine, name):
    member, x = members()[name]
    want = _core.gzip_inflate_plan_host(member)
    assert want["status"] == "ok" and want["out_bytes"] == len(x)
    for sphase in SRC_PHASES:
        src = to_dev(bytes(sphase) + member + bytes(16))
        for dphase in DST_PHASES:
            plan, got = gunzip(engine, src, member, sphase, dphase)
            assert (plan["spans"], plan["out_bytes"]) == (want["spans"], len(x)), (sphase, dphase)
            assert got == x, (sphase, dphase)


@pytest.mark.parametrize("name", sorted(set(bad_members()) - {"flipped-stored"}))
def test_ineligible_members_report_the_host_status(engine, name):
    member, status = bad_members()[name]
    for sphase in (0, 5):
        src = to_dev(bytes(sphase) + member + bytes(16))
        plan = engine.gunzip_plan_device(src.data_ptr() + sphase, len(member))
        assert plan == {"status": status, "out_bytes": 0, "spans": 0, "plan": b""}


@pytest.mark.parametrize("name", ["trailer-crc", "flipped-stored"])
def test_emit_raises_on_a_wrong_crc(engine, name):
    """The plan call reads structure only: a wrong CRC-32 in the trailer, or a
    flipped stored byte under the right one, is found after the emit."""
    member = bytearray(members()["mixed"][0])
    member[-8] ^= 1
    member = bytes(member) if name == "trailer-crc" else bad_members()[name][0]
    src = to_dev(member + bytes(16))
    with pytest.raises(RuntimeError, match="CRC-32"):
        gunzip(engine, src, member, 0, 0)


def test_emit_raises_on_a_short_destination(engine):
    member, x = members()["mixed"]
    src = to_dev(member + bytes(16))
    with pytest.raises(RuntimeError, match="dst_cap"):
        gunzip(engine, src, member, 0, 0, cap=len(x) - 1)


# ------------------------------------------------------------ end to end --

@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    from util_servers import start_modelxd_s3, start_s3d

    s3d = start_s3d(str(tmp_path_factory.mktemp("s3-gunzip")))
    mdx = start_modelxd_s3(s3d.url, redirect=True)
    yield mdx, s3d
    mdx.stop()
    s3d.stop()


@pytest.fixture(scope="module")
def clients(stack):
    from modelx_amd.client.gpu import GpuClient

    made = {flag: GpuClient(stack[0].url, device=0, num_slots=4, slot_bytes=1 << 20,
                            gpu_gunzip=flag) for flag in (False, True)}
    yield made
    made.clear()
    gc.collect()


WANT = {"a.bin": payload("words")[5:5 + 2 * C + 4999], "empty.bin": b"",
        "sub/r.bin": payload("random")[1:3002]}


def pull(client, repo, want):
    client.last_stats.clear()
    back = client.pull_to_gpu(repo, "v1", expand_dirs=True)
    assert {k: to_host(t) for k, t in back.items()} == {"d/" + k: v for k, v in want.items()}
    return {s["phase"]: s for s in client.last_stats}


def test_pull_of_a_gpu_pushed_directory(clients):
    files = {k: to_dev(v + bytes(16))[:len(v)] for k, v in WANT.items()}
    manifest = clients[True].push_from_gpu("gunzip/own", "v1", {}, dirs={"d": files},
                                           dir_format="tar+gz", part_bytes=65536)
    desc, = [b for b in manifest.blobs if b.name == "d"]
    phases = pull(clients[True], "gunzip/own", WANT)
    assert "pull-targz-stream" not in phases and "pull-gunzip-cpu" not in phases
    assert phases["pull-gunzip"]["stored_bytes"] == desc.size
    assert phases["pull-gunzip"]["bytes"] > 2 * C and phases["pull-gunzip"]["spans"] >= 3
    phases = pull(clients[False], "gunzip/own", WANT)
    assert "pull-targz-stream" in phases and "pull-gunzip" not in phases


def test_pull_of_a_stock_gzip_directory(clients, stack, tmp_path):
    from modelx_amd.client import Client
    from modelx_amd.config import ModelConfig

    # 1 MiB of words: more than GUNZIP_SPAN_MAX_CODED of Huffman blocks in one span
    want = dict(WANT, **{"big.txt": words(6, 1 << 20)})
    root = tmp_path / "model"
    for k, v in want.items():
        (root / "d" / k).parent.mkdir(parents=True, exist_ok=True)
        (root / "d" / k).write_bytes(v)
    (root / "modelx.yaml").write_text(ModelConfig(description="stock gzip").to_yaml())
    Client(stack[0].url).push("gunzip/stock", "v1", str(root), quiet=True)
    phases = pull(clients[True], "gunzip/stock", want)
    assert "pull-targz-stream" not in phases and "pull-gunzip" not in phases
    assert phases["pull-gunzip-cpu"]["status"] == "too-long"
