"""Block-search gunzip on the GPU: ``gunzip_plan_device(search=True)`` and
``gunzip_emit_device`` (core/hip/inflate.hip) on the stock streams of
test_inflate_search, against the source bytes and the host model's span count,
at two source and two destination phases with guard bytes around the output;
a stale plan and a flipped stored byte; and ``GpuClient(gpu_gunzip="any")``
pulling a directory that the stock CPU client pushed."""
import gc
import gzip

import pytest

torch = pytest.importorskip("torch")

from modelx_amd import _core

from test_deflate import words
from test_gpu_aead import to_dev, to_host
from test_gpu_gunzip import GUARD, WANT, engine, pull, stack  # noqa: F401 (fixtures)
from test_inflate import bad_members
from test_inflate_search import KEPT_STATUSES, noise, search_members

pytestmark = pytest.mark.gpu


def gunzip(engine, src, member, sphase, dphase):
    ptr = src.data_ptr() + sphase
    plan = engine.gunzip_plan_device(ptr, len(member), search=True)
    assert plan["status"] == "ok"
    n, at = plan["out_bytes"], GUARD + dphase
    out = torch.full((n + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert engine.gunzip_emit_device(ptr, len(member), plan["plan"], out.data_ptr() + at, n) == n
    got = to_host(out)
    assert got[:at] == b"\xa5" * at and got[at + n:] == b"\xa5" * (len(got) - at - n)
    return plan, got[at:at + n]


@pytest.mark.parametrize("name", sorted(search_members()))
def test_device_equals_source_and_host_spans(engine, name):
    member, x = search_members()[name]
    want = _core.gzip_inflate_plan_host(member, search=True)
    for sphase in (0, 5):
        src = to_dev(bytes(sphase) + member + bytes(16))
        for dphase in (0, 3):
            plan, got = gunzip(engine, src, member, sphase, dphase)
            assert (plan["spans"], plan["out_bytes"]) == (want["spans"], len(x)), (sphase, dphase)
            assert got == x, (sphase, dphase)


@pytest.mark.parametrize("name", KEPT_STATUSES)
def test_ineligible_members_keep_their_status(engine, name):
    member, status = bad_members()[name]
    src = to_dev(bytes(5) + member + bytes(16))
    plan = engine.gunzip_plan_device(src.data_ptr() + 5, len(member), search=True)
    assert plan == {"status": status, "out_bytes": 0, "spans": 0, "plan": b""}


def test_emit_raises_on_a_stale_search_plan(engine):
    member, x = search_members()["mix"]
    src = to_dev(member + bytes(16))
    plan = engine.gunzip_plan_device(src.data_ptr(), len(member), search=True)
    engine.gunzip_plan_device(src.data_ptr(), len(member))  # any plan call replaces the windows
    out = torch.zeros(len(x), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="stale"):
        engine.gunzip_emit_device(src.data_ptr(), len(member), plan["plan"], out.data_ptr(), len(x))


def test_emit_of_a_search_plan_raises_on_a_flipped_stored_byte(engine):
    member = bytearray(gzip.compress(noise(300000)))
    member[150000] ^= 1  # inside a stored block: only the CRC-32 can tell
    member = bytes(member)
    src = to_dev(member + bytes(16))
    with pytest.raises(RuntimeError, match="CRC-32"):
        gunzip(engine, src, member, 0, 0)


def test_pull_of_a_stock_gzip_directory_with_search(stack, tmp_path):
    from modelx_amd.client import Client
    from modelx_amd.client.gpu import GpuClient
    from modelx_amd.config import ModelConfig

    want = dict(WANT, **{"big.txt": words(6, 1 << 20)})  # test_pull_of_a_stock_gzip_directory's
    root = tmp_path / "model"
    for k, v in want.items():
        (root / "d" / k).parent.mkdir(parents=True, exist_ok=True)
        (root / "d" / k).write_bytes(v)
    (root / "modelx.yaml").write_text(ModelConfig(description="stock gzip").to_yaml())
    Client(stack[0].url).push("gunzip/stock-any", "v1", str(root), quiet=True)
    client = GpuClient(stack[0].url, device=0, num_slots=4, slot_bytes=1 << 20, gpu_gunzip="any")
    phases = pull(client, "gunzip/stock-any", want)
    assert "pull-targz-stream" not in phases and "pull-gunzip-cpu" not in phases
    assert phases["pull-gunzip"]["search"] is True and phases["pull-gunzip"]["spans"] >= 3
    del client
    gc.collect()
