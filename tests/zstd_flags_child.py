"""Child process of test_gpu_zstd_interop.py::test_serial_switches_in_a_child.

MODELX_ZSTD_FLAGS is read once per process, so the other position of its
switches needs a process of its own. Decodes the one-blob libzstd corpus on the
device and runs one device compress + decode of the bf16 payload, then prints
one JSON line of SHA-256 digests; the parent compares them with hashlib over
the payloads. Run as a program, never imported by the suite.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main() -> int:
    import torch  # before the extension (docs/engineering-notes.md #16)

    from modelx_amd import _core

    import util_zframes as uz

    def to_dev(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()

    def sha(t, n):
        return hashlib.sha256(t[:n].cpu().numpy().tobytes()).hexdigest()

    eng = _core.GpuEngine(device=0, num_slots=2, slot_bytes=1 << 20, num_streams=2)
    out = {"flags": os.environ.get("MODELX_ZSTD_FLAGS")}

    blob, payload = uz.corpus_blob()
    src = to_dev(blob)
    dst = torch.zeros(len(payload), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = eng.zstd_decompress_device(src.data_ptr(), len(blob), dst.data_ptr(), len(payload))
    out["corpus_len"] = n
    out["corpus"] = sha(dst, n)

    data = uz.payloads()["bf16"]
    src = to_dev(data)
    bound = _core.zstd_compress_bound(len(data), 128 << 10)
    comp = torch.zeros(bound, dtype=torch.uint8, device="cuda")
    back = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c = eng.zstd_compress_device(src.data_ptr(), len(data), 128 << 10, comp.data_ptr(), bound)
    host_blob = comp[:c].cpu().numpy().tobytes()
    seen = uz.collections.Counter()
    for c_off, c_size, _, _ in _core.zstd_seek_table(host_blob):
        seen += uz.walk(host_blob[c_off:c_off + c_size])
    out["bf16_huffman_blocks"] = seen["lit:huffman-4"]
    out["bf16_libzstd"] = hashlib.sha256(uz.decompress(host_blob, len(data))).hexdigest()
    m = eng.zstd_decompress_device(comp.data_ptr(), c, back.data_ptr(), len(data))
    out["bf16_len"] = m
    out["bf16_device"] = sha(back, m)
    torch.cuda.synchronize()
    print("ZFLAGS " + json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
