#!/usr/bin/env python
"""Which paths of the DEFLATE host model the test corpus walks (no GPU).

Runs ``_core.gzip_chunk_stats_host`` over every chunk of every case of
tests/test_gpu_gzip.py::test_device_equals_host_model (payload family x length
x source offset, from tests/test_deflate.py) and prints, for the five families
the suite started with and for all of them, the table of
profiles/deflate_kernel.md.

    python tools/gzip_corpus_stats.py
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import torch  # noqa: F401,E402  (before _core)

import test_deflate as td  # noqa: E402
from modelx_amd import _core  # noqa: E402

OLD = ["far", "onebyte_runs", "random", "words", "zeros"]


def corpus(names):
    agg = {"cases": 0, "chunks": 0, "stored": 0, "max_ll_len": 0, "max_d_len": 0,
           "max_token_bits": 0, "three_word_puts": 0, "three_word_nonzero": 0, "max_dist": 0,
           "builder_steps_max": 0, "shrink_steps": 0}
    for name in names:
        for n in td.LENGTHS:
            for offset in td.OFFSETS:
                agg["cases"] += 1
                x = td.payload(name)[offset:offset + n]
                for at in range(0, n, td.C):
                    s = _core.gzip_chunk_stats_host(x[at:at + td.C])
                    agg["chunks"] += 1
                    agg["stored"] += s["stored"]
                    agg["three_word_puts"] += s["three_word_puts"]
                    agg["three_word_nonzero"] += s["three_word_nonzero"]
                    agg["shrink_steps"] += sum(s["builder_shrink_steps"].values())
                    for k in ("max_dist", "builder_steps_max"):
                        agg[k] = max(agg[k], s[k])
                    if not s["stored"]:  # a stored chunk's codes never reach the writer
                        for k in ("max_ll_len", "max_d_len", "max_token_bits"):
                            agg[k] = max(agg[k], s[k])
    return agg


if __name__ == "__main__":
    before, after = corpus(OLD), corpus(sorted(td.PAYLOADS))
    for k in before:
        print("| %s | %s | %s |" % (k, before[k], after[k]))
