#!/usr/bin/env python3
"""Record tests/golden/nt_plan_parent.npz: the answers of the five gemm_nt selection queries that existed before the host-side plan
(spgan_gemm_nt_col_blocks / _owns_columns / _y16_ok / _uses_w_image, spgan_edge_attend_bwd_dt_selected) on every case of
tests/nt_plan_cases.py, asked of a libspgan_hip.so built from the commit BEFORE csrc/gemm_nt_plan.hpp (its parent).  No GPU: the queries
never read through a pointer.  Recorded once; the cases and the struct layout must be those of the recording.

    git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/sp-gan_amd
    env -u SPGAN_NT_WIDE -u SPGAN_NT_WIDE16 -u SPGAN_NT_WIDE3 -u SPGAN_NT3_CFG \\
        python tests/golden/make_golden_nt_plan.py /tmp/parent/sp-gan_amd/spgan/libspgan_hip.so
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nt_plan_cases as npc                                           # noqa: E402
from spgan import _lib                                                # noqa: E402


def main():
    assert not any(os.environ.get(v) for v in ("SPGAN_NT_WIDE", "SPGAN_NT_WIDE16", "SPGAN_NT_WIDE3", "SPGAN_NT3_CFG")), "record with the switches unset"
    lib = ctypes.CDLL(sys.argv[1])
    for q in ("spgan_gemm_nt_col_blocks", "spgan_gemm_nt_owns_columns", "spgan_gemm_nt_y16_ok", "spgan_gemm_nt_uses_w_image",
              "spgan_edge_attend_bwd_dt_selected"):
        getattr(lib, q).restype, getattr(lib, q).argtypes = _lib.SIGNATURES[q]
    cs, _ = npc.cases()
    answers = np.array([npc.ask(lib, c["fields"]) for c in cs], dtype=np.int16)
    out = os.path.join(HERE, "nt_plan_parent.npz")
    np.savez_compressed(out, names=np.array([c["name"] for c in cs]), answers=answers, queries=np.array(npc.QUERIES))
    print("%s: %d cases, %d bytes" % (out, len(cs), os.path.getsize(out)))


if __name__ == "__main__":
    main()
