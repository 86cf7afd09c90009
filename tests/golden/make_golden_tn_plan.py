#!/usr/bin/env python3
"""Record tests/golden/tn_plan_parent.npz: the answers of the seven shape-only gemm_tn / gemm_dual selection queries that existed before the
host-side plan (spgan_gemm_tn_ws_bytes / _splits / _ws_bytes_lp / _splits_lp, spgan_splitk_reduce_blocks on those splits, spgan_gemm_dual_wgs /
_rows_per_wg) on every shape of tests/tn_plan_cases.py, asked of a libspgan_hip.so built from the commit BEFORE csrc/gemm_tn_plan.hpp (its
parent).  No GPU: the queries take integers.  Recorded once; the shapes must be those of the recording.

    git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/sp-gan_amd
    python tests/golden/make_golden_tn_plan.py /tmp/parent/sp-gan_amd/spgan/libspgan_hip.so
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import tn_plan_cases as tpc                                           # noqa: E402


def main():
    lib = ctypes.CDLL(sys.argv[1])
    tpc.shape_signatures(lib)
    sh = tpc.shapes()
    answers = np.array([tpc.ask_shape(lib, *s) for s in sh], dtype=np.int64)
    out = os.path.join(HERE, "tn_plan_parent.npz")
    np.savez_compressed(out, shapes=np.array(sh, dtype=np.int32), answers=answers, queries=np.array(tpc.SHAPE_QUERIES))
    print("%s: %d shapes x %d answers, %d bytes" % (out, len(sh), answers.shape[1], os.path.getsize(out)))


if __name__ == "__main__":
    main()
