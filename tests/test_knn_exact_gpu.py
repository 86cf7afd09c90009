"""GPU: the kNN graph's order contract (csrc/graph.hip, header) and accuracy, on clouds whose answer is known exactly.

Contract: neighbours in stable ascending (distance, index) order, the lower index first on equal distances, rank 0 dropped
positionally -- `sort(dist, stable)[..., 1:k+1]`.  tests/knn_cases.py builds the clouds and the float64 reference;
tests/test_knn_cases_cpu.py proves that the clouds have the ties they are here for.

Which launch each test reaches with the default environment (launch_knn in csrc/graph.hip, spgan_knn_ws in csrc/knn_pipe.hip):

  test_lattice_f64                      knn_f64_kernel<11,1> <21,2> <11,3> <33,4>
  test_lattice_f32                      knn_f32_kernel<11,8> <21,16> <33,16> <21,32> <21,64> <33,128> <21,128> <33,64>
  test_lattice_matrix_core[pipe-*]      knn_split_kernel + knn_pipe_kernel, 1 / 2 / 3 / 4 / 5 / 6 / 9 tiles
  test_lattice_matrix_core[single-*]    knn_mfma3_kernel<11,64>, the same shapes
  test_lattice_mfma3_128                knn_mfma3_kernel<11,128>
  test_fp32_mfma_kernel_in_a_child_process   knn_mfma_kernel<11,64> and <11,128> (child with SPGAN_KNN_BF16X3=0: read once per process)
  test_prototype[*]                     pipe, mfma3<11,64>, mfma3<11,128>, f32<21,32>, f64<11,3>
  test_offset[*]                        pipe, mfma3<11,64> (C 20 and 64), mfma3<11,128>, f32<21,64>
  test_offset_aligned_lo_plane[*]       pipe, mfma3<11,64> (C 17): the third bfloat16 plane of the split
  test_csr_of_*                         csr_kernel<true> (the LDS-segment route, N*k <= 65536)

When the whole suite is started with SPGAN_KNN_BF16X3=0 the "single" parametrisations run knn_mfma_kernel instead; the expectations
hold for it unchanged.
"""
import os
import subprocess
import sys

import pytest
import torch

import kernel_model as km
import knn_cases as kc
from test_kernels_gpu import knn_tie_aware, ops  # noqa: F401  (ops is a fixture)

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROUTES = pytest.mark.parametrize("pipelined", [True, False], ids=["pipe", "single"])


def run_knn(ops, x, B, N, k, mode=0, pipelined=True):
    try:
        ops.KNN_PIPELINED[0] = pipelined
        return ops.knn(x.cuda(), B, N, k, mode=mode)
    finally:
        ops.KNN_PIPELINED[0] = True


def check_lattice(ops, case, pipelined=True):
    x, ref = kc.lattice(case)
    idx = run_knn(ops, x, case.B, case.N, case.k, case.mode, pipelined)
    diff = kc.first_difference(idx, ref)
    assert diff is None, "%s (%s): %s" % (kc.case_id(case), case.route, diff)


# ----------------------------------------------------------------------------- lattice clouds: exact equality, every row and column
@pytest.mark.parametrize("case", kc.LATTICE_F64, ids=kc.case_id)
def test_lattice_f64(ops, case):
    check_lattice(ops, case)


@pytest.mark.parametrize("case", kc.LATTICE_F32, ids=kc.case_id)
def test_lattice_f32(ops, case):
    check_lattice(ops, case)


@pytest.mark.parametrize("case", kc.LATTICE_MATRIX, ids=kc.case_id)
@ROUTES
def test_lattice_matrix_core(ops, case, pipelined):
    from spgan import _lib
    assert _lib.load().spgan_knn_ws_bytes(case.B, case.N, case.C, case.k, 0) > 0      # the shape is one the tile-image route takes
    check_lattice(ops, case, pipelined)


@pytest.mark.parametrize("case", kc.LATTICE_MFMA3_128, ids=kc.case_id)
def test_lattice_mfma3_128(ops, case):
    check_lattice(ops, case)


def test_fp32_mfma_kernel_in_a_child_process():
    """knn_mfma_kernel is behind a switch that is read once per process: a fresh child, four lattice cases, one OK line."""
    env = dict(os.environ, SPGAN_KNN_BF16X3="0")
    r = subprocess.run([sys.executable, os.path.join(TESTS, "knn_cases.py"), "mfma-child"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "MFMA-CHILD OK %d cases" % len(kc.MFMA_CHILD_CASES) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ----------------------------------------------------------------------------- prototype clouds: closed form on arbitrary fp32 values
PROTO_ROUTES = [  # (B, N, C, k, mode, pipelined)
    pytest.param(2, 130, 64, 10, 0, True, id="pipe"),
    pytest.param(2, 130, 64, 10, 0, False, id="mfma3-64"),
    pytest.param(2, 130, 128, 10, 0, True, id="mfma3-128"),
    pytest.param(2, 130, 20, 20, 0, True, id="f32-k20"),
    pytest.param(2, 130, 3, 10, 1, True, id="f64"),
]


@pytest.mark.parametrize("m", kc.PROTO_M)
@pytest.mark.parametrize("B,N,C,k,mode,pipelined", PROTO_ROUTES)
def test_prototype(ops, B, N, C, k, mode, pipelined, m):
    """Identical rows give identical distances whatever the rounding: the result is the tie rule's alone (m = 1: b*N + [1..k])."""
    x = kc.prototype_cloud(B, N, C, m, lattice_protos=(mode == 1))
    diff = kc.first_difference(run_knn(ops, x, B, N, k, mode, pipelined), kc.prototype_expected(B, N, m, k))
    assert diff is None, diff


# ----------------------------------------------------------------------------- offset clouds: accuracy where the expanded form cancels
OFFSET_ROUTES = [  # (C, N, k, pipelined)
    pytest.param(20, 97, 10, True, id="pipe-C20"),
    pytest.param(20, 97, 10, False, id="mfma3-64-C20"),
    pytest.param(64, 333, 10, True, id="pipe-C64"),
    pytest.param(64, 333, 10, False, id="mfma3-64-C64"),
    pytest.param(128, 130, 10, True, id="mfma3-128"),
    pytest.param(64, 130, 20, True, id="f32-k20"),
]


@pytest.mark.parametrize("C,N,k,pipelined", OFFSET_ROUTES)
def test_offset(ops, C, N, k, pipelined):
    """x = 8 + 0.5 * normal.  The bound is derived (knn_cases.offset_tol), not measured."""
    B = 2
    x = kc.offset_cloud(B, N, C)
    # Maximum rank error measured on the MI355X against the derived bound (which stays the bound):
    #   knn_split + knn_pipe   C 20: 0       of 0.0079     C 64: 0.00092 of 0.070
    #   knn_mfma3<11,64>       C 20: 0       of 0.0079     C 64: 0.00092 of 0.070
    #   knn_mfma3<11,128>      C 128: 0.00051 of 0.27
    #   knn_f32<21,64>         C 64, k 20: 0.0018 of 0.070
    tol = kc.offset_tol(x)
    sd = kc.sorted_dist_f64(x, B, N)[0]
    med = sd[:, :, k].median().item()
    assert tol <= 0.02 * med, "vacuous: tol %.4g against a median k-th-neighbour distance of %.4g" % (tol, med)
    idx = run_knn(ops, x, B, N, k, 0, pipelined)
    print("offset C=%d N=%d k=%d pipelined=%s: rank error %.4g, tol %.4g, median k-th distance %.4g"
          % (C, N, k, pipelined, kc.rank_error(idx, x, B, N, k, sd), tol, med))
    knn_tie_aware(idx, x.cuda(), B, N, k, tol=tol)


@ROUTES
def test_offset_aligned_lo_plane(ops, pipelined):
    """The same bound on a cloud whose lo planes are aligned (knn_cases.aligned_lo_cloud): a split product without its third plane is
    at 0.041 there (tests/test_knn_cases_cpu.py), four times the bound; with it at 0."""
    B, N, C, k = kc.ALIGNED_LO_SHAPE
    x = kc.aligned_lo_cloud(B, N, C)
    tol = kc.offset_tol(x)
    sd = kc.sorted_dist_f64(x, B, N)[0]
    assert tol <= 0.02 * sd[:, :, k].median().item()
    idx = run_knn(ops, x, B, N, k, 0, pipelined)
    print("aligned lo C=%d N=%d pipelined=%s: rank error %.4g, tol %.4g" % (C, N, pipelined, kc.rank_error(idx, x, B, N, k, sd), tol))
    knn_tie_aware(idx, x.cuda(), B, N, k, tol=tol)


# ----------------------------------------------------------------------------- CSR of the graphs these clouds produce
def test_csr_of_a_collapsed_cloud(ops):
    """m = 1: ten hubs of in-degree N (rows 1..10 of each shape), every other segment empty."""
    B, N, k = 2, 256, 10
    idx = kc.prototype_expected(B, N, 1, k).cuda()
    rowptr, src = ops.csr_build(idx, B, N)
    rp, sr = km.csr_build(idx, B, N)
    deg = rp.cpu().long().diff().view(B, N)
    assert (deg[:, 1:k + 1] == N).all() and deg.sum().item() == B * N * k
    assert torch.equal(rowptr.cpu(), rp.cpu()) and torch.equal(src.cpu(), sr.cpu())


def test_csr_of_five_prototypes(ops):
    B, N, k = 2, 130, 10
    idx = kc.prototype_expected(B, N, 5, k).cuda()
    rowptr, src = ops.csr_build(idx, B, N)
    rp, sr = km.csr_build(idx, B, N)
    assert torch.equal(rowptr.cpu(), rp.cpu()) and torch.equal(src.cpu(), sr.cpu())
