"""GPU: spgan_gemm_tn executes its host-side plan (csrc/gemm_tn_plan.hpp).  One shape per branch of the plan, launched through the C ABI with a
workspace of exactly the plan's bytes in front of a guard region: the plan names the expected kernel, the kernel writes `splits` partials and
nothing behind them, and the finished product meets the bound of that kernel's own test (test_kernels_gpu.py::test_gemm_tn,
test_kernels2_gpu.py::test_gemm_tn_skinny, test_f16_gpu.py::test_gemm_tn_bf16_operands / ::test_gemm_tn_bf16x3_is_fp32_equivalent).  The three
invalid forms are refused by the launch and reported by the query."""
import ctypes as C

import pytest
import torch

from test_kernels_gpu import close, ops, rnd  # noqa: F401  (ops is a fixture)

pytestmark = pytest.mark.gpu

SKINNY, TILE, LP, WIDE3 = 1, 2, 3, 4
EINVAL = -22
GUARD = 4096                    # floats behind the workspace
SENTINEL = -12345.5
LP_OF = {"f32": 0, "f16": 1, "bf16x3": 2}


def _plan(lib, a):
    from spgan import _lib
    out = (C.c_int32 * len(_lib.TN_PLAN_FIELDS))()
    assert lib.spgan_gemm_tn_plan(C.byref(a), out) == 0
    p = dict(zip(_lib.TN_PLAN_FIELDS, out))
    assert lib.spgan_gemm_tn_kernel(C.byref(a)) == p["kernel"]
    return p


def _block(A, Bm, out, mode, two=None):
    from spgan._lib import GemmTNArgs
    a = GemmTNArgs()
    a.A, a.lda, a.B, a.ldb, a.C, a.ldc = A.data_ptr(), A.stride(0), Bm.data_ptr(), Bm.stride(0), out.data_ptr(), out.stride(0)
    a.M, a.Na, a.Nb = A.shape[0], A.shape[1], Bm.shape[1]
    a.mfma_lp = LP_OF[mode]
    if two is not None:
        y, p, q, r = two
        a.A2, a.lda2, a.a_scale, a.a_scale2, a.a_shift = y.data_ptr(), y.stride(0), p.data_ptr(), q.data_ptr(), r.data_ptr()
    return a


# name -> (M, Na, Nb, operand mode, unaligned views, two-tensor A; expected kernel, tile_b, fast, narrow_b, wide3_cfg)
BRANCHES = {
    "skinny.narrow_b": (4096, 64, 3, "f32", False, False, SKINNY, 0, None, 1, 0),
    "skinny.narrow_a": (4096, 3, 64, "f32", False, False, SKINNY, 0, None, 0, 0),
    "tile.32": (4096, 128, 32, "f32", False, False, TILE, 32, 1, 0, 0),
    "tile.64": (4096, 128, 64, "f32", False, False, TILE, 64, 1, 0, 0),
    "tile.128": (4096, 128, 128, "f32", False, False, TILE, 128, 1, 0, 0),
    "tile.32.unaligned": (4096, 128, 32, "f32", True, False, TILE, 32, 0, 0, 0),
    "tile.64.unaligned": (4096, 128, 64, "f32", True, False, TILE, 64, 0, 0, 0),
    "tile.128.unaligned": (4096, 128, 128, "f32", True, False, TILE, 128, 0, 0, 0),
    "lp": (8192, 128, 128, "f16", False, False, LP, 128, 1, 0, 0),
    "wide3.24": (8192, 256, 256, "bf16x3", False, False, WIDE3, 0, 1, 0, 24),
    "wide3.22": (8192, 256, 128, "bf16x3", False, False, WIDE3, 0, 1, 0, 22),
    "wide3.14": (8192, 128, 256, "bf16x3", False, False, WIDE3, 0, 1, 0, 14),
    "wide_split.tile": (8192, 256, 256, "bf16x3", False, True, TILE, 128, 1, 0, 0),     # Affine2 A: the fp32 kernel on the wide split
}


@pytest.mark.parametrize("name", list(BRANCHES))
def test_branch_runs_its_plan(ops, name):
    from spgan import _lib
    lib = _lib.load()
    M, Na, Nb, mode, unaligned, two, kernel, tile_b, fast, narrow_b, cfg = BRANCHES[name]
    if unaligned:       # A[:, 1:]-style views: rows that start 4 bytes off a 16-byte boundary
        A, Bm = rnd("tp.A.%s" % name, (M, Na + 4))[:, 1:1 + Na], rnd("tp.B.%s" % name, (M, Nb + 4))[:, 1:1 + Nb]
    else:
        A, Bm = rnd("tp.A.%s" % name, (M, Na)), rnd("tp.B.%s" % name, (M, Nb))
    tw = None
    a_eff = A.double()
    if two:
        y = rnd("tp.y.%s" % name, (M, Na))
        p, q, r = rnd("tp.p.%s" % name, (Na,)).abs() + 0.5, rnd("tp.q.%s" % name, (Na,), 0.3), rnd("tp.r.%s" % name, (Na,), 0.1)
        tw = (y, p, q, r)
        a_eff = A.double() * p.double() + y.double() * q.double() + r.double()
    out = torch.zeros((Na, Nb), device="cuda")
    a = _block(A, Bm, out, mode, tw)
    pl = _plan(lib, a)
    assert (pl["kernel"], pl["invalid"], pl["tile_b"], pl["narrow_b"], pl["wide3_cfg"]) == (kernel, 0, tile_b, narrow_b, cfg), pl
    assert fast is None or pl["fast"] == fast, pl
    splits, n = pl["splits"], Na * Nb
    assert splits == lib.spgan_gemm_tn_splits_lp(M, Na, Nb, a.mfma_lp) and splits * n * 4 == lib.spgan_gemm_tn_ws_bytes_lp(M, Na, Nb, a.mfma_lp)
    assert splits > 1
    if name == "wide_split.tile":
        assert splits == lib.spgan_gemm_tn_splits_lp(M, Na, Nb, 2)
    ws = torch.full((splits * n + GUARD,), float("nan"), device="cuda")
    ws[splits * n:] = SENTINEL
    a.ws, a.ws_bytes, a.defer_reduce = ws.data_ptr(), splits * n * 4, 1
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.spgan_gemm_tn(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert (ws[splits * n:] == SENTINEL).all(), "the launch wrote behind the plan's workspace"
    part = ws[:splits * n].view(splits, Na, Nb)
    assert torch.isfinite(part).all(), "a partial of the plan was not written"
    assert (out == 0).all(), "defer_reduce: C is the caller's to finish"
    a.ws_bytes -= 4
    assert lib.spgan_gemm_tn(C.byref(a), stream) == EINVAL          # a workspace one float short of the plan
    a.ws_bytes += 4
    a.defer_reduce = 0
    assert lib.spgan_gemm_tn(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert (ws[splits * n:] == SENTINEL).all()
    ref = a_eff.t() @ Bm.double()
    for got, what in ((out, name + ": finished product"), (part.double().sum(0).float(), name + ": sum of the partials")):
        if kernel == SKINNY:
            close(got, ref.float(), rtol=3e-5, atol=2e-4, what=what)
        elif kernel == TILE:
            close(got, ref.float(), rtol=3e-5, what=what)
        elif kernel == LP:
            rb = lambda t: t.bfloat16().float()                      # noqa: E731
            close(got, (rb(A).double().t() @ rb(Bm).double()).float(), rtol=3e-5, atol=1e-12, what=what + " (bf16-operand arithmetic)")
            close(got, ref.float(), rtol=6e-3, atol=1e-12, what=what + " (vs fp32)")
        else:
            close(got, ref.float(), rtol=2e-5, atol=1e-12, what=what)
            e3 = ((got.double() - ref).norm() / ref.norm()).item()
            assert e3 <= 2e-6, (what, e3)


@pytest.mark.parametrize("M,Na,Nb,kernel", [(4096, 64, 3, SKINNY), (4096, 128, 64, TILE)])
def test_colsum_by_product_follows_the_plan(ops, M, Na, Nb, kernel):
    """with_colsum=True asks the library which kernel runs: the by-product rides in the MFMA launch, the streaming kernel gets a colsum pass."""
    from spgan import _lib
    A, Bm = rnd("tpc.A%d" % Na, (M, Na)), rnd("tpc.B%d" % Nb, (M, Nb))
    out = torch.zeros((Na, Nb), device="cuda")
    assert _plan(_lib.load(), _block(A, Bm, out, "f32"))["kernel"] == kernel
    got, cs = ops.gemm_tn(A, Bm, with_colsum=True)
    close(cs, A.double().sum(0).float(), rtol=2e-6, atol=2e-5, what="column sums")
    close(got, (A.double().t() @ Bm.double()).float(), rtol=3e-5, atol=2e-4 if kernel == SKINNY else 1e-6, what="product")
    assert torch.equal(got, ops.gemm_tn(A, Bm))


@pytest.mark.parametrize("form", ["b_half_off_the_bf16_kernel", "a_half_on_a_skinny_shape", "b_half_unaligned"])
def test_invalid_forms_are_refused_before_any_launch(ops, form):
    """Argument errors, detected on the host: the query reports invalid, the launch returns SPGAN_EINVAL and leaves C and the workspace alone.
    (Every operand is allocated at fp32 size, whatever the block says about its storage.)"""
    from spgan import _lib
    lib = _lib.load()
    M, Na, Nb, mode = {"b_half_off_the_bf16_kernel": (8192, 128, 128, "f32"), "a_half_on_a_skinny_shape": (8192, 64, 4, "f16"),
                       "b_half_unaligned": (8192, 128, 128, "f16")}[form]
    A, Bm = torch.zeros((M, Na), device="cuda"), torch.zeros((M, Nb + 4), device="cuda")
    Bv = Bm[:, 1:1 + Nb] if form == "b_half_unaligned" else Bm[:, :Nb]
    out = torch.full((Na, Nb), SENTINEL, device="cuda")
    a = _block(A, Bv, out, mode)
    if form == "a_half_on_a_skinny_shape":
        a.a_half = 1
    else:
        a.b_half = 1
    pl = _plan(lib, a)
    assert pl["invalid"] == 1, pl
    ws = torch.full((pl["splits"] * Na * Nb,), SENTINEL, device="cuda")
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    assert lib.spgan_gemm_tn(C.byref(a), torch.cuda.current_stream().cuda_stream) == EINVAL
    torch.cuda.synchronize()
    assert (ws == SENTINEL).all() and (out == SENTINEL).all()
