"""GPU: the promises of the non-default operand modes ("f16", "bf16x3": ops.set_mfma_operands) where they could break.
1. A grouped launch (ops.gemm_bn_groups, the Discriminator's grouped passes) equals its separate passes bit for bit in every mode -- also
   where one pass's rows and the whole launch's rows fall on different sides of a kernel-selection threshold (the selection rules must
   decide from the rows of ONE group: the kernels sum in different orders).
2. The split-bf16 operands of "bf16x3" keep fp32's whole range (csrc/split_bf16.hpp): the top binade up to FLT_MAX, where a plain
   round-to-nearest hi term overflows bf16, and +-inf / NaN, whose NaN / inf pattern in a product is the fp32 mode's."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_model as km
from test_kernels_gpu import close, rnd
from test_parity_gpu import grouped_passes_equal_separate_calls, sp  # noqa: F401  (sp is a fixture)

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16", "bf16x3"]


@pytest.fixture(scope="module")
def ops():
    from spgan import ops as o
    from spgan import _lib
    _lib.load()
    return o


@contextlib.contextmanager
def operands(ops, mode):
    ops.set_mfma_operands(mode)
    try:
        yield ops
    finally:
        ops.set_mfma_operands("f32")


# ------------------------------------------------------------------------------------------------------------------ grouped == separate
# groups, rows per pass, N, K, the mode whose selection rule the shape straddles (None: a control).  f16: the 256-row kernel
# (gemm_wide16.hip) takes (Mg/256)*(N/256) >= 256 tiles; bf16x3: the split-bf16 256-row kernel (gemm_wide3.hip) (Mg/256)*(N/128) >= 128.
GROUP_SHAPES = [
    (3, 32768, 256, 128, "f16"),        # 128 tiles per pass, 384 in the launch
    (4, 16384, 512, 256, "f16"),        # 128 per pass, 512
    (2, 65536, 256, 128, None),         # 256 per pass: every pass takes the wide kernel
    (3, 16384, 256, 128, None),         # 64 per pass, 192: below the threshold either way
    (2, 16384, 128, 64, "bf16x3"),      # 64 per pass, 128 in the launch
    (4, 8192, 256, 128, "bf16x3"),      # 64 per pass, 256
    (2, 32768, 128, 64, None),          # 128 per pass
    (3, 8192, 128, 64, None),           # 32 per pass, 96
]


def _col_blocks(ops, A, W, M, pro, group_rows, pool):
    """spgan_gemm_nt_col_blocks of the argument block gemm_bn_groups (group_rows > 0) / gemm_nt(bn=) / gemm_bn_pool (group_rows = 0) builds:
    the N-tile width of the kernel the launch runs."""
    from spgan import _lib
    N, K = W.shape
    a = _lib.GemmNTArgs()
    a.mfma_f16 = ops._MFMA_F16[0]; a.tile_hint = 0
    a.A = ops._p(A); a.lda = K; a.W = ops._p(W); a.ldw = K
    a.M, a.N, a.K = M, N, K
    a.a_mode = ops.A_PLAIN
    if pro is not None:
        a.a_mode = ops.A_AFFINE_LRELU
        a.p_scale = ops._p(pro[0]); a.p_shift = ops._p(pro[1]); a.p_slope = float(pro[2])
    a.p_group_rows = group_rows
    a.epi_mode = ops.EPI_LINEAR
    dummy = torch.empty(16, device="cuda")
    a.stats = ops._p(dummy)
    if pool:
        a.pool_val = ops._p(dummy); a.pool_arg = ops._p(dummy)
    else:
        a.Y = ops._p(dummy); a.ldy = N
    return int(_lib.load().spgan_gemm_nt_col_blocks(C.byref(a)))


def _reference(mode, A, W, b, bn, groups, pro):
    """float64 model of the grouped layer; "f16": of the fp16-rounded operands (the prologue evaluated first, as the kernels stage them)."""
    d = lambda t: t.double()
    bn64 = tuple(d(t) for t in bn)
    if mode != "f16":
        return km.gemm_bn_groups(d(A), d(W), d(b), bn64, groups, pro=None if pro is None else (d(pro[0]), d(pro[1]), pro[2]))
    Mg = A.shape[0] // groups
    opd = A
    if pro is not None:
        sc, sh = pro[0].repeat_interleave(Mg, 0), pro[1].repeat_interleave(Mg, 0)
        v = A * sc + sh
        opd = torch.where(v > 0, v, v * pro[2])
    return km.gemm_bn_groups(d(opd.half()), d(W.half()), d(b), bn64, groups)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("groups,Mg,N,K,straddles", GROUP_SHAPES)
def test_gemm_bn_groups_equal_separate_calls(ops, mode, groups, Mg, N, K, straddles):
    """ops.gemm_bn_groups against `groups` separate gemm_nt(bn=) / gemm_bn_pool calls, bit for bit: activations, the four BatchNorm vectors,
    the running statistics, pooled values, arg-max rows and their activations -- and both argument blocks name the same kernel."""
    M = groups * Mg
    A, W, b = rnd("om.A%d.%d" % (M, K), (M, K)), rnd("om.W%d.%d" % (N, K), (N, K), 0.1), rnd("om.b%d" % N, (N,))
    A = A + torch.arange(groups, device="cuda").repeat_interleave(Mg).view(M, 1) * 0.5          # the passes have different statistics
    sc, sh = rnd("om.sc%d.%d" % (groups, K), (groups, K)).abs() + 0.5, rnd("om.sh%d.%d" % (groups, K), (groups, K), 0.3)
    gamma, beta = rnd("om.ga%d" % N, (N,)).abs() + 0.5, rnd("om.be%d" % N, (N,), 0.1)
    rows = 2048
    with operands(ops, mode):
        for pro in (None, (sc, sh, 0.01)):
            pg = [None if pro is None else (pro[0][g].contiguous(), pro[1][g].contiguous(), pro[2]) for g in range(groups)]
            for pool in (False, True):
                grouped = _col_blocks(ops, A, W, M, pro, Mg, pool)
                assert grouped == _col_blocks(ops, A[:Mg], W, Mg, pg[0], 0, pool), "grouped launch and its passes select different kernels"
                if straddles == mode:       # the shape does straddle this mode's rule: the rows of the whole launch would pick another kernel
                    assert _col_blocks(ops, A, W, M, pg[0], 0, pool) != grouped
            rm, rv = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
            Y, out = ops.gemm_bn_groups(A, W, b, (gamma, beta, rm, rv), groups, pro=pro)
            rm2, rv2 = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
            for g in range(groups):
                y1, st1 = ops.gemm_nt(A[g * Mg:(g + 1) * Mg], W, b, pro=pg[g], bn=(gamma, beta, rm2, rv2))
                assert torch.equal(Y[g * Mg:(g + 1) * Mg], y1), "pass %d: activations differ" % g
                for q in range(4):
                    assert torch.equal(out[q, g], st1[q]), (g, q)
            assert torch.equal(rm, rm2) and torch.equal(rv, rv2)
            bn0 = (gamma, beta, torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"))
            Ym, outm = _reference(mode, A, W, b, bn0, groups, pro)
            if mode == "f16":
                close(Y, Ym, rtol=2e-5, atol=1e-5, what="Y vs float64 of fp16 operands")
            else:
                close(Y, Ym, rtol=5e-5, what="Y vs float64")
            close(out, outm, rtol=2e-4, atol=2e-5, what="bn vs float64")
            del Y, Ym
            # rows > 0: the Discriminator's last conv layer (Y not stored, max-pool over `rows` rows)
            rm, rv = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
            out, pooled, arg, yarg = ops.gemm_bn_groups(A, W, b, (gamma, beta, rm, rv), groups, pro=pro, rows=rows, slope=0.01)
            rm2, rv2 = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
            Bg = Mg // rows
            for g in range(groups):
                _, st1, p1, a1, ya1 = ops.gemm_bn_pool(A[g * Mg:(g + 1) * Mg], W, b, (gamma, beta, rm2, rv2), rows, 0.01, pro=pg[g])
                sl = slice(g * Bg, (g + 1) * Bg)
                assert torch.equal(pooled[sl], p1) and torch.equal(arg[sl], a1) and torch.equal(yarg[sl], ya1), "pass %d: pooling differs" % g
                for q in range(4):
                    assert torch.equal(out[q, g], st1[q]), (g, q)
            assert torch.equal(rm, rm2) and torch.equal(rv, rv2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [4, 8, 16])
def test_discriminator_grouped_passes_equal_separate_calls(sp, mode, B):   # noqa: F811
    """The Discriminator's grouped forms (forward_stacks_grouped, forward_stack_after_stats_pass) at N = 2048 points, where layers of the
    grouped conv stack straddle a selection rule (bf16x3: mlps.3 at B = 8, mlps.6 at B = 4; f16: mlps.6 at B = 16, fc2.0 at B = 4): logits,
    input and parameter gradients and buffers of the separate calls, bit for bit."""
    with operands(sp.ops, mode):
        grouped_passes_equal_separate_calls(sp, B, 2048)


# ------------------------------------------------------------------------------------------------------------------ split-bf16 range
BF16_MAX = km.BF16_MAX
EDGES = np.array([0x7F7F0000, 0x7F7F0001, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF], dtype=np.uint32)   # BF16_MAX .. FLT_MAX
INF = float("inf")


def _bits(b):
    return torch.from_numpy(np.asarray(b, dtype=np.uint32).view(np.float32).copy())


def _split_classes(N, K, seed):
    """[N, K] fp32: every binade from 2^-100 (all three planes normal) to 2^127 with random and all-ones mantissas, the bf16 overflow point's
    neighbourhood, FLT_MAX, +-0, +-inf and NaN; both signs."""
    g = np.random.default_rng(seed)
    e = g.integers(-100 + 127, 255, (N, K)).astype(np.uint32)
    mant = g.integers(0, 1 << 23, (N, K), dtype=np.uint32)
    mant[:, ::5] = (1 << 23) - 1
    bits = (e << 23) | mant
    bits[:, 1::7] = g.integers(0x7F000000, 0x7F800000, bits[:, 1::7].shape, dtype=np.uint32)       # the top binade
    bits[:, 3::11] = EDGES[g.integers(0, EDGES.size, bits[:, 3::11].shape)]
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000], dtype=np.uint32)
    bits[::3, 2::13] = special[g.integers(0, special.size, bits[::3, 2::13].shape)]
    bits ^= g.integers(0, 2, (N, K), dtype=np.uint32) << 31
    return _bits(bits)


def test_split_image_range(ops):
    """ops.split_image (spgan_split_bf16x3_image) of values over the whole fp32 range equals its model (kernel_model.split_image) bit for bit;
    where the model's plane holds a NaN only NaN-ness is compared (the payload is not part of the contract)."""
    W = _split_classes(256, 96, 3).cuda()
    got = ops.split_image(W).view(torch.bfloat16)
    ref = km.split_image(W).view(torch.bfloat16)
    nan = torch.isnan(ref)
    assert nan.any() and torch.equal(torch.isnan(got), nan), "NaN planes differ"
    bad = got.view(torch.int16)[~nan] != ref.view(torch.int16)[~nan]
    assert not bad.any(), "%d of %d plane values differ from the model" % (bad.sum().item(), bad.numel())


def _one_product_operands(seed):
    """A [256, 64], W [256, 64] (exactly representable) whose product has ONE non-zero term per output (row m of A is non-zero at k = m % 64
    only): every output is a single a*b, reproduced within 4 * 2^-24 |a*b| when finite.  Magnitudes per k band: k < 16 both 2^-20..2^20;
    16 <= k < 40 A up to 2^127 (the top binade, the bf16 overflow point, FLT_MAX), W 2^-40..2^-3; k >= 40 the other way round -- |a*b| <= 2^126.
    Rows 192..223 / columns 240..251 hold the non-finite values: +-inf / NaN in A (at k 8..15), dense positive rows (k < 16), and W rows with
    +inf at k = 3, -inf at k = 5, NaN at k = 7.  A's and W's infinities never meet in one product (inf * inf is NaN in the split: split_bf16.hpp)."""
    g = torch.Generator().manual_seed(seed)
    M, N, K = 256, 256, 64
    mant = lambda shape: 1.0 + torch.randint(0, 2 ** 23, shape, generator=g).double() / 2 ** 23
    full = 2.0 - 2.0 ** -23
    k = torch.arange(K)
    lo_a = torch.where(k < 16, -20, torch.where(k < 40, 100, -40)); hi_a = torch.where(k < 16, 20, torch.where(k < 40, 127, -3))
    lo_w = torch.where(k < 16, -20, torch.where(k < 40, -40, 100)); hi_w = torch.where(k < 16, 20, torch.where(k < 40, -3, 127))
    expo = lambda lo, hi, shape: (lo + (torch.rand(shape, generator=g) * (hi - lo + 1)).floor().clamp(max=hi - lo)).double()
    sign = lambda shape: torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    km_ = k.repeat(M // K)[:M]                                                   # k of row m
    A = torch.zeros(M, K, dtype=torch.float64)
    ea = expo(lo_a[km_], hi_a[km_], (M,))
    A[torch.arange(M), km_] = mant((M,)) * 2.0 ** ea * sign((M,))
    A[torch.arange(0, M, 7), km_[::7]] = full * 2.0 ** ea[::7]
    top = [m for m in range(M) if 16 <= km_[m] < 40][:len(EDGES) * 2]
    A[top, km_[top]] = torch.cat([_bits(EDGES), -_bits(EDGES)]).double()
    W = mant((N, K)) * 2.0 ** expo(lo_w[None, :], hi_w[None, :], (N, K)) * sign((N, K))
    W[::5] = full * 2.0 ** expo(lo_w[None, :], hi_w[None, :], (N // 5 + 1, K))[:W[::5].shape[0]]
    for i, n in enumerate(range(0, 48)):
        W[n, 40 + i % 6] = (1 if i % 2 else -1) * float(_bits(EDGES[i % 6]))
    # non-finite operands
    for r0, v in ((192, INF), (200, -INF), (208, float("nan"))):
        A[r0:r0 + 8] = 0
        A[torch.arange(r0, r0 + 8), 8 + torch.arange(8)] = v
    A[216:224] = 0
    A[216:224, :16] = mant((8, 16)) * 2.0 ** expo(-4, 4, (8, 16))
    W[240:252, :16] = mant((12, 16)) * 2.0 ** expo(-4, 4, (12, 16)) * sign((12, 16))
    W[240:244, 3], W[244:248, 5], W[248:252, 7] = INF, -INF, float("nan")
    Af, Wf = A.float(), W.float()
    assert torch.equal(Af.double().isnan(), A.isnan()) and torch.equal(Af.double()[~A.isnan()], A[~A.isnan()])
    assert torch.equal(Wf.double().isnan(), W.isnan()) and torch.equal(Wf.double()[~W.isnan()], W[~W.isnan()])
    fin = torch.ones(M, N, dtype=torch.bool)
    fin[192:224] = False; fin[:, 240:252] = False
    ref = (A[:, None, :] * W[None, :, :]).sum(-1)                                 # float64, term by term (IEEE inf / NaN rules)
    return Af, Wf, ref, fin


def _pattern(x):
    x = x.double().cpu()
    return torch.stack([torch.isnan(x), x == INF, x == -INF])


def _check_range(got, f32, ref, fin, what):
    assert torch.equal(_pattern(f32), _pattern(ref)), what + ": the fp32 mode's NaN / inf pattern is not the exact product's"
    p, q = _pattern(got), _pattern(f32)
    assert torch.equal(p, q), "%s: NaN / inf pattern differs from the fp32 mode's at %d outputs (NaN %d, +inf %d, -inf %d against %d, %d, %d)" % (
        what, (p != q).any(0).sum().item(), *p.sum((1, 2)).tolist(), *q.sum((1, 2)).tolist())
    g, r = got.double().cpu()[fin], ref[fin]
    assert torch.isfinite(g).all(), what + ": a finite product came out non-finite"
    rel = ((g - r).abs() / r.abs()).max().item()
    assert rel <= 4 * 2.0 ** -24, (what, rel / 2.0 ** -24)


@pytest.mark.parametrize("route", ["wide3", "wide3+image", "split128"])
def test_gemm_nt_bf16x3_range(ops, route):
    """gemm_nt in the bf16x3 mode over fp32's whole range (_one_product_operands): through the 256-row split kernel (tile hint 2), with and
    without W's pre-split image, and the 128-row split kernel (hint 1)."""
    A, W, ref, fin = _one_product_operands(17)
    A, W = A.cuda(), W.cuda()
    f32 = ops.gemm_nt(A, W)
    with operands(ops, "bf16x3"):
        ops.w_image_provider = (lambda Wt: ops.split_image(Wt)) if route == "wide3+image" else None
        try:
            with ops.nt_tile_hint(1 if route == "split128" else 2):
                got = ops.gemm_nt(A, W)
        finally:
            ops.w_image_provider = None
    _check_range(got, f32, ref, fin, route)


def test_gemm_tn_bf16x3_range(ops):
    """gemm_tn (the weight gradient) in the bf16x3 mode through its split-bf16 kernel (gemm_tn_wide3.hip: ops.TN_SPLIT_BF16, >= TN_LP_MIN_ROWS
    rows): the same one-product operands, row k * 256 of the [16384, 256] operands holding column k of A and W."""
    A, W, ref, fin = _one_product_operands(23)
    M = 16384
    At = torch.zeros(M, 256); Bt = torch.zeros(M, 256)
    At[::256] = A.t(); Bt[::256] = W.t()
    At, Bt = At.cuda(), Bt.cuda()
    f32 = ops.gemm_tn(At, Bt)
    was = ops.TN_SPLIT_BF16[0]
    ops.TN_SPLIT_BF16[0] = True
    try:
        with operands(ops, "bf16x3"):
            got = ops.gemm_tn(At, Bt)
    finally:
        ops.TN_SPLIT_BF16[0] = was
    _check_range(got, f32, ref, fin, "gemm_tn")
