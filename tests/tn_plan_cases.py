"""The shapes and argument blocks on which tests/test_tn_plan_cpu.py and tests/golden/make_golden_tn_plan.py ask the gemm_tn / gemm_dual
selection queries.

Deterministic, no GPU: the queries never read through a pointer of the block, so integers stand in for addresses.  Every address and size
choice of those tests is made here and nowhere else.

  shapes()   every (M, Na, Nb) of the grid.  ask_shape() asks the seven shape-only queries that exist since before the plan (the fixture's
             columns, SHAPE_QUERIES): both sides of every threshold of the split rules, the skinny rule, the three tile widths, the wide
             tile configurations and gemm_dual's shape test.
  blocks()   spgan_gemm_tn_args blocks: a reduced shape set x operand mode x operand form.  A case is a dict {"name", "form", "fields"}:
             `fields` are the members that differ from zero.  Every block is one spgan_gemm_tn's argument checks accept, but for the 16-bit
             forms that the plan itself reports as invalid.
"""
import ctypes as C

A_PLAIN, A_AFFINE, A_EDGE = 0, 1, 2

MS = (1, 31, 32, 63, 64, 100, 1000, 1024, 4096, 8192, 20000, 65536, 196608, 655360, 2 ** 24 - 1)
NS = (1, 3, 4, 5, 32, 33, 64, 65, 128, 192, 256, 384, 512, 1024, 1280, 2048, 2049)
LPS = (0, 1, 2)
EKS = (0, 5, 10)

SHAPE_QUERIES = (("ws_bytes", "splits", "reduce_blocks") + tuple("%s_lp%d" % (q, lp) for lp in LPS for q in ("ws_bytes", "splits", "reduce_blocks"))
                 + tuple("dual_wgs_ek%d" % ek for ek in EKS) + ("dual_rows_per_wg",))


def shapes():
    return [(M, Na, Nb) for M in MS for Na in NS for Nb in NS]


def shape_signatures(lib):
    """restype / argtypes of the seven queries (a library loaded without the package's table: the parent commit's)."""
    I, SZ = C.c_int, C.c_size_t
    for name, res, args in (("spgan_gemm_tn_ws_bytes", SZ, [I] * 3), ("spgan_gemm_tn_splits", I, [I] * 3), ("spgan_gemm_tn_ws_bytes_lp", SZ, [I] * 4),
                            ("spgan_gemm_tn_splits_lp", I, [I] * 4), ("spgan_splitk_reduce_blocks", I, [I] * 3), ("spgan_gemm_dual_wgs", I, [I] * 4),
                            ("spgan_gemm_dual_rows_per_wg", I, [I] * 3)):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args


def ask_shape(lib, M, Na, Nb):
    """The answers of one shape in the order of SHAPE_QUERIES."""
    s = lib.spgan_gemm_tn_splits(M, Na, Nb)
    out = [lib.spgan_gemm_tn_ws_bytes(M, Na, Nb), s, lib.spgan_splitk_reduce_blocks(s, Na, Nb)]
    for lp in LPS:
        s = lib.spgan_gemm_tn_splits_lp(M, Na, Nb, lp)
        out += [lib.spgan_gemm_tn_ws_bytes_lp(M, Na, Nb, lp), s, lib.spgan_splitk_reduce_blocks(s, Na, Nb)]
    out += [lib.spgan_gemm_dual_wgs(M, Na, Nb, ek) for ek in EKS]
    out.append(lib.spgan_gemm_dual_rows_per_wg(M, Na, Nb))
    return out


# ----------------------------------------------------------------------------------------------- argument blocks
POINTERS = ("A", "B", "C", "ws", "p_scale", "p_shift", "e_idx", "e_bias", "a_scale", "a_shift", "a_sp_val", "a_sp_arg", "A2", "a_scale2", "a_colsum_ws")
ADDR = {name: 0x10000000 * (i + 1) for i, name in enumerate(POINTERS)}   # 16-byte aligned, all different

BLOCK_MS = (100, 4096, 8192)          # no multiple of 32 (never the wide kernel), multiples of it below and at the Python side's TN_LP_MIN_ROWS
BLOCK_NS = (3, 4, 5, 32, 64, 65, 128, 256, 384, 2049)

_AFF = dict(p_scale=ADDR["p_scale"], p_shift=ADDR["p_shift"])
_ASC = dict(a_scale=ADDR["a_scale"], a_shift=ADDR["a_shift"])
_SP = dict(_ASC, a_sp_val=ADDR["a_sp_val"], a_sp_arg=ADDR["a_sp_arg"], a_sp_rows=50, defer_reduce=0)


def _forms(Na):
    """name -> the fields beside the plain block's.  (A2: lda2 = Na.)"""
    two = dict(_ASC, A2=ADDR["A2"], lda2=Na, a_scale2=ADDR["a_scale2"])
    odd = Na + (-Na) % 4 + 2            # a leading dimension >= Na that is no multiple of 4
    return (
        ("plain", {}),
        ("affine", dict(_AFF, b_mode=A_AFFINE, p_slope=0.2)),
        ("affine_slope_out", dict(_AFF, b_mode=A_AFFINE, p_slope=1.5)),
        ("edge", dict(_AFF, b_mode=A_EDGE, p_slope=0.2, e_idx=ADDR["e_idx"], e_k=10, e_bias=ADDR["e_bias"])),
        ("a_scale", dict(_ASC)),
        ("a_scale.affine", dict(_ASC, **dict(_AFF, b_mode=A_AFFINE, p_slope=0.2))),
        ("A2", two),
        ("a_lrelu", dict(_ASC, a_lrelu=1, a_slope=0.2)),
        ("a_lrelu_slope_out", dict(_ASC, a_lrelu=1, a_slope=-0.5)),
        ("a_sp", dict(_SP)),
        ("a_sp.affine", dict(_SP, **dict(_AFF, b_mode=A_AFFINE, p_slope=0.2))),
        ("colsum", dict(a_colsum_ws=ADDR["a_colsum_ws"])),
        ("colsum.a_lrelu", dict(_ASC, a_lrelu=1, a_slope=0.2, a_colsum_ws=ADDR["a_colsum_ws"])),
        ("b_half", dict(b_half=1)),
        ("b_half.colsum", dict(b_half=1, a_colsum_ws=ADDR["a_colsum_ws"])),
        ("b_half.affine", dict(_AFF, b_mode=A_AFFINE, p_slope=0.2, b_half=1)),
        ("b_half.a_sp", dict(_SP, b_half=1)),
        ("b_half.off_B", dict(b_half=1, B=ADDR["B"] + 4)),
        ("a_half", dict(a_half=1)),
        ("a_half.A2", dict(two, a_half=1)),
        ("a_half.a_sp", dict(_SP, a_half=1)),
        ("a_half.odd_lda", dict(a_half=1, lda=odd)),
        ("off_A", dict(A=ADDR["A"] + 4)),
        ("off_B", dict(B=ADDR["B"] + 4)),
        ("off_A2", dict(two, A2=ADDR["A2"] + 4)),
        ("odd_lda", dict(lda=odd)),
        ("odd_lda2", dict(two, lda2=odd)),
    )


def blocks():
    out = []
    for M in BLOCK_MS:
        for Na in BLOCK_NS:
            for Nb in BLOCK_NS:
                for lp in LPS:
                    for form, more in _forms(Na):
                        f = dict(A=ADDR["A"], lda=Na, B=ADDR["B"], ldb=Nb, C=ADDR["C"], ldc=Nb, M=M, Na=Na, Nb=Nb, b_mode=A_PLAIN, ws=ADDR["ws"],
                                 ws_bytes=1 << 40, defer_reduce=1, mfma_lp=lp)
                        f.update(more)
                        out.append({"name": "%s.%dx%dx%d.lp%d" % (form, M, Na, Nb, lp), "form": form, "fields": f})
    assert len({c["name"] for c in out}) == len(out)
    return out


def to_args(fields, binding=None):
    """The spgan_gemm_tn_args block of a case."""
    if binding is None:
        from spgan import _lib as binding
    a = binding.GemmTNArgs()
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def plan(lib, fields, binding=None):
    """spgan_gemm_tn_kernel and the whole plan (spgan_gemm_tn_plan: a tuple in the order of spgan._lib.TN_PLAN_FIELDS) of one block."""
    a = to_args(fields, binding)
    out = (C.c_int32 * 9)()
    assert lib.spgan_gemm_tn_plan(C.byref(a), out) == 0
    return lib.spgan_gemm_tn_kernel(C.byref(a)), tuple(out)
