"""The argument blocks on which tests/test_nt_plan_cpu.py and tests/golden/make_golden_nt_plan.py ask the gemm_nt selection queries.

Deterministic, no GPU: the queries never read through a pointer of the block, so integers stand in for addresses.  Every address and size
choice of those tests is made here and nowhere else.  A case is a dict {"name", "group", "fields"}: `fields` are the members of
spgan_gemm_nt_args that differ from zero.  Groups:

  aligned       every address 16-byte aligned.  The five queries of the parent commit (the fixture) are pinned exactly on these.
  launch_first  aligned blocks of the two argument forms for which the parent's spgan_gemm_nt_col_blocks did not follow the parent's own
                launch (the ADAIN epilogue, whose only 128-row form is 128 columns wide whatever K is; fp16-stored A, which the launch
                sends to the 128-row kernels before it asks about 256 x 256 tiles).  The other four queries are pinned on the fixture.
  misaligned    exactly one of A, W, p_scale, e_bias, A2, sp_val, w_image offset by 4 bytes.

cases() returns them with a dict that maps the name of every grouped block (three passes as one product, p_group_rows = M / 3) to the name
of its single pass.
"""
import ctypes as C

A_PLAIN, A_AFFINE, A_EDGE = 0, 1, 2
EPI_LINEAR, EPI_MASK_OUT, EPI_BNBWD, EPI_EDGE_BNBWD, EPI_ADAIN = 0, 1, 2, 3, 4

# both sides of every threshold of the rules
MS = (32, 64, 65, 128, 256, 8192, 32512, 32768, 65280, 65536, 196608)
NS = (8, 32, 64, 128, 256, 1024, 1280)
KS = (3, 4, 32, 64, 96, 128, 160, 256, 512, 1024)
MFMA = (0, 1, 2)
HINTS = (0, 1, 2)
# the smaller grids of everything but the plain linear product
MS_CORE = (32, 64, 65, 256, 8192, 32512, 65536)
NS_CORE = (32, 64, 128, 256, 1024)
KS_CORE = (3, 4, 32, 64, 128, 512)
SHAPES_OPT = [(M, N, K) for M in (64, 256, 8192, 65536) for N in (64, 256, 1024) for K in (32, 128, 512)]

POINTERS = ("A", "W", "Y", "p_scale", "p_shift", "e_idx", "e_bias", "bias", "rowbias", "stats", "ref", "b_scale", "b_shift", "b_mean", "b_invstd",
            "e_bias2", "sp_val", "sp_arg", "pool_val", "pool_arg", "A2", "p_scale2", "w_image", "gout_add", "gout_scale", "ad_x", "ad_mean", "ad_var",
            "tail.out0", "tail.out1")
ADDR = {name: 0x10000000 * (i + 1) for i, name in enumerate(POINTERS)}   # 16-byte aligned, all different
OFFSET_POINTERS = ("A", "W", "p_scale", "e_bias", "A2", "sp_val", "w_image")


def _block(M, N, K, mfma=0, hint=0, a_mode=A_PLAIN, epi=EPI_LINEAR, **more):
    f = dict(A=ADDR["A"], lda=K, W=ADDR["W"], ldw=K, Y=ADDR["Y"], ldy=N, M=M, N=N, K=K, a_mode=a_mode, epi_mode=epi, mfma_f16=mfma, tile_hint=hint)
    if a_mode != A_PLAIN:
        f.update(p_scale=ADDR["p_scale"], p_shift=ADDR["p_shift"], p_slope=0.2)
    if a_mode == A_EDGE:
        f.update(e_idx=ADDR["e_idx"], e_k=10, e_bias=ADDR["e_bias"])
    if epi in (EPI_MASK_OUT, EPI_BNBWD, EPI_EDGE_BNBWD):
        f.update(ref=ADDR["ref"], ld_ref=N, b_slope=0.2)
    if epi in (EPI_BNBWD, EPI_EDGE_BNBWD):
        f.update(b_scale=ADDR["b_scale"], b_shift=ADDR["b_shift"], b_mean=ADDR["b_mean"], b_invstd=ADDR["b_invstd"], stats=ADDR["stats"])
    if epi == EPI_EDGE_BNBWD:
        f.update(e_idx=ADDR["e_idx"], e_k=10, e_bias2=ADDR["e_bias2"])
    if epi == EPI_ADAIN:
        f.update(ldy=N // 2, ad_x=ADDR["ad_x"], ad_ldx=N // 2, ad_rows=M, ad_mean=ADDR["ad_mean"], ad_var=ADDR["ad_var"], ad_eps=1e-5, ad_slope=0.2)
    f.update(more)
    return f


def _sparse(M):
    return dict(sp_val=ADDR["sp_val"], sp_arg=ADDR["sp_arg"], sp_rows=256 if M % 256 == 0 else M)


def _two(K):
    return dict(A2=ADDR["A2"], lda2=K, p_scale2=ADDR["p_scale2"])


# every (a_mode, A2, sp_val) x epi_mode pair spgan_gemm_nt accepts
MODE_PAIRS = (
    ("plain.linear", A_PLAIN, EPI_LINEAR, None), ("affine.linear", A_AFFINE, EPI_LINEAR, None), ("sparse.linear", A_AFFINE, EPI_LINEAR, "sp"),
    ("two.linear", A_AFFINE, EPI_LINEAR, "A2"), ("edge.linear", A_EDGE, EPI_LINEAR, None), ("plain.mask", A_PLAIN, EPI_MASK_OUT, None),
    ("plain.bnbwd", A_PLAIN, EPI_BNBWD, None), ("affine.bnbwd", A_AFFINE, EPI_BNBWD, None), ("sparse.bnbwd", A_AFFINE, EPI_BNBWD, "sp"),
    ("two.bnbwd", A_AFFINE, EPI_BNBWD, "A2"), ("plain.edge_bnbwd", A_PLAIN, EPI_EDGE_BNBWD, None), ("two.edge_bnbwd", A_AFFINE, EPI_EDGE_BNBWD, "A2"),
    ("plain.adain", A_PLAIN, EPI_ADAIN, None),
)


def _pair_block(pair, M, N, K, mfma, hint, **more):
    _, a_mode, epi, extra = pair
    f = _block(M, N, K, mfma, hint, a_mode, epi)
    if extra == "sp":
        f.update(_sparse(M))
    if extra == "A2":
        f.update(_two(K))
    f.update(more)
    return f


def _pair_accepts(pair, M, N, K, mfma):
    """What spgan_gemm_nt's argument checks ask of the sizes of a mode pair (A2: M > 64; ADAIN: fp32 operands, M > 64, N % 64 == 0, K % 4 == 0)."""
    _, _, epi, extra = pair
    if extra == "A2" and M <= 64:
        return False
    if epi == EPI_ADAIN and (mfma != 0 or M <= 64 or N % 64 or K % 4):
        return False
    return True


def cases():
    out, single_of = [], {}

    def add(group, name, fields):
        out.append({"name": name, "group": group, "fields": fields})
        return name

    def tag(M, N, K, mfma, hint):
        return "%dx%dx%d.m%d.h%d" % (M, N, K, mfma, hint)

    # 1. the plain linear product on the whole size grid
    for M in MS:
        for N in NS:
            for K in KS:
                for mfma in MFMA:
                    for hint in HINTS:
                        add("aligned", "sweep." + tag(M, N, K, mfma, hint), _block(M, N, K, mfma, hint))
    # 2. every accepted mode pair
    for pair in MODE_PAIRS:
        adain = pair[2] == EPI_ADAIN
        for M in MS_CORE:
            for N in NS_CORE:
                for K in KS_CORE:
                    for mfma in MFMA:
                        for hint in HINTS:
                            if _pair_accepts(pair, M, N, K, mfma):
                                add("launch_first" if adain else "aligned", pair[0] + "." + tag(M, N, K, mfma, hint), _pair_block(pair, M, N, K, mfma, hint))
    # 3. options of the linear epilogue (and what goes with them), on plain and activation operands
    for M, N, K in SHAPES_OPT:
        for mfma in MFMA:
            for hint in HINTS:
                t = tag(M, N, K, mfma, hint)
                for pair in MODE_PAIRS[:2]:
                    p = pair[0]
                    add("aligned", "stats.%s.%s" % (p, t), _pair_block(pair, M, N, K, mfma, hint, stats=ADDR["stats"]))
                    add("aligned", "stats_noY.%s.%s" % (p, t), _pair_block(pair, M, N, K, mfma, hint, stats=ADDR["stats"], Y=0))
                    add("aligned", "act.%s.%s" % (p, t), _pair_block(pair, M, N, K, mfma, hint, act=1, act_slope=0.2, bias=ADDR["bias"]))
                    for rpg in (1, 256, 128):   # a row per row, per 256 rows (whole 256-row tiles), per 128 rows only
                        add("aligned", "rowbias%d.%s.%s" % (rpg, p, t),
                            _pair_block(pair, M, N, K, mfma, hint, rowbias=ADDR["rowbias"], rows_per_group=rpg, ld_rowbias=N))
                    if M > 64:
                        pool = dict(pool_val=ADDR["pool_val"], pool_arg=ADDR["pool_arg"], stats=ADDR["stats"])
                        add("aligned", "pool.%s.%s" % (p, t), _pair_block(pair, M, N, K, mfma, hint, **pool))
                        add("aligned", "pool_noY.%s.%s" % (p, t), _pair_block(pair, M, N, K, mfma, hint, Y=0, **pool))
                    if M > 64 and mfma == 1:   # 16-bit result storage: fp16 operand mode only
                        add("aligned", "y_half.%s.%s" % (p, t), _pair_block(pair, M, N, K, mfma, hint, y_half=1))
                        add("aligned", "y_bf16.%s.%s" % (p, t), _pair_block(pair, M, N, K, mfma, hint, y_bf16=1))
                    if mfma == 2:
                        add("aligned", "w_image.%s.%s" % (p, t), _pair_block(pair, M, N, K, mfma, hint, w_image=ADDR["w_image"]))
                if mfma == 2:
                    add("aligned", "w_image.affine.bnbwd." + t, _pair_block(MODE_PAIRS[7], M, N, K, mfma, hint, w_image=ADDR["w_image"]))
                    add("aligned", "gout.affine.bnbwd." + t, _pair_block(MODE_PAIRS[7], M, N, K, mfma, hint, gout_add=ADDR["gout_add"], ld_gout_add=N,
                                                                          gout_scale=ADDR["gout_scale"]))
                    add("aligned", "sparse128.linear." + t, _pair_block(MODE_PAIRS[2], M, N, K, mfma, hint, sp_rows=128))
                if mfma == 0:
                    add("aligned", "sparse128.bnbwd." + t, _pair_block(MODE_PAIRS[8], M, N, K, mfma, hint, sp_rows=128))
                    if M > 64:
                        add("launch_first", "pool.plain.adain." + t, _pair_block(MODE_PAIRS[12], M, N, K, mfma, hint, pool_val=ADDR["pool_val"],
                                                                                  pool_arg=ADDR["pool_arg"], ad_rows=128))
                if M > 64 and mfma == 1:   # 16-bit operand storage
                    add("launch_first", "a_half.plain.linear." + t, _block(M, N, K, mfma, hint, a_half=1))
                    add("aligned", "a_half.two.edge_bnbwd." + t, _pair_block(MODE_PAIRS[11], M, N, K, mfma, hint, a_half=1))
                add("aligned", "odd_lda.plain.linear." + t, _block(M, N, K, mfma, hint, lda=K + 2))   # aligned base, rows that are not
                add("aligned", "batch4.plain.linear." + t, _block(M, N, K, mfma, hint, batch=4, batch_stride_a=M * K, batch_stride_w=N * K, batch_stride_y=M * N))
    # 4. the column tail: accepted with M <= 64 on the column-owning kernel; no such kernel for K = 3 (unaligned rows) or M > 64
    for M in (32, 64, 256):
        for N in (8, 64, 256):
            for K in (3, 32, 512):
                for mfma in MFMA:
                    for pair in MODE_PAIRS[:2] + MODE_PAIRS[6:8]:
                        mode1 = pair[2] != EPI_LINEAR
                        tail = {"stats": ADDR["stats"], "tail.enabled": 1, "tail.mode": 1 if mode1 else 0, "tail.out0": ADDR["tail.out0"],
                                "tail.out1": ADDR["tail.out1"]}
                        add("aligned", "tail.%s.%s" % (pair[0], tag(M, N, K, mfma, 0)), _pair_block(pair, M, N, K, mfma, 0, **tail))
    # 5. three passes as one product (p_group_rows = M / 3) beside their single pass
    for Mg in (128, 256, 8192, 32512, 32768, 65280, 65536):
        for N in (64, 128, 256, 1024):
            for K in (32, 64, 128, 256, 512):
                for mfma in MFMA:
                    for hint in HINTS:
                        for pair in MODE_PAIRS[:2] + MODE_PAIRS[5:8]:
                            for opt, more in (("", {}), (".image", dict(w_image=ADDR["w_image"]))):
                                if opt and mfma != 2:
                                    continue
                                if pair[2] == EPI_LINEAR:
                                    more = dict(more, stats=ADDR["stats"])
                                one = add("aligned", "pass%s.%s.%s" % (opt, pair[0], tag(Mg, N, K, mfma, hint)), _pair_block(pair, Mg, N, K, mfma, hint, **more))
                                three = add("aligned", "grouped%s.%s.%s" % (opt, pair[0], tag(3 * Mg, N, K, mfma, hint)),
                                            _pair_block(pair, 3 * Mg, N, K, mfma, hint, p_group_rows=Mg, **more))
                                single_of[three] = one
    # 6. one address 4 bytes off
    for M, N, K in ((32, 64, 32), (256, 64, 32), (8192, 256, 128), (8192, 256, 512), (65536, 1024, 256), (65536, 256, 512)):
        for mfma in MFMA:
            for hint in (0, 2):
                t = tag(M, N, K, mfma, hint)
                for which in OFFSET_POINTERS:
                    if which in ("A", "W"):
                        users = MODE_PAIRS[:2] + MODE_PAIRS[5:8]
                    elif which == "p_scale":
                        users = (MODE_PAIRS[1], MODE_PAIRS[4], MODE_PAIRS[7])
                    elif which == "e_bias":
                        users = (MODE_PAIRS[4],)
                    elif which == "A2":
                        users = (MODE_PAIRS[3], MODE_PAIRS[9], MODE_PAIRS[11])
                    elif which == "sp_val":
                        users = (MODE_PAIRS[2], MODE_PAIRS[8])
                    else:
                        users = MODE_PAIRS[:2] + (MODE_PAIRS[7],)
                    for pair in users:
                        if not _pair_accepts(pair, M, N, K, mfma) or (which == "w_image" and mfma != 2):
                            continue
                        f = _pair_block(pair, M, N, K, mfma, hint, **({"w_image": ADDR["w_image"]} if which == "w_image" else {}))
                        f[which] += 4
                        add("misaligned", "off_%s.%s.%s" % (which, pair[0], t), f)
    assert len({c["name"] for c in out}) == len(out)
    return out, single_of


def to_args(fields, binding=None):
    """The spgan_gemm_nt_args block of a case (binding: the spgan._lib module, where the caller has loaded it without the package)."""
    if binding is None:
        from spgan import _lib as binding
    a = binding.GemmNTArgs()
    for k, v in fields.items():
        if k.startswith("tail."):
            setattr(a.tail, k[5:], v)
        else:
            setattr(a, k, v)
    return a


def dt_block(fields):
    """The argument block spgan_edge_attend_bwd_dt_selected(A, lda, W, ldw, M, 10, K, tile_hint) asks about: the chain's product
    dT = gemm_nt(dout, WoT), a plain linear fp32 product [M, K] x [10 K, K]^T (include/spgan_hip.h)."""
    return dict(A=fields["A"], lda=fields["lda"], W=fields["W"], ldw=fields["ldw"], Y=fields["A"], ldy=10 * fields["K"], M=fields["M"], N=10 * fields["K"],
                K=fields["K"], a_mode=A_PLAIN, epi_mode=EPI_LINEAR, mfma_f16=0, tile_hint=fields["tile_hint"])


QUERIES = ("col_blocks", "owns_columns", "y16_ok", "uses_w_image", "dt_selected")


def ask(lib, fields, binding=None):
    """The five queries that exist since before the plan, on one case."""
    a = to_args(fields, binding)
    r = C.byref(a)
    return (lib.spgan_gemm_nt_col_blocks(r), lib.spgan_gemm_nt_owns_columns(r), lib.spgan_gemm_nt_y16_ok(r), lib.spgan_gemm_nt_uses_w_image(r),
            lib.spgan_edge_attend_bwd_dt_selected(fields["A"], fields["lda"], fields["W"], fields["ldw"], fields["M"], 10, fields["K"], fields["tile_hint"]))


def plan(lib, fields, binding=None):
    """spgan_gemm_nt_kernel and the whole plan (spgan_gemm_nt_plan: a tuple in the order of spgan._lib.NT_PLAN_FIELDS) of one case."""
    a = to_args(fields, binding)
    out = (C.c_int32 * 10)()
    assert lib.spgan_gemm_nt_plan(C.byref(a), out) == 0
    return lib.spgan_gemm_nt_kernel(C.byref(a)), tuple(out)
