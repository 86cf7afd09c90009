"""CPU: which kernel spgan_gemm_tn runs, on which split, is decided in one host-side plan (csrc/gemm_tn_plan.hpp) that the launch executes and
every query reads; gemm_dual's run plan is one function too.  The queries never read through a pointer, so the library answers them without a
GPU, on the shapes and argument blocks of tn_plan_cases.py:

  (a) the seven shape-only queries that existed before the plan answer what the parent commit's library answered on every shape
      (tests/golden/tn_plan_parent.npz, recorded by tests/golden/make_golden_tn_plan.py);
  (b) the plan's splits are those of spgan_gemm_tn_splits_lp, its workspace that of spgan_gemm_tn_ws_bytes_lp, for every block;
  (c) the plan tells one story, and the blocks reach every branch of it;
  (d) a table of written-out expectations for the kernel, derived by hand from the parent's launch_tn;
  (e) spgan_gemm_tn_skinny_multi's acceptance: the plan's condition equals the parent's list of argument checks.
"""
import os

import numpy as np
import pytest

import tn_plan_cases as tpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKINNY, TILE, LP, WIDE3 = 1, 2, 3, 4
F = {n: i for i, n in enumerate(("kernel", "invalid", "splits", "rows", "tile_b", "fast", "narrow_b", "wide3_cfg", "sparse_rows"))}


@pytest.fixture(scope="module")
def lib():
    from spgan import _lib
    assert tuple(F) == _lib.TN_PLAN_FIELDS
    assert (SKINNY, TILE, LP, WIDE3) == (_lib.TN_KERNEL_SKINNY, _lib.TN_KERNEL_TILE, _lib.TN_KERNEL_LP, _lib.TN_KERNEL_WIDE3)
    return _lib.load()


@pytest.fixture(scope="module")
def world(lib):
    """Every block once: its fields, the kernel and the plan."""
    cs = tpc.blocks()
    kp = [tpc.plan(lib, c["fields"]) for c in cs]
    kern = np.array([k for k, _ in kp])
    plan = np.array([p for _, p in kp], dtype=np.int64)
    assert np.array_equal(kern, plan[:, F["kernel"]])
    get = lambda k: np.array([c["fields"].get(k, 0) for c in cs])       # noqa: E731
    return dict(cases=cs, index={c["name"]: i for i, c in enumerate(cs)}, kern=kern, plan=plan, get=get)


def test_shape_queries_equal_parent(lib):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "tn_plan_parent.npz"))
    sh = tpc.shapes()
    assert np.array_equal(gold["shapes"], np.array(sh)) and tuple(gold["queries"]) == tpc.SHAPE_QUERIES, "the shapes are not those of the recording"
    assert len(sh) == 15 * 17 * 17
    now = np.array([tpc.ask_shape(lib, *s) for s in sh], dtype=np.int64)
    for j, q in enumerate(tpc.SHAPE_QUERIES):
        bad = np.flatnonzero(now[:, j] != gold["answers"][:, j])
        assert bad.size == 0, (q, [(sh[i], int(now[i, j]), int(gold["answers"][i, j])) for i in bad[:8]])
    # the recording is not trivial: both answers of every query family occur
    col = {q: gold["answers"][:, j] for j, q in enumerate(tpc.SHAPE_QUERIES)}
    assert (col["splits_lp2"] != col["splits"]).any() and np.array_equal(col["splits_lp0"], col["splits"]) and np.array_equal(col["splits_lp1"], col["splits"])
    assert (col["dual_wgs_ek0"] > 0).any() and (col["dual_wgs_ek10"] > 0).any() and not (col["dual_wgs_ek5"] > 0).any()
    # spgan_gemm_dual_rows_per_wg answers on a wider set of shapes than spgan_gemm_dual_wgs accepts (M = 4096; Na = 256 with Nb = 64)
    assert ((col["dual_rows_per_wg"] > 0) & (col["dual_wgs_ek0"] == 0)).any()
    assert not ((col["dual_rows_per_wg"] == 0) & (col["dual_wgs_ek0"] > 0)).any()


def test_non_positive_sizes_answer_zero(lib):
    for M, Na, Nb in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 64, 64)):
        assert lib.spgan_gemm_tn_splits(M, Na, Nb) == 0 and lib.spgan_gemm_tn_ws_bytes(M, Na, Nb) == 0
        assert lib.spgan_gemm_tn_splits_lp(M, Na, Nb, 2) == 0 and lib.spgan_gemm_tn_ws_bytes_lp(M, Na, Nb, 2) == 0
    assert lib.spgan_gemm_tn_kernel(None) == 0


def test_plan_split_is_the_shape_query(lib, world):
    w = world
    M, Na, Nb, lp = (w["get"](k) for k in ("M", "Na", "Nb", "mfma_lp"))
    seen = {}
    for i in range(len(w["cases"])):
        key = (M[i], Na[i], Nb[i], lp[i])
        if key not in seen:
            seen[key] = (lib.spgan_gemm_tn_splits_lp(*map(int, key)), lib.spgan_gemm_tn_ws_bytes_lp(*map(int, key)))
        s, b = seen[key]
        assert w["plan"][i, F["splits"]] == s and w["plan"][i, F["splits"]] * Na[i] * Nb[i] * 4 == b, w["cases"][i]["name"]
    assert (w["plan"][:, F["rows"]] % 32 == 0).all() and (w["plan"][:, F["rows"]] > 0).all()
    assert (w["plan"][:, F["splits"]] == -(-M // w["plan"][:, F["rows"]])).all()


def _skinny_shape(Na, Nb):
    return ((Na <= 4) | (Nb <= 4)) & (Na <= 2048) & (Nb <= 2048)


def test_plan_tells_one_story(world):
    w = world
    plan, kern, get = w["plan"], w["kern"], w["get"]
    M, Na, Nb, lp = get("M"), get("Na"), get("Nb"), get("mfma_lp")
    sk = kern == SKINNY
    assert (_skinny_shape(Na, Nb)[sk]).all() and (get("b_mode")[sk] == tpc.A_PLAIN).all()
    assert not get("a_colsum_ws")[sk].any() and not get("b_half")[sk].any() and not get("a_half")[sk].any()
    assert np.array_equal(plan[sk, F["narrow_b"]], (Nb[sk] <= 4).astype(int)) and not plan[~sk, F["narrow_b"]].any()
    w3 = kern == WIDE3
    assert np.array_equal(w3, plan[:, F["wide3_cfg"]] != 0)
    assert (lp[w3] == 2).all() and (M[w3] % 32 == 0).all() and (Na[w3] % 128 == 0).all() and (Nb[w3] % 128 == 0).all()
    assert np.array_equal(plan[w3, F["wide3_cfg"]], np.where(Na[w3] % 256 == 0, 20, 10) + np.where(Nb[w3] % 256 == 0, 4, 2))
    assert ((lp[kern == LP] == 1) & (plan[kern == LP, F["fast"]] == 1)).all()
    tiled = (kern == TILE) | (kern == LP)
    assert np.array_equal(plan[tiled & (plan[:, F["invalid"]] == 0), F["tile_b"]],
                          np.where(Nb > 64, 128, np.where(Nb > 32, 64, 32))[tiled & (plan[:, F["invalid"]] == 0)])
    assert not plan[~tiled, F["tile_b"]].any()
    # the sparse-addend launch follows every kernel but the streaming one (which no block with a prologue on a dense A runs)
    assert np.array_equal(plan[~sk, F["sparse_rows"]] != 0, (get("a_sp_val") != 0)[~sk]) and not plan[sk, F["sparse_rows"]].any()
    # an invalid block names no kernel of its own; 16-bit storage only
    inv = plan[:, F["invalid"]] == 1
    assert ((get("b_half")[inv] == 1) | (get("a_half")[inv] == 1)).all()
    # every branch is reached
    ok = ~inv
    assert set(kern[ok]) == {SKINNY, TILE, LP, WIDE3}
    for k in (TILE, LP):
        assert set(plan[ok & (kern == k), F["tile_b"]]) == {32, 64, 128}, k
    assert set(plan[ok & (kern == TILE), F["fast"]]) == {0, 1} and set(plan[sk, F["narrow_b"]]) == {0, 1}
    assert set(plan[w3, F["wide3_cfg"]]) == {24, 22, 14} and set(plan[w3, F["fast"]]) == {0, 1}
    assert inv.any() and set(plan[:, F["sparse_rows"]]) == {0, 1}


# (d) Written-out expectations, derived by hand from the parent's launch_tn (csrc/gemm.hip of the parent commit, line numbers below).
#   :2012       not skinny and spgan_tn_wide3_eligible (gemm_tn_wide3.hip:323-335: lp == 2, a configuration, no EDGE / 16-bit / A2, 4-byte aligned
#               A and B, slopes in [0, 1]) -> the split-bf16 kernel
#   :2021-2022  PLAIN, skinny shape, no a_colsum_ws, no b_half, and (no a_scale, or A2 on a narrow B without a_lrelu / a_sp_val) -> streaming
#   :2030       b_half off the bf16 kernel (b_mode, lp != 1, a_sp_val) -> SPGAN_EINVAL
#   :2031       a_half with lp != 1, a_sp_val or a skinny shape -> SPGAN_EINVAL
#   :2034-2036  fast = sizes and leading dimensions multiples of 4, A, B (A2) 16-byte aligned; 16-bit storage and not fast -> SPGAN_EINVAL
#   :2037-2048  fast and lp == 1 -> bf16 kernel; else the fp32 kernel, with or without vector loads; width by Nb (:1897)
#   :2002-2004  the split: lp == 2, not skinny, a wide configuration (from the shape alone) -> the wide split, whichever kernel runs
# name -> (kernel, invalid, tile_b, fast, narrow_b, wide3_cfg); None: any
TABLE = {
    "plain.8192x256x256.lp2": (WIDE3, 0, 0, 1, 0, 24),                # :2012
    "plain.8192x256x128.lp2": (WIDE3, 0, 0, 1, 0, 22),
    "plain.8192x128x256.lp2": (WIDE3, 0, 0, 1, 0, 14),
    "plain.8192x384x256.lp2": (WIDE3, 0, 0, 1, 0, 14),
    "affine.8192x256x256.lp2": (WIDE3, 0, 0, 1, 0, 24),
    "a_lrelu.8192x256x256.lp2": (WIDE3, 0, 0, 1, 0, 24),
    "a_sp.8192x256x256.lp2": (WIDE3, 0, 0, 1, 0, 24),
    "colsum.8192x256x256.lp2": (WIDE3, 0, 0, 1, 0, 24),
    "off_A.8192x256x256.lp2": (WIDE3, 0, 0, 0, 0, 24),                # 4-byte alignment is all that kernel asks
    "plain.8192x128x128.lp2": (TILE, 0, 128, 1, 0, 0),                # configuration 12: not the wide kernel's (gemm_tn_wide3.hip:306)
    "plain.8192x384x384.lp2": (TILE, 0, 128, 1, 0, 0),
    "plain.100x256x256.lp2": (TILE, 0, 128, 1, 0, 0),                 # M % 32
    "A2.8192x256x256.lp2": (TILE, 0, 128, 1, 0, 0),                   # a wide shape the kernel refuses: the fp32 kernel ON THE WIDE SPLIT (below)
    "edge.8192x256x256.lp2": (TILE, 0, 128, 1, 0, 0),
    "affine_slope_out.8192x256x256.lp2": (TILE, 0, 128, 1, 0, 0),
    "a_lrelu_slope_out.8192x256x256.lp2": (TILE, 0, 128, 1, 0, 0),
    "plain.8192x256x256.lp0": (TILE, 0, 128, 1, 0, 0),
    "plain.8192x256x256.lp1": (LP, 0, 128, 1, 0, 0),                  # :2037
    "plain.8192x128x64.lp1": (LP, 0, 64, 1, 0, 0),
    "edge.8192x128x32.lp1": (LP, 0, 32, 1, 0, 0),
    "off_B.8192x256x256.lp1": (TILE, 0, 128, 0, 0, 0),                # unaligned: the fp32 kernel without vector loads, whatever lp is
    "odd_lda.8192x256x64.lp1": (TILE, 0, 64, 0, 0, 0),
    "off_A2.8192x256x32.lp0": (TILE, 0, 32, 0, 0, 0),
    "plain.8192x65x65.lp1": (TILE, 0, 128, 0, 0, 0),                  # Na % 4
    "plain.8192x64x3.lp0": (SKINNY, 0, 0, None, 1, 0),                # :2021
    "plain.8192x3x64.lp2": (SKINNY, 0, 0, None, 0, 0),
    "plain.8192x4x4.lp1": (SKINNY, 0, 0, None, 1, 0),
    "A2.8192x64x3.lp0": (SKINNY, 0, 0, None, 1, 0),                   # the two-tensor operand on the wide side
    "A2.8192x3x64.lp0": (TILE, 0, 64, 0, 0, 0),                       # ... but not on the narrow side
    "a_scale.8192x64x3.lp0": (TILE, 0, 32, 0, 0, 0),                  # any other prologue: the MFMA kernel
    "affine.8192x64x3.lp0": (TILE, 0, 32, 0, 0, 0),
    "colsum.8192x64x3.lp0": (TILE, 0, 32, 0, 0, 0),                   # a skinny shape with the by-product: the MFMA kernel
    "colsum.8192x64x4.lp1": (LP, 0, 32, 1, 0, 0),
    "plain.8192x2049x3.lp0": (TILE, 0, 32, 0, 0, 0),                  # more than 2048 columns on the wide side
    "plain.8192x64x5.lp0": (TILE, 0, 32, 0, 0, 0),
    "b_half.8192x256x256.lp1": (LP, 0, 128, 1, 0, 0),                 # 16-bit storage on the bf16 kernel
    "a_half.A2.8192x256x64.lp1": (LP, 0, 64, 1, 0, 0),
    "b_half.colsum.8192x128x128.lp1": (LP, 0, 128, 1, 0, 0),
    "b_half.8192x256x256.lp0": (None, 1, None, None, None, 0),        # :2030
    "b_half.8192x256x256.lp2": (None, 1, None, None, None, 0),
    "b_half.affine.8192x256x256.lp1": (None, 1, None, None, None, 0),
    "b_half.a_sp.8192x256x256.lp1": (None, 1, None, None, None, 0),
    "a_half.8192x256x256.lp0": (None, 1, None, None, None, 0),        # :2031
    "a_half.a_sp.8192x256x256.lp1": (None, 1, None, None, None, 0),
    "b_half.off_B.8192x256x256.lp1": (None, 1, None, None, None, 0),  # :2036
    "a_half.odd_lda.8192x256x256.lp1": (None, 1, None, None, None, 0),
    "b_half.8192x65x64.lp1": (None, 1, None, None, None, 0),
    # 16-bit storage on a skinny shape: the query follows the launch, where ops.gemm_tn's copy of the rule said "streaming".
    "b_half.8192x64x4.lp1": (LP, 0, 32, 1, 0, 0),                     # :2021 `!a.b_half` -> :2037, the bf16 kernel
    "b_half.8192x4x64.lp1": (LP, 0, 64, 1, 0, 0),
    "b_half.8192x64x3.lp1": (None, 1, None, None, None, 0),           # ... Nb % 4: :2036
    # a_half: the parent's :2021 did not ask, so a plain or A2 / narrow-B block ran the streaming kernel on 16-bit memory as if it were
    # fp32 (it read past the operand); :2031 rejected the rest.  The plan rejects every 16-bit A on a skinny shape.
    "a_half.8192x64x4.lp1": (None, 1, None, None, None, 0),
    "a_half.A2.8192x64x4.lp1": (None, 1, None, None, None, 0),
    "a_half.A2.8192x4x64.lp1": (None, 1, None, None, None, 0),
    "a_half.8192x3x64.lp0": (None, 1, None, None, None, 0),
}


def test_written_out_kernels(lib, world):
    w = world
    cols = [F[n] for n in ("kernel", "invalid", "tile_b", "fast", "narrow_b", "wide3_cfg")]
    for name, want in TABLE.items():
        got = w["plan"][w["index"][name]][cols]
        assert all(x is None or int(g) == x for g, x in zip(got, want)), (name, list(map(int, got)), want)
    # the wide split on the fp32 kernel: a wide-shaped lp == 2 problem with a two-tensor A runs the split of its plain sibling, which is not
    # the fp32 kernel's own (at M = 65536, where the two rules differ: 256 partials of 256 rows against 128 of 512)
    a2, plain, own = (np.array(tpc.plan(lib, dict(w["cases"][w["index"][n]]["fields"], M=65536))[1])
                      for n in ("A2.8192x256x256.lp2", "plain.8192x256x256.lp2", "A2.8192x256x256.lp0"))
    assert a2[F["kernel"]] == TILE and plain[F["kernel"]] == WIDE3 and own[F["kernel"]] == TILE
    assert tuple(a2[[F["splits"], F["rows"]]]) == tuple(plain[[F["splits"], F["rows"]]]) == (256, 256)
    assert tuple(own[[F["splits"], F["rows"]]]) == (128, 512)
    assert lib.spgan_gemm_tn_splits_lp(65536, 256, 256, 2) == 256 and lib.spgan_gemm_tn_splits(65536, 256, 256) == 128


def _parent_skinny_multi_accepts(f):
    """The parent's spgan_gemm_tn_skinny_multi argument checks on one block (csrc/gemm.hip:2229-2234 of the parent), geometry equalities apart."""
    g = lambda k: f.get(k, 0)                                           # noqa: E731
    ok = g("A") and g("B") and g("ws") and 0 < g("M") < (1 << 24) and g("Na") > 0 and 0 < g("Nb") <= 4 and g("Na") <= 2048
    ok = ok and g("lda") >= g("Na") and g("ldb") >= g("Nb")
    ok = ok and g("b_mode") == tpc.A_PLAIN and g("defer_reduce") and not g("a_colsum_ws") and not g("b_half") and not g("a_half")
    ok = ok and not g("a_lrelu") and not g("a_sp_val")
    if g("A2"):
        ok = ok and g("a_scale") and g("a_scale2") and g("a_shift") and g("lda2") >= g("Na")
    else:
        ok = ok and not g("a_scale")
    return bool(ok)


def test_skinny_multi_acceptance_is_the_plan(world):
    w = world
    n = {True: 0, False: 0}
    for i, c in enumerate(w["cases"]):
        f = c["fields"]
        if f["Nb"] > 4:
            continue
        p = w["plan"][i]
        says = bool(p[F["kernel"]] == SKINNY and p[F["narrow_b"]] and not p[F["invalid"]] and f["defer_reduce"])
        assert says == _parent_skinny_multi_accepts(f), c["name"]
        n[says] += 1
    assert n[True] > 100 and n[False] > 1000
