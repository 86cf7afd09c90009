"""CPU: which kernel spgan_gemm_nt runs is decided in one host-side plan (csrc/gemm_nt_plan.hpp) that the launch executes and every query
reads.  The queries never read through a pointer, so the library answers them without a GPU, on the argument blocks of nt_plan_cases.py:

  (a) on aligned blocks the five queries that existed before the plan answer what the parent commit's library answered
      (tests/golden/nt_plan_parent.npz, recorded by tests/golden/make_golden_nt_plan.py with the SPGAN_NT_* switches unset);
  (b) the new query spgan_gemm_nt_kernel and the old ones tell one story;
  (c) with one address 4 bytes off -- and on the two aligned argument forms of the group `launch_first` -- col_blocks follows the launch
      where the parent's copy of the rule did not; the exceptions are written out, derived by hand from the parent's gemm.hip;
  (d) a grouped block (three passes as one product) gets the kernel and the configuration of its single pass;
  (e) the environment switches, each in a fresh process (they are read once per process).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nt_plan_cases as npc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4, SMALL, TILE, WIDE, WIDE16, WIDE3 = 1, 2, 3, 4, 5, 6
SWITCHES = ("SPGAN_NT_WIDE", "SPGAN_NT_WIDE16", "SPGAN_NT_WIDE3", "SPGAN_NT3_CFG")
F = {n: i for i, n in enumerate(("kernel", "invalid", "tile_n", "owns_columns", "cfg", "db", "fast", "operand", "store16", "wide3_cfg"))}
Q = {n: i for i, n in enumerate(npc.QUERIES)}


@pytest.fixture(scope="module")
def world():
    """Every case once: the five old queries, the kernel and the plan; the parent's answers beside them."""
    if any(os.environ.get(v) for v in SWITCHES):
        pytest.fail("the SPGAN_NT_* switches must be unset: the fixture was recorded without them")
    from spgan import _lib
    assert tuple(F) == _lib.NT_PLAN_FIELDS
    assert (K4, SMALL, TILE, WIDE, WIDE16, WIDE3) == (_lib.NT_KERNEL_K4_STREAM, _lib.NT_KERNEL_SMALL, _lib.NT_KERNEL_TILE, _lib.NT_KERNEL_WIDE,
                                                      _lib.NT_KERNEL_WIDE16, _lib.NT_KERNEL_WIDE3)
    lib = _lib.load()
    cs, single_of = npc.cases()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "nt_plan_parent.npz"))
    assert [c["name"] for c in cs] == list(gold["names"]) and tuple(gold["queries"]) == npc.QUERIES, "the cases are not those of the recording"
    old = np.array([npc.ask(lib, c["fields"]) for c in cs], dtype=np.int64)
    kp = [npc.plan(lib, c["fields"]) for c in cs]
    kern = np.array([k for k, _ in kp])
    plan = np.array([p for _, p in kp], dtype=np.int64)
    assert np.array_equal(kern, plan[:, F["kernel"]])
    group = np.array([c["group"] for c in cs])
    return dict(cases=cs, single_of=single_of, index={c["name"]: i for i, c in enumerate(cs)}, old=old, parent=gold["answers"].astype(np.int64),
                kern=kern, plan=plan, group=group, lib=lib)


def _first_diff(w, rows, got, want):
    bad = np.flatnonzero(rows)[np.flatnonzero(got[rows] != want[rows])]
    return [(w["cases"][i]["name"], int(got[i]), int(want[i])) for i in bad[:8]]


def test_aligned_queries_equal_parent(world):
    w = world
    rows = w["group"] == "aligned"
    assert rows.sum() > 40000
    for q, j in Q.items():
        assert np.array_equal(w["old"][rows, j], w["parent"][rows, j]), (q, _first_diff(w, rows, w["old"][:, j], w["parent"][:, j]))


def test_aligned_group_reaches_every_kernel_and_config(world):
    w = world
    rows = w["group"] == "aligned"
    assert set(w["kern"][rows]) == {K4, SMALL, TILE, WIDE, WIDE16, WIDE3}
    assert set(w["plan"][rows & (w["kern"] == WIDE3), F["wide3_cfg"]]) == {24, 22, 14}
    assert set(w["plan"][w["kern"] != WIDE3, F["wide3_cfg"]]) == {0}
    tiles = w["plan"][rows & (w["kern"] == TILE)]
    forms = {tuple(t[[F["cfg"], F["db"], F["fast"], F["operand"], F["store16"]]]) for t in tiles}
    # the launch_nt_cfg forms of the 128-row family: fp32 in three widths (the two wider ones with and without vector loads), fp16 and
    # split-bf16 operands, 16-bit operand storage
    assert forms == {(0, 1, 1, 0, 0), (0, 1, 0, 0, 0), (1, 0, 1, 0, 0), (1, 0, 0, 0, 0), (2, 0, 0, 0, 0), (1, 0, 1, 2, 0), (0, 1, 1, 1, 0), (1, 0, 1, 1, 0),
                     (0, 1, 1, 1, 1), (1, 0, 1, 1, 1)}
    assert w["plan"][rows, F["invalid"]].any()           # a column tail that no kernel can finish (the launch returns SPGAN_EINVAL)


def test_queries_tell_one_story(world):
    w = world
    old, plan, kern = w["old"], w["plan"], w["kern"]
    N = np.array([c["fields"]["N"] for c in w["cases"]])
    assert np.array_equal(old[:, Q["uses_w_image"]] == 1, kern == WIDE3)
    assert np.array_equal(old[:, Q["owns_columns"]] == 1, plan[:, F["owns_columns"]] == 1)
    assert (kern[old[:, Q["owns_columns"]] == 1] == SMALL).all() and (old[kern == SMALL, Q["owns_columns"]] == 1).all()
    assert np.array_equal(old[:, Q["col_blocks"]], -(-N // plan[:, F["tile_n"]]))
    # the width belongs to the kernel: 256-row tiles are 256 wide (128 in configuration 22), the 128-row family 128 >> CFG
    assert (plan[(kern == WIDE) | (kern == WIDE16), F["tile_n"]] == 256).all()
    w3 = kern == WIDE3
    assert np.array_equal(plan[w3, F["tile_n"]], np.where(plan[w3, F["wide3_cfg"]] == 22, 128, 256))
    assert np.array_equal(plan[~w3 & (kern != WIDE) & (kern != WIDE16), F["tile_n"]], 128 >> plan[~w3 & (kern != WIDE) & (kern != WIDE16), F["cfg"]])
    assert not (plan[:, F["invalid"]] & (kern != TILE)).any()
    # dt_selected <=> the chain's product (its own block) runs the 256 x 256-tile kernel
    seen = set()
    for i, c in enumerate(w["cases"]):
        f = c["fields"]
        if f["K"] != 128:
            assert old[i, Q["dt_selected"]] == 0
            continue
        k, _ = npc.plan(w["lib"], npc.dt_block(f))
        assert (old[i, Q["dt_selected"]] == 1) == (k == WIDE), c["name"]
        seen.add(int(old[i, Q["dt_selected"]]))
    assert seen == {0, 1}


# (c) One address 4 bytes off.  The parent's nt_tile_n (gemm.hip:2093-2103 of the parent) tested `fast` on A and W alone, its launch_nt
# (gemm.hip:1283-1287) also on p_scale / p_shift, e_bias, sp_val / sp_arg and A2 / p_scale2.  With split-bf16 operands (mfma_f16 == 2) and N > 32
# the query therefore answered the split kernel's 64 columns (gemm.hip:2099) where the launch skipped that kernel (gemm.hip:1322) and fell
# through to the fp32 rule (gemm.hip:1332-1343): 128 columns for N > 64 and K >= 512, 64 columns otherwise (no difference).  With fp16 operands
# both agree (128 / 64 by the same N, K rule, gemm.hip:2100 and 1327-1328), and the 256-row-tile kernels refuse such blocks in query and launch
# alike.  So col_blocks moves on exactly these blocks of the group, from N / 64 to N / 128:
MISALIGNED_COL_BLOCKS = {
    "off_%s.%s.%dx%dx512.m2.h%d" % (which, pair, M, N, h): N // 128
    for which, pairs in (("p_scale", ("affine.linear", "edge.linear", "affine.bnbwd")), ("e_bias", ("edge.linear",)),
                         ("A2", ("two.linear", "two.bnbwd", "two.edge_bnbwd")))
    for pair in pairs for M, N in ((8192, 256), (65536, 256)) for h in (0, 2)
}


def test_misaligned_queries_follow_the_launch(world):
    w = world
    rows = w["group"] == "misaligned"
    assert rows.sum() > 500 and set(MISALIGNED_COL_BLOCKS) <= set(w["index"])
    for q, j in Q.items():
        want = w["parent"][:, j].copy()
        if q == "col_blocks":
            for name, v in MISALIGNED_COL_BLOCKS.items():
                assert want[w["index"][name]] == 2 * v, name        # the parent answered N / 64 there
                want[w["index"][name]] = v
        assert np.array_equal(w["old"][rows, j], want[rows]), (q, _first_diff(w, rows, w["old"][:, j], want))
    offsets = {c["name"].split(".")[0] for c in w["cases"] if c["group"] == "misaligned"}
    assert offsets == {"off_" + p for p in npc.OFFSET_POINTERS}


def test_launch_first_forms(world):
    """Two aligned argument forms on which the parent's col_blocks did not follow its own launch; the plan does.
    ADAIN epilogue: spgan_gemm_nt launched the 256 x 256-tile kernel or launch_nt_cfg<PLAIN, ADAIN, 0, 1, 1>, 128 columns wide, whatever K is
    (parent gemm.hip:2200-2201); nt_tile_n answered 64 for K < 512 or N = 64 (gemm.hip:2101-2102).
    fp16-stored A (a_half) of a plain linear product: launch_nt took the 128-row kernels, 128 columns for N > 64 and K >= 512, else 64 (parent
    gemm.hip:1301-1306) BEFORE it asked about the 256-row tiles (gemm.hip:1308-1311); nt_tile_n asked spgan_nt_wide_selected first
    (gemm.hip:2096), which does not look at a_half, and answered 256."""
    w = world
    rows = w["group"] == "launch_first"
    assert rows.sum() > 400
    for q, j in Q.items():
        if q != "col_blocks":
            assert np.array_equal(w["old"][rows, j], w["parent"][rows, j]), q
    moved = 0
    for i in np.flatnonzero(rows):
        f = w["cases"][i]["fields"]
        if f["epi_mode"] == npc.EPI_ADAIN:
            assert w["kern"][i] in (WIDE, TILE)
            width = 256 if w["kern"][i] == WIDE else 128
        else:
            assert f["a_half"] == 1 and w["kern"][i] == TILE and w["plan"][i, F["store16"]] == 1
            width = 128 if (f["N"] > 64 and f["K"] >= 512) else 64
        assert w["old"][i, Q["col_blocks"]] == -(-f["N"] // width), w["cases"][i]["name"]
        moved += int(w["old"][i, Q["col_blocks"]] != w["parent"][i, Q["col_blocks"]])
    assert moved > 0


def test_grouped_block_runs_its_single_pass_kernel(world):
    w = world
    assert len(w["single_of"]) > 5000
    cols = [F[n] for n in ("kernel", "invalid", "tile_n", "cfg", "db", "fast", "operand", "store16", "wide3_cfg")]
    three = np.array([w["index"][a] for a in w["single_of"]])
    one = np.array([w["index"][b] for b in w["single_of"].values()])
    same = (w["plan"][three][:, cols] == w["plan"][one][:, cols]).all(axis=1)
    assert same.all(), [w["cases"][i]["name"] for i in three[~same][:8]]
    assert not w["plan"][three, F["invalid"]].any()
    assert set(w["kern"][three]) == {TILE, WIDE, WIDE16, WIDE3}       # both sides of every pay rule, decided from the rows of ONE group


CHILD = r"""
import importlib.util, json, os, sys, ctypes
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import nt_plan_cases as npc
spec = importlib.util.spec_from_file_location("spgan_lib_binding", os.path.join(sys.argv[1], "sp-gan_amd", "spgan", "_lib.py"))
binding = importlib.util.module_from_spec(spec); spec.loader.exec_module(binding)     # the ctypes table alone: no torch in this process
lib = binding.load()
cs, _ = npc.cases()
names = set(json.loads(sys.argv[2]))
print(json.dumps({c["name"]: list(npc.plan(lib, c["fields"], binding)[1]) for c in cs if c["name"] in names}))
"""

ENV_CASES = ["%s.%dx%dx%d.m%d.h%d" % (kind, M, N, K, m, h) for kind in ("sweep", "affine.bnbwd", "sparse.linear") for M, N, K in
             ((65536, 1024, 128), (65536, 256, 64), (8192, 128, 512), (256, 256, 32)) for m in (0, 1, 2) for h in (0, 1, 2)
             if kind == "sweep" or M in (65536, 256)] + \
            ["w_image.plain.linear.%dx%dx%d.m2.h%d" % (M, N, K, h) for M, N, K in ((65536, 1024, 128), (65536, 1024, 512), (256, 256, 32)) for h in (0, 2)]


def _child(env_extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(ENV_CASES)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def unswitched(world):
    got = _child({})
    assert set(got) == set(ENV_CASES)
    for n, p in got.items():
        assert p == list(world["plan"][world["index"][n]]), n     # a fresh process without switches answers what this one does
    return got


@pytest.mark.parametrize("switch,kernel", [("SPGAN_NT_WIDE", WIDE), ("SPGAN_NT_WIDE16", WIDE16), ("SPGAN_NT_WIDE3", WIDE3)])
def test_switch_removes_exactly_its_kernel(unswitched, switch, kernel):
    got = _child({switch: "0"})
    had = [n for n, p in unswitched.items() if p[F["kernel"]] == kernel]
    assert len(had) >= 4
    for n, p in got.items():
        assert p[F["kernel"]] != kernel, n
        if n not in had:
            assert p == unswitched[n], n
    # what runs instead: the fp16 form of the 256 x 256-tile kernel behind the row-pipelined one, the 128-row family behind the others
    assert {got[n][F["kernel"]] for n in had} == ({WIDE} if kernel == WIDE16 else {TILE})


def test_switch_forces_the_split_bf16_configuration(unswitched):
    got = _child({"SPGAN_NT3_CFG": "22"})
    free = [n for n, p in unswitched.items() if p[F["kernel"]] == WIDE3 and not n.startswith("sparse")]
    assert {unswitched[n][F["wide3_cfg"]] for n in free} == {24, 22, 14}
    for n, p in got.items():
        if n in free:
            assert p[F["wide3_cfg"]] == 22 and p[F["tile_n"]] == 128 and p[F["kernel"]] == WIDE3, n
        else:
            assert p == unswitched[n], n        # the sparse addend keeps configuration 24; other kernels do not read the switch
