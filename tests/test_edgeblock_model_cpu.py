"""CPU: tests/edgeblock_model.py (the float64-autograd reference of the EdgeBlock gather kernels) against the oracle and against the older
hand-derived float32 model, its constructed graphs, and the seed search of tests/test_edgeblock_gpu.py on the reference alone."""
import pytest
import torch

import edgeblock_model as em
import kernel_model as km
from oracle import spgan_oracle as orc


@pytest.mark.parametrize("Fin,Fout,k,B,N,hand", [(3, 8, 4, 2, 20, True), (6, 10, 3, 1, 17, False)])
def test_block_equals_oracle_float64(Fin, Fout, k, B, N, hand):
    """Output, input gradient, every parameter gradient and the running buffers, train mode, same injected graph: 1e-12 rel-L2."""
    c = em.module_case(Fin, Fout, k, B, N, seed=7)
    if not hand:
        c["idx"] = em.random_graph(B, N, k, torch.Generator().manual_seed(3))[0]
    mine = em.run_block(c, torch.float64)
    p = {"e." + n: v.double().requires_grad_(True) for n, v in c["params"].items()}
    bufs = {"e." + n: v for n, v in em.fresh_buffers(Fout, torch.float64).items()}
    x = c["x"].double().requires_grad_(True)
    loc = c["idx"].view(B, N * k) - (torch.arange(B) * N).view(B, 1)
    out = orc.edge_block(p, "e", x, k, idx=loc, training=True, buffers=bufs)
    grads = torch.autograd.grad((out * c["dy"].double()).sum(), [x] + list(p.values()))
    assert em.rel(mine["out"], out) <= 1e-12 and em.rel(mine["dx"], grads[0]) <= 1e-12
    for n, g in zip(p, grads[1:]):
        if n.endswith(("conv_w.0.bias", "conv_w.3.bias", "conv_x.0.bias")):      # in front of a train-mode BatchNorm: zero up to rounding
            assert float((mine["grad|" + n[2:]] - g).abs().max()) <= 1e-12, n
        else:
            assert em.rel(mine["grad|" + n[2:]], g) <= 1e-12, n
    for n, b in bufs.items():
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(mine["buf|" + n[2:]]) == 1
        else:
            assert em.rel(mine["buf|" + n[2:]], b) <= 1e-12, n


@pytest.mark.parametrize("B,N,k,H,F_,hand", [(2, 50, 10, 12, 24, True), (1, 77, 3, 16, 36, False), (2, 33, 1, 8, 16, True)])
def test_autograd_model_agrees_with_hand_derived_model(B, N, k, H, F_, hand):
    """kernel_model.edge_attend_bwd / edge_scatter (the kernels' formulas, float32) against the float64 autograd of this model, held to the
    bound of a float32 launcher: max(1e-5, 5 x the float32-vs-float64 distance of this model); forward quantities to max(2e-6, 5 x ...)."""
    c = em.find_launcher_case(B, N, k, H, F_, hand)
    idx, slope = c["idx"], c["slope"]

    def run(dt, mod):
        t = lambda n: c[n].to(dt)
        a = (t("h2pre"), t("sc2"), t("sh2"), t("PQR"), idx, t("bx"), t("scx"), t("shx"), slope)
        ab = (t("dT"), t("h2pre"), t("sc2"), t("sh2"), t("mean2"), t("inv2"), t("PQR"), idx, t("bx"), t("scx"), t("shx"), t("meanx"), t("invx"), slope)
        r = {}
        if mod is em:
            r["T"] = em.attend(*a)[0]
            r["mean"], r["var"] = em.stats(t("PQR"), idx, t("b1"), t("bx"))
            r["g2"], r["gy"], r["sums2"], r["sumsy"] = em.attend_bwd(*ab)
        else:
            r["T"] = km.edge_attend_fwd(*a)
            r["mean"], r["var"] = km.edge_stats(t("PQR"), idx, t("b1"), t("bx"))
            r["g2"], r["gy"], r["sums2"], r["sumsy"] = km.edge_attend_bwd(*ab)
        g1, gy = t("g1"), r["gy"]
        s1 = torch.cat([g1.sum(0), (g1 * ((em.pre(t("PQR"), idx, t("b1"), t("bx"))[0] - t("mean1")) * t("inv1"))).sum(0)])
        sc = (g1, gy, t("PQR"), idx) + ((t("b1"), t("mean1"), t("inv1"), t("gam1"), s1, t("bx"), t("meanx"), t("invx"), t("gamx"), r["sumsy"]))
        r["dPQR"] = em.scatter(*sc) if mod is em else km.edge_scatter(*sc[:4], None, None, *sc[4:])
        return r
    m64, m32, old = run(torch.float64, em), run(torch.float32, em), run(torch.float32, km)
    for q in m64:
        bound = max(2e-6 if q in ("T", "mean", "var") else 1e-5, 5.0 * em.rel(m32[q], m64[q]))
        assert em.rel(old[q], m64[q]) <= bound, (q, em.rel(old[q], m64[q]), bound)


def test_scatter_refuses_foreign_statistics():
    c = em.find_launcher_case(1, 3, 2, 4, 8, True)
    d = lambda n: c[n].double()
    g1, gy = d("g1"), d("dT").view(-1, 8)
    h1, yp = em.pre(d("PQR"), c["idx"], d("b1"), d("bx"))
    s = lambda g, v, m, i: torch.cat([g.sum(0), (g * ((v - m) * i)).sum(0)])
    args = [g1, gy, d("PQR"), c["idx"], d("b1"), d("mean1"), d("inv1"), d("gam1"), s(g1, h1, d("mean1"), d("inv1")),
            d("bx"), d("meanx"), d("invx"), d("gamx"), s(gy, yp, d("meanx"), d("invx"))]
    em.scatter(*args)
    args[8] = args[8] * 1.001
    with pytest.raises(AssertionError, match="sums1"):
        em.scatter(*args)


@pytest.mark.parametrize("B,N,k", sorted({(c[0], c[1], c[2]) for c in em.LAUNCHER_CASES + em.SPECIAL_CASES} | {(c[3], c[4], c[2]) for c in em.MODULE_CASES}))
def test_hand_graph_realises_its_in_degrees(B, N, k):
    idx, indeg = em.hand_graph(B, N, k, torch.Generator().manual_seed(N + k))
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (B * N, k)
    assert torch.equal(indeg, torch.bincount(idx.reshape(-1), minlength=B * N)) and int(indeg.sum()) == B * N * k
    targets = em.hand_targets(N, k)
    if N * k >= 400 and k > 1:
        assert targets == list(em.TARGET_DEGREES)                # every case of this size has room for all six
    for b in range(B):
        rows, deg = idx[b * N:(b + 1) * N], indeg[b * N:(b + 1) * N]
        assert int(rows.min()) >= b * N and int(rows.max()) < (b + 1) * N       # edges stay inside their shape
        assert bool((rows[:, 0] == b * N + em.HUB).all()) and int(deg[em.HUB]) == N + k - 1     # gathered by every point, itself included
        assert int(deg[em.LONELY]) == 0
        assert bool((rows[em.REPEATER] == b * N + em.HUB).all())                # one neighbour k times
        assert [int(deg[3 + t]) for t in range(len(targets))] == targets


def test_random_graph_rows_are_permutation_prefixes():
    idx, indeg = em.random_graph(2, 9, 5, torch.Generator().manual_seed(1))
    for r in range(18):
        assert len(set(idx[r].tolist())) == 5 and r // 9 * 9 <= int(idx[r].min()) and int(idx[r].max()) < (r // 9 + 1) * 9
    assert int(indeg.sum()) == 90


@pytest.mark.parametrize("hand", [False, True])
@pytest.mark.parametrize("B,N,k,H,F_", em.LAUNCHER_CASES)
def test_seed_search_terminates_for_launcher_cases(B, N, k, H, F_, hand):
    c = em.find_launcher_case(B, N, k, H, F_, hand)
    assert em.case_kinks_clear(c)
    for n in ("sc2", "scx", "gam1", "gamx"):                     # every third entry is negative
        assert bool((c[n][::3] < 0).all()) and bool((c[n][1::3] > 0).all()) and bool((c[n][2::3] > 0).all()), n


@pytest.mark.parametrize("B,N,k,H,F_", em.SPECIAL_CASES)
def test_seed_search_terminates_for_special_cases(B, N, k, H, F_):
    c = em.find_launcher_case(B, N, k, H, F_, True, "softmax")
    _, z2, _ = em.attend(*[c[n].double() if n != "idx" else c[n] for n in ("h2pre", "sc2", "sh2", "PQR", "idx", "bx", "scx", "shx")], c["slope"])
    assert 100.0 < float(z2.abs().max()) < 160.0                 # expf overflows near 88.7
    assert em.case_kinks_clear(em.find_launcher_case(B, N, k, H, F_, True, "offset"))


def test_slopes_split_evenly():
    s = [em.case_slope(*c) for c in em.LAUNCHER_CASES]
    assert 4 <= s.count(0.2) <= 5 and s.count(0.2) + s.count(0.01) == len(s)


@pytest.mark.parametrize("Fin,Fout,k,B,N", em.MODULE_CASES)
def test_seed_search_terminates_for_module_cases(Fin, Fout, k, B, N):
    c = em.find_module_case(Fin, Fout, k, B, N)
    assert set(c["m64"]["z"]) == {"z1", "z2", "zy"}
    assert all(em.kinks_clear(z) for z in c["m64"]["z"].values())
