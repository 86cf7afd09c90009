"""CPU: the float64 model of the decomposed PointTransformerLayer (tests/point_transformer_model.py) against the vectors captured from
the reference (golden point_transformer.npz), the written-out backward of the launcher contracts against autograd, the module's
state_dict and initialisation against nn.Linear's, and the argument checks of the pair-attention entry points (no GPU needed)."""
import numpy as np
import pytest
import torch
from torch import nn

import point_transformer_model as pm
from helpers import golden

TAGS = list(pm.CASES)
QUANTITIES = ("out", "dx", "dpos") + tuple("grad|" + k for k in pm.STATE_KEYS)


@pytest.fixture(scope="module")
def d():
    return golden("point_transformer.npz")


def _inputs(d, tag, dtype):
    return (torch.from_numpy(d[tag + "|x"]).to(dtype), torch.from_numpy(d[tag + "|pos"]).to(dtype), torch.from_numpy(d[tag + "|g"]).to(dtype),
            pm.golden_state_dict(d, tag))


def _named(out, g):
    res = {"out": out, "dx": g["dx"], "dpos": g["dpos"]}
    res.update({"grad|" + k: g[k] for k in pm.STATE_KEYS})
    return res


@pytest.mark.parametrize("tag", TAGS)
def test_float64_model_matches_reference(d, tag):
    """The decomposed formulation, written-out backward included, is the reference's function: 1e-9 rel-L2 in float64.  The gradient of
    attn_mlp.2.bias is an exact zero in the model and rounding noise (below 1e-12 in float64) in the reference."""
    x, pos, g, sd = _inputs(d, tag, torch.float64)
    res = _named(*pm.layer_backward(sd, x, pos, g))
    for q in QUANTITIES:
        if q == "grad|attn_mlp.2.bias":
            assert float(res[q].abs().max()) == 0.0 and float(np.abs(d["%s|%s|full" % (tag, q)]).max()) < 1e-12
            continue
        assert pm.golden_rel(d, tag, q, res[q]) <= 1e-9, (tag, q, pm.golden_rel(d, tag, q, res[q]))


@pytest.mark.parametrize("tag", TAGS)
def test_float32_model_within_reference_noise(d, tag):
    """The same model evaluated in float32 stays within 5 x the reference's own float32 error."""
    x, pos, g, sd = _inputs(d, tag, torch.float32)
    res = _named(*pm.layer_backward(sd, x, pos, g))
    for q in QUANTITIES:
        if q == "grad|attn_mlp.2.bias":
            continue
        assert pm.golden_rel(d, tag, q, res[q]) <= 5 * pm.noise(d, tag, q), (tag, q)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "f"])
def test_written_out_backward_matches_autograd(d, tag):
    x, pos, g, sd = _inputs(d, tag, torch.float64)
    out, grads = pm.layer_backward(sd, x, pos, g)
    out_a, auto = pm.autograd_run(sd, x, pos, g)
    assert torch.equal(out, out_a)
    for k in grads:
        assert pm.rel(grads[k], auto[k]) <= 1e-12, (tag, k)
    # the launcher contracts one by one: dS and the four sums of the pair backward from autograd through pair_fwd
    Wq, Wk, Wv, Wp1, bp1, Wp2, bp2, Wa1, wa2, Wc, c = pm.derived(sd, torch.float64)
    _, (q, k, v, QaC, Ka, R, lse) = pm.layer_forward(sd, x, pos, keep=True)
    leaves = [t.clone().requires_grad_(True) for t in (QaC, Ka, Wc, wa2, v, pos)]
    Sv, Rr, _ = pm.pair_fwd(leaves[5], Wp1, bp1, leaves[0], leaves[1], leaves[2], leaves[3], leaves[4])
    dR = g @ Wp2
    ((Sv * g).sum() + (Rr * dR).sum()).backward()
    P = pm.pair_probs(pos, Wp1, bp1, QaC, Ka, Wc, wa2, lse)
    assert pm.rel(P.sum(-1), torch.ones_like(lse)) <= 1e-12
    dS = pm.pair_dsim(P, g, v, dR, pos, Wp1, bp1)
    dQa, dKa, Zq, Zk, dWc, dwa2 = pm.pair_bwd(pos, Wp1, bp1, QaC, Ka, Wc, wa2, P, dS, dR)
    for got, want, nm in ((dQa, leaves[0].grad, "dQa"), (dKa, leaves[1].grad, "dKa"), (dWc, leaves[2].grad, "dWc"), (dwa2, leaves[3].grad, "dwa2"),
                          (P.transpose(1, 2) @ g, leaves[4].grad, "dv"), ((Zq - Zk) @ Wp1, leaves[5].grad, "dpos")):
        assert pm.rel(got, want) <= 1e-12, (tag, nm)


def test_case_conditions(d):
    """b: one point -> out = v + bp2 and exact zeros; d: every row's maximum in the last key tile, sim spanning +-30 or more;
    f: uniform attention -> out_i = mean_j (v_j + e_ij)."""
    x, pos, g, sd = _inputs(d, "b", torch.float64)
    Wq, Wk, Wv, Wp1, bp1, Wp2, bp2, Wa1, wa2, Wc, c = pm.derived(sd, torch.float64)
    assert pm.rel(torch.from_numpy(d["b|out|full"]), x @ Wv.t() + torch.relu(bp1) @ Wp2.t() + bp2) <= 1e-12
    for q in ("dpos",) + tuple("grad|" + n for n in pm.ATTN_PARAMS):
        assert not np.any(d["b|%s|full" % q]), q
    x, pos, g, sd = _inputs(d, "d", torch.float64)
    sim = pm.sim_of(sd, x, pos)
    last0 = (sim.shape[2] - 1) // pm.TILE * pm.TILE
    assert last0 == 3 * pm.TILE and float(sim.max()) > 30 and float(sim.min()) < -30
    assert bool((sim[:, :, last0:].max(-1).values > sim[:, :, :last0].max(-1).values).all())
    x, pos, g, sd = _inputs(d, "f", torch.float64)
    Wq, Wk, Wv, Wp1, bp1, Wp2, bp2, Wa1, wa2, Wc, c = pm.derived(sd, torch.float64)
    e = pm.hidden(pos, Wp1, bp1) @ Wp2.t() + bp2
    assert pm.rel(torch.from_numpy(d["f|out|full"]), ((x @ Wv.t())[:, None] + e).mean(2)) <= 1e-12
    for tag in TAGS:
        x, pos, g, sd = _inputs(d, tag, torch.float64)
        assert pm.relu_margin(sd, x, pos) >= 2e-6, tag


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_matches_reference(d, tag):
    import spgan
    c = pm.CASES[tag]
    m = spgan.PointTransformerLayer(c["dim"], pos_mlp_hidden_dim=c["H"], attn_mlp_hidden_mult=c["mult"])
    assert list(m.state_dict().keys()) == list(d["state_keys"]) == list(pm.STATE_KEYS)
    sd = pm.golden_state_dict(d, tag)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()} == pm.state_shapes(c)
    m.load_state_dict(sd, strict=True)                                     # the reference's state_dict into the module ...
    twin = nn.ModuleDict({"to_qkv": nn.Linear(c["dim"], 3 * c["dim"], bias=False),
                          "pos_mlp": nn.Sequential(nn.Linear(3, c["H"]), nn.ReLU(), nn.Linear(c["H"], c["dim"])),
                          "attn_mlp": nn.Sequential(nn.Linear(c["dim"], c["dim"] * c["mult"]), nn.ReLU(), nn.Linear(c["dim"] * c["mult"], 1))})
    twin.load_state_dict(m.state_dict(), strict=True)                      # ... and the module's into the reference's layout
    for k, v in twin.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_default_initialisation_is_nn_linear():
    import spgan
    torch.manual_seed(1234)
    m = spgan.PointTransformerLayer(16, pos_mlp_hidden_dim=8, attn_mlp_hidden_mult=2)
    torch.manual_seed(1234)
    ref = [nn.Linear(16, 48, bias=False), nn.Linear(3, 8), nn.Linear(8, 16), nn.Linear(16, 32), nn.Linear(32, 1)]
    want = [p for lin in ref for p in lin.parameters()]
    got = list(m.parameters())
    assert len(got) == len(want) == 9
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    after = torch.rand(3)                                                  # the generator has advanced exactly as far
    torch.manual_seed(1234)
    spgan.PointTransformerLayer(16, pos_mlp_hidden_dim=8, attn_mlp_hidden_mult=2)
    assert torch.equal(after, torch.rand(3))


def test_domain_and_cpu_tensors():
    import spgan
    for bad in (dict(dim=513), dict(dim=16, pos_mlp_hidden_dim=65), dict(dim=512, attn_mlp_hidden_mult=9), dict(dim=0)):
        with pytest.raises(ValueError, match="dim"):
            spgan.PointTransformerLayer(**bad)
    m = spgan.PointTransformerLayer(8, 8, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 4, 8), torch.zeros(1, 4, 3))


def test_entry_points_reject_bad_arguments():
    """Bad sizes and null pointers give SPGAN_EINVAL (-22) before any launch."""
    from spgan import _lib
    lib = _lib.load()
    assert [lib.spgan_pair_attn_padded_m(m) for m in (0, 1, 128, 129, 512, 4096, 4097)] == [0, 128, 128, 256, 512, 4096, 0]
    assert [lib.spgan_pair_attn_padded_h(h) for h in (0, 1, 32, 33, 64, 65)] == [0, 32, 32, 64, 64, 0]
    assert lib.spgan_pair_attn_max_dim() == 512
    p = 256                                                                # a non-null pointer value: never dereferenced on these paths
    fwd = lambda **k: lib.spgan_pair_attn_fwd(*[{**dict(pos=p, Wp1p=p, QaC=p, Ka=p, Wc=p, wa2=p, v=p, ldv=8, b=1, n=4, D=8, Mp=128, Hp=32, lse_in=None,
                                                        Sv=p, R=p, lse=p, P=None, s=None), **k}[a] for a in
                                                ("pos", "Wp1p", "QaC", "Ka", "Wc", "wa2", "v", "ldv", "b", "n", "D", "Mp", "Hp", "lse_in", "Sv", "R", "lse", "P", "s")])
    for bad in (dict(pos=None), dict(wa2=None), dict(v=None), dict(Sv=None), dict(n=0), dict(b=0), dict(D=0), dict(D=513), dict(Mp=100), dict(Mp=4224),
                dict(Hp=48), dict(ldv=4), dict(lse_in=p, P=None)):
        assert fwd(**bad) == -22, bad
    assert lib.spgan_pair_attn_dsim(None, p, p, p, 1, 4, 32, p, None) == -22
    assert lib.spgan_pair_attn_dsim(p, p, p, p, 1, 0, 32, p, None) == -22
    assert lib.spgan_pair_attn_dsim(p, p, p, p, 1, 4, 16, p, None) == -22
    assert lib.spgan_pair_attn_dsim(p, p, p, p, 1, 4, 32, None, None) == -22
    assert lib.spgan_pair_attn_bwd_ws_bytes(1, 4, 100, 32) == 0 and lib.spgan_pair_attn_bwd_records(0, 4) == 0
    assert lib.spgan_pair_attn_bwd_ws_bytes(2, 1000, 256, 64) == lib.spgan_pair_attn_bwd_records(2, 1000) * (256 * 64 + 256) * 4
    assert lib.spgan_pair_attn_bwd_records(2, 1000) == 512 and lib.spgan_pair_attn_bwd_records(1, 7) == 7
    bwd = lambda role=0, pos=p, n=4, Mp=128, Hp=32, ws=p, wsb=1 << 30, dA=p: lib.spgan_pair_attn_bwd(role, pos, p, p, p, p, p, p, p, p, p, 1, n, Mp, Hp, dA, p, ws, wsb, None)
    for bad in (dict(role=2), dict(pos=None), dict(n=0), dict(Mp=64), dict(Hp=0), dict(ws=None), dict(wsb=16), dict(dA=None)):
        assert bwd(**bad) == -22, bad
