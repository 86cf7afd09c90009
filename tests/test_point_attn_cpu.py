"""CPU: the float64 model of dot-product point attention and of the two modules on it (tests/point_attn_model.py) against the vectors
captured from the reference (golden point_attn.npz); spgan.Self_Attn's state_dict and initialisation against nn.Conv1d's in the reference's
order; Attention's materialize option; the domain; and the argument checks of the point-attention entry points (no GPU needed).

query.bias of Self_Attn adds the same number to every score of one softmax column and cancels: its gradient is rounding noise around zero in
the reference (below 1e-12 in float64, stored for float32 as `tag|qbias_f32`), so it is compared as an absolute number."""
import numpy as np
import pytest
import torch
from torch import nn

import point_attn_model as pm
from helpers import golden

TAGS = list(pm.CASES)


@pytest.fixture(scope="module")
def d():
    return golden("point_attn.npz")


@pytest.mark.parametrize("tag", TAGS)
def test_float64_model_matches_reference(d, tag):
    """Every quantity of every case at 1e-10 rel-L2; exact zeros where the case table says so."""
    kind = pm.CASES[tag]["module"]
    x, cot, sd = pm.golden_inputs(d, tag)
    res = pm.module_run(kind, sd, x, cot, torch.float64)
    assert tuple(res) == pm.quantities(tag)
    for q in pm.quantities(tag):
        if q == "grad|query.bias":
            assert float(res[q].abs().max()) < 1e-12 and float(np.abs(pm.stored(d, tag, q)).max()) < 1e-12 and float(d[tag + "|qbias_f32"]) < 1e-5
        elif q in pm.EXACT_ZERO.get(tag, ()):
            assert not np.any(pm.stored(d, tag, q)) and float(res[q].abs().max()) == 0.0, (tag, q)
        else:
            assert np.any(pm.stored(d, tag, q)), (tag, q)
            assert pm.golden_rel(d, tag, q, res[q]) <= 1e-10, (tag, q, pm.golden_rel(d, tag, q, res[q]))
        if "%s|%s|l2" % (tag, q) in d:
            assert abs(float(res[q].norm()) - float(d["%s|%s|l2" % (tag, q)])) <= 1e-10 * float(d["%s|%s|l2" % (tag, q)])


@pytest.mark.parametrize("tag", ["a", "d", "f"])
def test_written_out_core_backward_matches_autograd(d, tag):
    """dQ, dK, dV of the launcher contract (dS = P (dP - D), D = dO . O) against autograd through the core's forward, float64."""
    c = pm.CASES[tag]
    g = torch.Generator().manual_seed(11)
    q, k = (torch.randn(c["B"], c["N"], 8, generator=g, dtype=torch.float64) for _ in range(2))
    v, dO = (torch.randn(c["B"], c["N"], 12, generator=g, dtype=torch.float64) for _ in range(2))
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    O, lse, P = pm.core_forward(*leaves)
    (O * dO).sum().backward()
    assert pm.rel(P.detach().sum(-1), torch.ones_like(lse.detach())) <= 1e-12
    for got, leaf, nm in zip(pm.core_backward(q, k, v, dO), leaves, ("dQ", "dK", "dV")):
        assert pm.rel(got, leaf.grad) <= 1e-12, (tag, nm)


def test_case_conditions(d):
    """gamma non-zero everywhere; b: one point; d: every row spans +-30, its maximum at j = N - 1, the prefix maximum rises across every
    32-key boundary; g: uniform attention."""
    for tag in TAGS:
        x, cot, sd = pm.golden_inputs(d, tag)
        assert float(sd["gamma"].abs().min()) > 0 and tuple(x.shape) == (pm.CASES[tag]["B"], pm.CASES[tag]["ch"], pm.CASES[tag]["N"])
    x, cot, sd = pm.golden_inputs(d, "d")
    S = pm.scores("d", sd, x.double())
    N = S.shape[2]
    assert bool((S.max(-1).values >= 30).all()) and bool((S.min(-1).values <= -30).all()) and bool((S.argmax(-1) == N - 1).all())
    for m in range(32, N, 32):
        assert bool((S[:, :, m:m + 32].max(-1).values > S[:, :, :m].max(-1).values).all()), m
    x, cot, sd = pm.golden_inputs(d, "g")
    assert float(pm.scores("g", sd, x.double()).abs().max()) == 0.0


def _twin(in_dim):
    """the reference's Self_Attn as a parameter container: nn.Conv1d in its order, gamma first in the state_dict"""
    m = nn.Module()
    m.query = nn.Conv1d(in_dim, in_dim // 8, 1)
    m.key = nn.Conv1d(in_dim, in_dim // 8, 1)
    m.value = nn.Conv1d(in_dim, in_dim, 1)
    m.gamma = nn.Parameter(torch.zeros(1))
    return m


@pytest.mark.parametrize("tag", ["e", "f"])
def test_self_attn_state_dict_matches_reference(d, tag):
    import spgan
    c = pm.CASES[tag]
    m = spgan.Self_Attn(c["ch"])
    assert list(m.state_dict().keys()) == list(d["state_keys|Self_Attn"]) == list(pm.STATE_KEYS["Self_Attn"])
    sd = pm.golden_state_dict(d, tag)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()} == pm.state_shapes(c)
    m.load_state_dict(sd, strict=True)                                     # the reference's state_dict into the module ...
    twin = _twin(c["ch"])
    twin.load_state_dict(m.state_dict(), strict=True)                      # ... and the module's into the reference's layout
    for k, v in twin.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_self_attn_default_initialisation():
    import spgan
    torch.manual_seed(4321)
    m = spgan.Self_Attn(48)
    torch.manual_seed(4321)
    twin = _twin(48)
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in twin.named_parameters()]
    for a, b in zip(m.parameters(), twin.parameters()):
        assert torch.equal(a, b)
    after = torch.rand(3)                                                  # the generator has advanced exactly as far
    torch.manual_seed(4321)
    spgan.Self_Attn(48)
    assert torch.equal(after, torch.rand(3))
    assert spgan.Self_Attn().chanel_in == 128 and float(m.gamma.detach()) == 0.0


def test_attention_materialize_option(d):
    import spgan
    torch.manual_seed(7)
    a = spgan.Attention(64)
    torch.manual_seed(7)
    b = spgan.Attention(64, materialize=False)
    assert a.materialize is True and b.materialize is False
    assert list(a.state_dict().keys()) == list(b.state_dict().keys()) == list(d["state_keys|Attention"]) == list(pm.STATE_KEYS["Attention"])
    for (k, v), w in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(v, w), k
    b.load_state_dict(pm.golden_state_dict(d, "a"), strict=True)
    big = spgan.Attention(1032)                                            # the default route has no such limit ...
    big.materialize = False                                                # ... and the attribute is checked at the call (GPU test)


def test_domain_and_cpu_tensors():
    import spgan
    from spgan import point_attn
    with pytest.raises(ValueError, match="ch=1032"):
        spgan.Attention(1032, materialize=False)
    with pytest.raises(ValueError, match="in_dim=520"):
        spgan.Self_Attn(520)
    with pytest.raises(ValueError, match="in_dim=0"):
        spgan.Self_Attn(0)
    spgan.Attention(1024, materialize=False), spgan.Self_Attn(512)         # the largest widths of the domain
    with pytest.raises(RuntimeError, match="GPU"):
        spgan.Self_Attn(16)(torch.zeros(1, 16, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        spgan.Attention(16, materialize=False)(torch.zeros(1, 16, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        point_attn.point_attention(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4, 8))
    with pytest.raises(ValueError):
        point_attn.padded_dk(129)
    assert [point_attn.padded_dk(k) for k in (1, 3, 4, 80, 128)] == [4, 4, 4, 80, 128]


def test_entry_points_reject_bad_arguments():
    """Bad sizes and null pointers give SPGAN_EINVAL (-22) before any launch."""
    from spgan import _lib
    lib = _lib.load()
    assert [lib.spgan_point_attn_padded_dk(k) for k in (0, 1, 3, 4, 80, 128, 129)] == [0, 4, 4, 4, 80, 128, 0]
    assert lib.spgan_point_attn_max_dv() == 512
    p = 256                                                                # a non-null, 16-byte aligned pointer value: never dereferenced here
    base = dict(q=p, ldq=8, k=p, ldk=8, v=p, ldv=16, b=1, n=4, dk=8, dv=16, o=p, ldo=16, lse=p, s=None)
    fwd = lambda **kw: lib.spgan_point_attn_fwd(*[{**base, **kw}[a] for a in ("q", "ldq", "k", "ldk", "v", "ldv", "b", "n", "dk", "dv", "o", "ldo", "lse", "s")])
    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(lse=None), dict(n=0), dict(b=0), dict(dk=6), dict(dk=3), dict(dk=0),
                dict(dk=132, ldq=132, ldk=132), dict(dv=513, ldv=516, ldo=516), dict(dv=516, ldv=516, ldo=516), dict(dv=0), dict(ldq=4),
                dict(ldv=8), dict(ldo=18), dict(q=264)):
        assert fwd(**bad) == -22, bad
    bbase = dict(role=0, q=p, ldq=8, k=p, ldk=8, v=p, ldv=16, dO=p, lddo=16, lse=p, D=p, b=1, n=4, dk=8, dv=16, dq=p, lddq=8, dkey=p, lddk=8,
                 dval=p, lddv=16, s=None)
    order = ("role", "q", "ldq", "k", "ldk", "v", "ldv", "dO", "lddo", "lse", "D", "b", "n", "dk", "dv", "dq", "lddq", "dkey", "lddk", "dval", "lddv", "s")
    bwd = lambda **kw: lib.spgan_point_attn_bwd(*[{**bbase, **kw}[a] for a in order])
    for bad in (dict(role=2), dict(q=None), dict(dO=None), dict(lse=None), dict(D=None), dict(n=0), dict(dk=6), dict(dv=513, ldv=516, lddo=516, lddv=516),
                dict(dq=None), dict(lddq=4), dict(role=1, dkey=None), dict(role=1, dval=None), dict(role=1, lddv=8), dict(role=1, n=0),
                dict(role=1, dk=5), dict(role=1, q=None)):
        assert bwd(**bad) == -22, bad
