"""CPU: the split-bf16 planes of the "bf16x3" operand mode (tests/kernel_model.py::_split_bf16x3, the model of csrc/split_bf16.hpp) over
the whole fp32 range -- every exponent, the whole top binade around the bf16 overflow point, signed zeros, infinities and NaN -- and
the six cross terms the kernels form from them on the non-finite values."""
import numpy as np
import torch

import kernel_model as km

BF16_MAX = km.BF16_MAX
OVERFLOW = 0x7F7F8000           # fp32 bits of the bf16 overflow point: from here on round-to-nearest gives bf16 inf


def _f32(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


def _plain_split(x):
    """The split without the clamp (what the kernels computed before it): the contract's planes wherever hi stays finite."""
    hi = x.bfloat16(); r1 = x - hi.float()
    mid = r1.bfloat16(); r2 = r1 - mid.float()
    return hi, mid, r2.bfloat16()


def _check_finite(x):
    assert torch.isfinite(x).all()
    hi, mid, lo = km._split_bf16x3(x)
    h, m, l_ = hi.double(), mid.double(), lo.double()
    assert torch.isfinite(h).all() and torch.isfinite(m).all() and torch.isfinite(l_).all(), "a plane of a finite value overflowed"
    ax = x.double().abs()
    # exact down to 2^-110, where lo's last bit (2^-23 of x's binade) reaches bf16's subnormal spacing 2^-133; below, lo is rounded to it
    bad = ((h + m + l_) != x.double()) & (ax >= 2.0 ** -110)
    assert not bad.any(), "hi + mid + lo != x at %s" % x[bad][:4].tolist()
    assert ((h + m + l_ - x.double()).abs() <= 2.0 ** -134).all()
    norm = ax >= 2.0 ** -126
    assert (h.abs() <= ax * (1 + 2.0 ** -8))[norm].all(), "hi is not x rounded to 8 bits"   # round to nearest: within half an ulp of 8 bits
    assert (h.abs() <= ax)[ax >= BF16_MAX].all(), "a clamped hi exceeds |x|"
    # bit-identical to the unclamped split wherever that one did not overflow
    keep = torch.isfinite(x.bfloat16().float())
    for p, q in zip((hi, mid, lo), _plain_split(x)):
        assert torch.equal(p[keep].view(torch.int16), q[keep].view(torch.int16)), "the clamp changed an in-range split"
    return hi, mid, lo


def test_split_every_exponent():
    """Every fp32 exponent field (0 = subnormals .. 254), both signs, random 23-bit mantissas and the all-ones mantissa."""
    g = np.random.default_rng(11)
    e = np.repeat(np.arange(255, dtype=np.uint32), 64)
    mant = g.integers(0, 1 << 23, e.size, dtype=np.uint32)
    mant[::64] = (1 << 23) - 1
    mant[1::64] = 0
    bits = (e << 23) | mant
    bits = np.concatenate([bits, bits | 0x80000000])
    _check_finite(_f32(bits))


def test_split_top_binade():
    """Every value of the top binade [2^127, FLT_MAX], both signs: below the overflow point the plain split, from it on hi = +-BF16_MAX."""
    bits = np.arange(0x7F000000, 0x7F800000, dtype=np.uint32)
    x = _f32(np.concatenate([bits, bits | 0x80000000]))
    hi, mid, lo = _check_finite(x)
    ax = x.abs()
    over = ax >= _f32([OVERFLOW])[0]
    assert over.sum().item() == 2 * (0x7F800000 - OVERFLOW)
    assert (hi.float().abs()[over] == BF16_MAX).all() and torch.equal(torch.sign(hi.float()), torch.sign(x))
    assert torch.isinf(x[over].bfloat16().float()).all()                      # ... where plain rounding gives inf (the case the clamp is for)
    # the values on either side of the overflow point, and FLT_MAX
    edge = _f32([0x7F7F0000, 0x7F7F0001, OVERFLOW - 1, OVERFLOW, OVERFLOW + 1, 0x7F7FFFFF])
    eh, em, el = km._split_bf16x3(torch.cat([edge, -edge]))
    assert (eh.float().abs() == BF16_MAX).all()
    assert torch.equal(eh.double() + em.double() + el.double(), torch.cat([edge, -edge]).double())
    fm = km._split_bf16x3(_f32([0x7F7FFFFF]))
    assert [t.item() for t in fm] == [BF16_MAX, float.fromhex("0x1.00p120"), float.fromhex("-0x1.00p104")], [t.item() for t in fm]


def test_split_zero_inf_nan():
    """+-0 keep their sign in hi (the residuals are +0); +-inf -> (+0, +0, +-inf); NaN -> (+0, +0, NaN)."""
    x = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")], dtype=torch.float32)
    hi, mid, lo = km._split_bf16x3(x)
    hb, mb = hi.view(torch.int16).tolist(), mid.view(torch.int16).tolist()
    assert hb == [0, -32768, 0, 0, 0] and mb == [0, 0, 0, 0, 0], (hb, mb)
    assert lo[:2].view(torch.int16).tolist() == [0, 0]
    assert lo[2].item() == float("inf") and lo[3].item() == float("-inf") and torch.isnan(lo[4])


def _six_terms(a, b):
    """a*b as the kernels form it: the six leading cross terms of the planes (float64: every bf16 x bf16 product is exact), smallest first."""
    ah, am, al = (t.double() for t in km._split_bf16x3(a))
    bh, bm, bl = (t.double() for t in km._split_bf16x3(b))
    return al * bh + ah * bl + am * bm + am * bh + ah * bm + ah * bh


def test_cross_terms_of_non_finite_values():
    """inf * b comes out as in fp32 for every finite b -- also b = 1 or 2^k, whose mid and lo planes are zero (inf in hi would meet them:
    inf * 0 = NaN) and b in the clamped top binade; NaN propagates; inf * 0 = NaN.  inf * inf is the one product the six terms cannot form
    (only hi * lo and lo * hi meet the two infinities: inf * 0)."""
    g = torch.Generator().manual_seed(5)
    b = torch.cat([torch.tensor([1.0, -1.0, 2.0 ** -100, 0.75, -3.0, BF16_MAX, -float.fromhex("0x1.fffffep127"), 0.0, -0.0, float("nan")]),
                   torch.randn(256, generator=g) * 2.0 ** torch.randint(-60, 60, (256,), generator=g).float()]).float()
    for a in (float("inf"), float("-inf"), float("nan")):
        av = torch.full_like(b, a)
        got, ref = _six_terms(av, b), av.double() * b.double()
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), (a, b[torch.isnan(got) != torch.isnan(ref)])
        fin = ~torch.isnan(ref)
        assert torch.equal(got[fin], ref[fin]), a
        got2 = _six_terms(b, av)
        assert torch.equal(torch.isnan(got2), torch.isnan(ref)) and torch.equal(got2[fin], ref[fin]), a
    inf = torch.tensor([float("inf")])
    assert torch.isnan(_six_terms(inf, inf)).all()
