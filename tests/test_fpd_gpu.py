"""GPU: the float64 MFMA kernels of csrc/frechet.hip and spgan.fpd on top of them, against tests/golden/fpd.npz.

  * product and reductions: element by element against numpy float64 with the standard forward bound, at one tile, ragged sizes, and
    on both sides of the tile-size switch at d = 1664; asymmetric operands (a transposed C write does not pass), op(A) = A^T, the
    alpha / beta / diag epilogue;
  * statistics: mean and cov against the golden's float64 values entry by entry -- the mean within 8 (n + 1) 2^-53 max|mean|, the
    covariance within 8 (n + 1) 2^-53 max|cov| (a float64 mean cannot be closer than its own rounding, so each is measured in its own
    unit); an update in chunks of 1, 7 and 64 rows within the same bound of the one-shot result;
  * distance against the exact value: 64 (n1 + n2 + d) 2^-53 scale, every stage stopped before its cap; 1e-6 scale on the graded case;
  * distance against the reference: |ours - reference| <= |reference - exact| + that bound (triangle inequality);
  * two calls return equal bits;
  * the host side: get_activations, save / load, the ValueError cases, the two opt-in drivers of spgan.gan_metrics.

Measured on MI355X (|ours - exact| / scale, iterations of sqrt(S1), sqrt(S2), polar): profiles/fpd_accuracy.json, written by
tools/fpd_accuracy.py."""
import functools

import numpy as np
import pytest
import torch

import fpd_model as fm
from helpers import golden
from spgan import _lib, fpd
from spgan import gan_metrics as gm
from spgan.ops import _p, _s

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def gold():
    return golden("fpd.npz")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    a, b = fm.case_inputs(name)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def _rand64(name, shape):
    return fm.fr.uniform(name, shape, -1.0, 1.0).double().numpy() + 1e-9 * fm.fr.uniform(name + ".lo", shape).double().numpy()


# ------------------------------------------------------------------------------------------------ product and reductions
@pytest.mark.parametrize("d", [2, 16, 20, 72, 129, 1031, 1663, 1671])
@pytest.mark.parametrize("trans_a", [0, 1])
def test_f64_gemm(d, trans_a):
    A, B, C0 = _rand64("fpd.gemm.A%d" % d, (d, d)), _rand64("fpd.gemm.B%d" % d, (d, d)), _rand64("fpd.gemm.C%d" % d, (d, d))
    opA = A.T if trans_a else A
    lib = _lib.load()
    prod, aprod = opA @ B, np.abs(opA) @ np.abs(B)
    for alpha, beta, diag in ((1.0, 0.0, 0.0), (-0.5, 0.0, 1.5), (0.75, -2.0, 0.25)):
        want = alpha * prod + beta * C0 + diag * np.eye(d)
        mag = abs(alpha) * aprod + abs(beta) * np.abs(C0) + abs(diag) * np.eye(d)
        a, b, c = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A, B, C0))
        _lib.check(lib.spgan_f64_gemm(_p(a), _p(b), _p(c), d, trans_a, alpha, beta, diag, _s()), "f64_gemm", d=d)
        err = np.abs(c.cpu().numpy() - want)
        # a sum of d products on each side (ours, numpy's) plus the four operations of the epilogue on each: (2 d + 8) u sum|a||b|
        assert (err <= (2 * d + 8) * U * mag).all(), (d, trans_a, alpha, float((err / mag).max()))
        c2 = torch.from_numpy(np.ascontiguousarray(C0)).cuda()
        _lib.check(lib.spgan_f64_gemm(_p(a), _p(b), _p(c2), d, trans_a, alpha, beta, diag, _s()), "f64_gemm", d=d)
        assert torch.equal(c, c2)


def test_f64_gemm_identity_with_asymmetric_operand():
    """A = I with B[i][j] = 100 i + j: exact in float64, and a row/column swap in the C write cannot pass."""
    d = 37
    B = (100.0 * np.arange(d)[:, None] + np.arange(d)[None, :]).astype(np.float64)
    a, b = torch.eye(d, dtype=torch.float64).cuda(), torch.from_numpy(B).cuda()
    c = torch.full((d, d), -1.0, dtype=torch.float64).cuda()
    _lib.check(_lib.load().spgan_f64_gemm(_p(a), _p(b), _p(c), d, 0, 1.0, 0.0, 0.0, _s()), "f64_gemm")
    np.testing.assert_array_equal(c.cpu().numpy(), B)
    _lib.check(_lib.load().spgan_f64_gemm(_p(b), _p(a), _p(c), d, 1, 1.0, 0.0, 0.0, _s()), "f64_gemm")      # B^T I
    np.testing.assert_array_equal(c.cpu().numpy(), B.T)


@pytest.mark.parametrize("d", [2, 33, 256, 1031])
def test_f64_reductions(d):
    A, B = _rand64("fpd.red.A%d" % d, (d, d)), _rand64("fpd.red.B%d" % d, (d, d))
    lib = _lib.load()
    a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    ws = torch.empty((lib.spgan_f64_reduce_ws_bytes() // 8,), dtype=torch.float64).cuda()
    got = []
    for rep in range(2):
        out = torch.empty((3,), dtype=torch.float64).cuda()
        for kind in range(3):
            _lib.check(lib.spgan_f64_reduce(kind, _p(a), _p(b), d, out.data_ptr() + 8 * kind, _p(ws), _s()), "f64_reduce", kind=kind)
        got.append(out.clone())
    assert torch.equal(got[0], got[1])
    tr, fro, dot = got[0].cpu().numpy()
    n = d * d
    assert abs(tr - np.trace(A)) <= 2 * d * U * np.abs(np.diag(A)).sum()
    assert abs(fro - np.sqrt((A * A).sum())) <= 2 * n * U * np.sqrt((A * A).sum())
    assert abs(dot - (A * B).sum()) <= 2 * n * U * np.abs(A * B).sum()


# ------------------------------------------------------------------------------------------------ statistics
def _check_stats(st_mean, st_cov, mu64, cov, n, d, what):
    stride = fm.COV_STRIDE if d >= 128 else 1
    bound = fm.stats_bound(n)
    em = np.abs(st_mean.cpu().numpy() - mu64).max() / max(np.abs(mu64).max(), 1e-300)
    ec = np.abs(st_cov.cpu().numpy().reshape(-1)[::stride] - cov).max() / max(np.abs(cov).max(), 1e-300)
    print("%s: mean err %.2e cov err %.2e bound %.2e" % (what, em, ec, bound))
    assert em <= bound and ec <= bound, (what, em, ec, bound)


@pytest.mark.parametrize("name", list(fm.CASES))
def test_statistics(gold, name):
    d = fm.CASES[name][0]
    for k, x in zip("12", _inputs(name)):
        n = x.shape[0]
        mean, cov = fpd.activation_statistics(x)
        assert mean.dtype == torch.float64 and cov.dtype == torch.float64 and mean.is_cuda and cov.shape == (d, d)
        assert torch.equal(cov, cov.t())
        mu64, c64 = gold["%s|mu64_%s" % (name, k)], gold["%s|cov%s" % (name, k)]
        _check_stats(mean, cov, mu64, c64, n, d, "%s set %s one shot" % (name, k))
        mean2, cov2 = fpd.activation_statistics(x)
        assert torch.equal(mean, mean2) and torch.equal(cov, cov2)
        if n < 3:
            continue
        for chunk in (1, 7, 64):
            st = fpd.ActivationStatistics()
            for lo in range(0, n, chunk):
                st.update(x[lo:lo + chunk])
            assert st.count == n
            _check_stats(st.mean, st.cov, mu64, c64, n, d, "%s set %s chunks of %d" % (name, k, chunk))
            scale = cov.abs().max().item()
            assert (st.cov - cov).abs().max().item() <= fm.stats_bound(n) * scale
            assert (st.mean - mean).abs().max().item() <= fm.stats_bound(n) * mean.abs().max().item()


def test_statistics_wide_tiles():
    """d >= 1024 takes the 64 x 64 tiles in the Gram kernel: ragged d = 1031, n = 70 (more than one k step, not a multiple of 16)."""
    x = fm.fr.normal("fpd.wide.x", (70, 1031), std=1.0, mean=0.5)
    mean, cov = fpd.activation_statistics(x.cuda())
    m64, c64 = fm.moments(x.numpy())
    assert np.abs(mean.cpu().numpy() - m64).max() <= fm.stats_bound(70) * np.abs(m64).max()
    assert np.abs(cov.cpu().numpy() - c64).max() <= fm.stats_bound(70) * np.abs(c64).max()


# ------------------------------------------------------------------------------------------------ distance
@pytest.mark.parametrize("name", list(fm.CASES))
def test_distance(gold, name):
    a, b = _inputs(name)
    exact, scale, ref = float(gold[name + "|exact"]), float(gold[name + "|scale"]), float(gold[name + "|ref"])
    m1, s1 = fpd.activation_statistics(a)
    m2, s2 = fpd.activation_statistics(b)
    info = fpd.frechet_distance_info(m1, s1, m2, s2)
    value, its = info["distance"], info["iterations"]
    err, gap, bound = abs(value - exact) / scale, abs(ref - exact) / scale, fm.bound(name)
    print("%s: ours %.15e exact %.15e err/scale %.2e bound %.2e reference gap %.2e iterations %s" % (name, value, exact, err, bound, gap, its))
    assert not info["used_eps"]
    assert value == fpd.FPD(a, b)
    assert err <= bound, (name, err, bound)
    assert abs(value - ref) / scale <= gap + bound, (name, value, ref)
    if name not in fm.GRADED:
        assert max(its) < fm.CAP, (name, its)
    # equal bits on a second call, on the device
    o1 = fpd.frechet_distance_device(m1, s1, m2, s2)
    o2 = fpd.frechet_distance_device(m1, s1, m2, s2)
    assert torch.equal(o1, o2) and o1[0].item() == value


def test_distance_wide_tiles():
    """d = 1671 (64 x 64 tiles in the moments and in every product of the driver), n 40 / 50: against the exact value computed here."""
    a = fm._relu_features("fpd.wide", ".a", 40, 1671, 0.3)
    b = fm._relu_features("fpd.wide", ".b", 50, 1671, 0.1)
    exact, scale = fm.exact(a, b)
    info = fpd.frechet_distance_info(*fpd.activation_statistics(torch.from_numpy(a).cuda()), *fpd.activation_statistics(torch.from_numpy(b).cuda()))
    err, bound = abs(info["distance"] - exact) / scale, 64.0 * (40 + 50 + 1671) * U
    print("wide1671: err/scale %.2e bound %.2e iterations %s" % (err, bound, info["iterations"]))
    assert err <= bound and max(info["iterations"]) < fm.CAP


def test_distance_accepts_numpy_and_float32(gold):
    a, b = _inputs("tile16")
    m1, s1 = fpd.activation_statistics(a)
    m2, s2 = fpd.activation_statistics(b)
    v = fpd.calculate_frechet_distance(m1, s1, m2, s2)
    assert isinstance(v, float)
    assert fpd.calculate_frechet_distance(m1.cpu().numpy(), s1.cpu().numpy(), m2.cpu().numpy(), s2.cpu().numpy()) == v
    v32 = fpd.calculate_frechet_distance(m1.float(), s1.float(), m2.float(), s2.float())
    assert abs(v32 - v) <= 1e-5 * float(gold["tile16|scale"])
    z = torch.zeros((16, 16), dtype=torch.float64).cuda()                    # a zero covariance: the square root of 0 is 0
    assert fpd.calculate_frechet_distance(m1, z, m1, z) == 0.0


# ------------------------------------------------------------------------------------------------ host side
class _Feat(torch.nn.Module):
    """(logits, activations [B,1,8]) from clouds [B,N,3]; dropout makes eval() visible; records its batch sizes."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 8)
        self.drop = torch.nn.Dropout(0.5)
        self.batches = []

    def forward(self, pc):
        self.batches.append((pc.shape[0], self.training))
        f = self.drop(self.lin(pc)).max(dim=1, keepdim=True)[0]
        return f.sum(-1), f


def test_get_activations():
    m = _Feat().cuda().train()
    pcs = fm.fr.normal("fpd.host.pcs", (23, 32, 3)).cuda()
    acts = fpd.get_activations(pcs, m, batch_size=5, dims=512)
    assert not m.training and m.batches == [(5, False)] * 4 + [(3, False)]
    assert acts.shape == (23, 8) and acts.is_cuda and not acts.requires_grad and acts.grad_fn is None
    with torch.no_grad():
        want = torch.cat([m(pcs[i:i + 1])[1].squeeze(1) for i in range(23)])
    assert torch.allclose(acts, want, rtol=1e-6, atol=1e-7)                   # row i is cloud i
    two = fpd.extract_acts_with_model([pcs, pcs[:7]], m, batch_size=16)
    assert [tuple(t.shape) for t in two] == [(23, 8), (7, 8)] and torch.equal(two[1], two[0][:7])


def test_save_load_and_state_dict(tmp_path):
    a, b = _inputs("ragged20")
    st = fpd.ActivationStatistics().update(a[:30])
    other = fpd.ActivationStatistics()
    other.load_state_dict(st.state_dict())
    st.update(a[30:])
    other.update(a[30:])
    assert other.count == st.count == a.shape[0] and torch.equal(other.cov, st.cov) and torch.equal(other.mean, st.mean)
    path = str(tmp_path / "stats.npz")
    st.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ["m", "s"]
    m, s = fpd.ActivationStatistics.load(path)
    assert m.dtype == np.float64 and np.array_equal(m, st.mean.cpu().numpy()) and np.array_equal(s, st.cov.cpu().numpy())
    m2, s2 = fpd.activation_statistics(b)
    assert fpd.calculate_frechet_distance(m, s, m2, s2) == fpd.calculate_frechet_distance(st.mean, st.cov, m2, s2)   # st: two chunks


def test_value_errors():
    a, b = _inputs("tile16")
    with pytest.raises(ValueError):
        fpd.FPD(a, b[:, :8])                                                  # feature sizes differ
    with pytest.raises(ValueError):
        fpd.FPD(a[:1], b)                                                     # fewer than 2 rows
    with pytest.raises(ValueError):
        fpd.activation_statistics(a[:0])
    with pytest.raises(ValueError):
        fpd.ActivationStatistics().update(a[:1]).cov
    with pytest.raises(ValueError):
        fpd.ActivationStatistics().update(a).update(b[:, :8])
    with pytest.raises(ValueError):
        fpd.FPD(a[:, :1], b[:, :1])                                           # d < 2
    m1, s1 = fpd.activation_statistics(a)
    with pytest.raises(ValueError):
        fpd.calculate_frechet_distance(m1, s1, m1[:8], s1)
    with pytest.raises(ValueError):
        fpd.calculate_frechet_distance(m1, s1, m1, s1[:8, :8])
    with pytest.raises(RuntimeError, match="GPU"):
        fpd.FPD(a.cpu(), b)


def test_compute_all_metrics_fpd():
    fs, fr_ = fm.fr.normal("fpd.drv.fs", (24, 16)).cuda(), fm.fr.normal("fpd.drv.fr", (30, 16), mean=0.2).cuda()
    with pytest.raises(NotImplementedError, match="evaluation.pointnet"):
        gm.compute_all_metrics(fs, fr_, 4, "l2")
    res = gm.compute_all_metrics(fs, fr_, 4, "l2", fpd=True)
    train = gm.compute_all_metrics_train(fs, fr_, None, 4, "l2")
    assert sorted(res) == ["1NN", "6NN", "COV", "FPD", "JSD", "MMD"]
    for k in ("JSD", "COV", "MMD", "1NN"):
        assert res[k] == train[k], k
    assert res["FPD"] == fpd.FPD(fs, fr_) and res["FPD"] > 0.0


def test_compute_all_metrics_train_with_model():
    m = _Feat().cuda()
    s = fm.fr.uniform("fpd.drv.s", (12, 64, 3), -0.45, 0.45).cuda()
    r = fm.fr.uniform("fpd.drv.r", (10, 64, 3), -0.3, 0.3).cuda()
    with pytest.raises(NotImplementedError, match="evaluation.pointnet"):
        gm.compute_all_metrics_train(s, r, None, 4, "CD", True)
    base = gm.compute_all_metrics_train(s, r, m, 4, "CD", False)
    assert base["FPD"] == 0 and base["JSD"] == 0
    res = gm.compute_all_metrics_train(s, r, model=m, batch_size=4, dist_type="CD", use_FPD_JSD=True)
    for k in ("COV", "MMD", "MMD_t", "1NN"):
        assert res[k] == base[k], k
    fa, fb = fpd.extract_acts_with_model([s, r], m, batch_size=4)
    assert res["FPD"] == fpd.FPD(fa, fb) and res["JSD"] == gm.JSD(s, r)
    assert not m.training
