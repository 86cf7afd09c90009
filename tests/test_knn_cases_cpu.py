"""CPU: the clouds of tests/knn_cases.py test what they claim -- no GPU needed.

* exactness: on every lattice case the fp32 expanded form (kernel_model.knn, mode 0) gives the float64 direct-difference graph, so any
  route's distances are exact there and the expected output is an exact integer array;
* the cases bite: enough rows have a tie straddling the cut-off (the k-th and (k+1)-th neighbour at one distance: the tie rule decides
  who is returned) and enough rows do not have themselves at rank 0 (a twin with a lower index: "drop rank 0" is not "drop yourself");
* the closed form of the prototype clouds is the float64 reference's answer.
The floors are conditions on the inputs, not tolerances on a kernel.
"""
import pytest
import torch

import kernel_model as km
import knn_cases as kc

LATTICE = pytest.mark.parametrize("case", kc.LATTICE_CASES, ids=[c.route.split("<")[0] + "-" + kc.case_id(c) for c in kc.LATTICE_CASES])


def test_case_tables():
    """The shapes reach the launches they are listed under (the dispatch of launch_knn / spgan_knn_ws_bytes)."""
    for c in kc.LATTICE_CASES:
        assert c.B in (2, 3) and c.k + 1 <= c.N and c.R in (1, 2, 3) and (c.R == 3) == (c.C <= 5)
    assert all(c.mode == 1 and c.C <= 4 for c in kc.LATTICE_F64)
    assert all(c.mode == 0 and (c.C <= 16 or c.k > 10) for c in kc.LATTICE_F32)
    assert all(c.mode == 0 and 16 < c.C <= 64 and c.k <= 10 for c in kc.LATTICE_MATRIX)
    assert all(c.mode == 0 and 64 < c.C <= 128 and c.k <= 10 for c in kc.LATTICE_MFMA3_128)
    assert {c.N for c in kc.LATTICE_MATRIX} == {11, 31, 32, 33, 64, 65, 96, 97, 129, 161, 257}
    assert {c.C for c in kc.LATTICE_MATRIX} == {17, 40, 64} and {c.k for c in kc.LATTICE_MATRIX} == {1, 7, 10}
    assert len({(c.C, c.N, c.k) for c in kc.LATTICE_CASES}) == len(kc.LATTICE_CASES)
    assert sum(c.C <= 64 for c in kc.MFMA_CHILD_CASES) == 2 and sum(c.C > 64 for c in kc.MFMA_CHILD_CASES) == 2


@LATTICE
def test_lattice_is_exact_in_fp32(case):
    x, ref = kc.lattice(case)
    assert x.dtype == torch.float32 and torch.equal(x, x.round()) and x.abs().max().item() <= case.R
    assert torch.equal(x.bfloat16().float(), x), "a coordinate is not exactly a bfloat16"
    assert torch.equal(km.knn(x, case.B, case.N, case.k, 0), ref), "the fp32 expanded form differs from float64 direct differences"
    if case.mode == 1:
        assert torch.equal(km.knn(x, case.B, case.N, case.k, 1), ref)
    assert ref.dtype == torch.int32 and ref.shape == (case.B * case.N, case.k)
    shape_of = torch.arange(case.B).repeat_interleave(case.N)[:, None]
    assert torch.equal(ref // case.N, shape_of.expand_as(ref).to(torch.int32)), "a neighbour outside the query's shape"


@pytest.mark.parametrize("case", [c for c in kc.LATTICE_CASES if c.k + 1 < c.N], ids=kc.case_id)   # k + 1 == N: nothing to tie with
def test_lattice_has_ties_at_the_cut_off(case):
    x, _ = kc.lattice(case)
    sd = kc.sorted_dist_f64(x, case.B, case.N)[0]
    frac = (sd[:, :, case.k] == sd[:, :, case.k + 1]).double().mean().item()
    print("tie at the cut-off in %.1f %% of rows" % (100 * frac))
    assert frac >= 0.10, frac


@LATTICE
def test_lattice_has_rows_that_are_not_their_own_rank_0(case):
    x, _ = kc.lattice(case)
    order = kc.sorted_dist_f64(x, case.B, case.N)[1]
    frac = (order[:, :, 0] != torch.arange(case.N)[None, :]).double().mean().item()
    print("not rank 0 of the own list: %.1f %% of rows" % (100 * frac))
    assert frac >= 0.02, frac


@pytest.mark.parametrize("m", kc.PROTO_M)
@pytest.mark.parametrize("B,N,C,k", [(2, 130, 3, 10), (2, 130, 20, 20), (2, 256, 3, 10)])
def test_prototype_closed_form(B, N, C, k, m):
    x = kc.prototype_cloud(B, N, C, m, lattice_protos=True)
    assert torch.equal(kc.prototype_expected(B, N, m, k), kc.stable_knn_f64(x, B, N, k))


@pytest.mark.parametrize("m", kc.PROTO_M)
@pytest.mark.parametrize("C", [20, 64, 128])
def test_prototype_fp32_clouds(C, m):
    """The fp32 prototypes of the GPU test are separated (prototype_cloud asserts it) and the float64 reference gives the closed form."""
    k = 20 if C == 20 else 10
    x = kc.prototype_cloud(2, 130, C, m)
    assert torch.equal(kc.prototype_expected(2, 130, m, k), kc.stable_knn_f64(x, 2, 130, k))


def test_prototype_collapsed_cloud_expects_one_to_k():
    exp = kc.prototype_expected(2, 130, 1, 10)
    for b in range(2):
        assert torch.equal(exp[b * 130:(b + 1) * 130], (b * 130 + torch.arange(1, 11)).to(torch.int32).expand(130, 10))


@pytest.mark.parametrize("C,N,k", [(20, 97, 10), (64, 333, 10), (128, 130, 10), (64, 130, 20)])
def test_offset_bound_is_not_vacuous(C, N, k):
    """The derived bound stays below 2 % of the median k-th-neighbour distance, and the fp32 model is inside it."""
    B = 2
    x = kc.offset_cloud(B, N, C)
    tol = kc.offset_tol(x)
    sd = kc.sorted_dist_f64(x, B, N)[0]
    med = sd[:, :, k].median().item()
    err = kc.rank_error(km.knn(x, B, N, k, 0), x, B, N, k, sd)
    print("tol %.4g, median k-th distance %.4g (%.2f %%), fp32 model rank error %.3g" % (tol, med, 100 * tol / med, err))
    assert tol <= 0.02 * med
    assert err <= tol


def _split_product_knn(x, B, N, k, planes):
    """A model of the split-bf16 routes' arithmetic (the six leading cross terms, exact products, fp32 distances); planes = 2 drops lo."""
    C = x.shape[1]
    h, m, l = (t.double().view(B, N, C) for t in kc.split_bf16(x))
    if planes == 2:
        l = torch.zeros_like(l)
    T = lambda a: a.transpose(1, 2)                                                      # noqa: E731
    dot = (h @ T(h) + (h @ T(m) + m @ T(h)) + (h @ T(l) + l @ T(h) + m @ T(m))).float()
    sq = (x * x).sum(-1).view(B, N)
    d = (-2 * dot + sq[:, :, None]) + sq[:, None, :]
    order = torch.sort(d, dim=2, stable=True)[1][:, :, 1:k + 1]
    return (order + (torch.arange(B) * N).view(B, 1, 1)).reshape(B * N, k).to(torch.int32)


def test_aligned_lo_cloud_shows_a_dropped_plane():
    """The planes are what the recipe says, the bound is not vacuous, the three-plane product and the fp32 model are far inside it --
    and the same product without its lo plane is outside: the GPU test on this cloud fails for a kernel that loses the plane."""
    B, N, C, k = kc.ALIGNED_LO_SHAPE
    x = kc.aligned_lo_cloud(B, N, C)
    hi, mid, lo = kc.split_bf16(x)
    assert torch.equal((hi + mid) + lo, x) and hi.min() >= 8.5 and hi.max() <= 11.5
    assert torch.equal(lo, (torch.where(torch.arange(B * N) % 2 == 0, 1.0, -1.0)[:, None] * 2.0 ** -14).expand_as(lo))
    tol = kc.offset_tol(x)
    sd = kc.sorted_dist_f64(x, B, N)[0]
    assert tol <= 0.02 * sd[:, :, k].median().item()
    e32 = kc.rank_error(km.knn(x, B, N, k, 0), x, B, N, k, sd)
    e3 = kc.rank_error(_split_product_knn(x, B, N, k, 3), x, B, N, k, sd)
    e2 = kc.rank_error(_split_product_knn(x, B, N, k, 2), x, B, N, k, sd)
    print("tol %.4g; rank error: fp32 model %.3g, three planes %.3g, lo plane dropped %.3g" % (tol, e32, e3, e2))
    assert e32 <= 0.25 * tol and e3 <= 0.25 * tol
    assert e2 > 2 * tol
