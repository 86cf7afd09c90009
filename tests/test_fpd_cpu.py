"""CPU: the numpy float64 model of the FPD kernels' route (tests/fpd_model.py) against tests/golden/fpd.npz on every case, with the
bounds the GPU suite uses; and the C entries' argument checks, which need no GPU.

  * |model - exact| <= 64 (n1 + n2 + d) 2^-53 scale, every stage stopped before its cap; 1e-6 scale on the graded case;
  * |model - reference| <= |reference - exact| + that bound (triangle inequality; the reference's own gap comes from the golden);
  * the regenerated inputs are the ones the golden was made from (their float64 means agree to rounding)."""
import numpy as np
import pytest

import fpd_model as fm
from helpers import golden


@pytest.fixture(scope="module")
def gold():
    return golden("fpd.npz")


@pytest.mark.parametrize("name", list(fm.CASES))
def test_model_against_exact_and_reference(gold, name):
    a, b = fm.case_inputs(name)
    m1, _ = fm.moments(a)
    np.testing.assert_allclose(m1, gold[name + "|mu64_1"], rtol=1e-13, atol=1e-300, err_msg="the inputs are not the golden's")
    exact, scale, ref = float(gold[name + "|exact"]), float(gold[name + "|scale"]), float(gold[name + "|ref"])
    value, its = fm.fpd(a, b)
    err, gap, bound = abs(value - exact) / scale, abs(ref - exact) / scale, fm.bound(name)
    print("%s: model %.15e exact %.15e err/scale %.2e bound %.2e reference gap %.2e iterations %s" % (name, value, exact, err, bound, gap, its))
    assert err <= bound, (name, err, bound)
    assert abs(value - ref) / scale <= gap + bound, (name, value, ref)
    if name not in fm.GRADED:
        assert max(its) < fm.CAP, (name, its)


def test_mean1000_differs_from_the_reference_on_purpose(gold):
    """np.mean of float32 activations is float32: the reference is 7e-4 of scale off the exact value, the float64 route is not."""
    name = "mean1000"
    exact, scale, ref = float(gold[name + "|exact"]), float(gold[name + "|scale"]), float(gold[name + "|ref"])
    assert abs(ref - exact) / scale > 1e-4
    assert abs(float(gold[name + "|ref_cfd"]) - exact) / scale < 1e-6          # its sqrtm alone, on float64 means, is fine
    value, _ = fm.fpd(*fm.case_inputs(name))
    assert abs(value - exact) / scale <= fm.bound(name)


def test_argument_validation_without_gpu():
    from spgan import _lib
    lib = _lib.load()
    assert lib.spgan_fpd_max_iterations() == fm.CAP
    assert lib.spgan_fpd_distance_ws_bytes(1) == 0 and lib.spgan_fpd_distance_ws_bytes(2049) == 0
    assert lib.spgan_fpd_distance_ws_bytes(512) >= 6 * 512 * 512 * 8
    assert lib.spgan_fpd_moments_ws_bytes(0, 16) == 0 and lib.spgan_fpd_moments_ws_bytes(300, 16) == 3 * 16 * 8
    assert lib.spgan_f64_reduce_ws_bytes() == 256 * 8
    assert lib.spgan_f64_gemm(1, 1, 1, 16, 0, 1.0, 0.0, 0.0, None) == -22             # C aliases A
    assert lib.spgan_f64_gemm(1, 2, 3, 1, 0, 1.0, 0.0, 0.0, None) == -22              # d < 2
    assert lib.spgan_f64_gemm(1, 2, 3, 2049, 0, 1.0, 0.0, 0.0, None) == -22
    assert lib.spgan_f64_reduce(3, 1, 2, 16, 3, 4, None) == -22
    assert lib.spgan_f64_reduce(2, 1, None, 16, 3, 4, None) == -22
    assert lib.spgan_fpd_moments_update(1, 0, 16, 0, 2, 3, 4, 1 << 20, None) == -22   # no rows
    assert lib.spgan_fpd_moments_update(1, 8, 16, 0, 2, 3, 4, 8, None) == -22         # workspace too small
    assert lib.spgan_fpd_distance(1, 2, 3, 4, 16, 5, 6, 8, None) == -22               # workspace too small
    assert lib.spgan_fpd_distance(1, 2, 3, 4, 1, 5, 6, 1 << 30, None) == -22
