"""CPU: the numpy model of the batch augmentation (tests/augment_model.py) against published Philox vectors, against the reference's
own functions (tests/golden/augment_ref.npz, written by tests/golden/make_golden_augment.py) and against the moments of its draws."""
import os

import numpy as np
import pytest

import augment_model as am

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_ref.npz")
Y, Z = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
TWO_PI = 2 * np.pi


@pytest.mark.parametrize("counter,key,expect", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_philox_known_answers(counter, key, expect):
    """The three Philox4x32-10 vectors published with Random123 (kat_vectors)."""
    assert am.philox4x32_10(counter, key).tolist() == expect


def test_host_stream_equals_model():
    """spgan.augment's host-side Philox (the epoch order) is the model's stream; the order is a permutation and moves with the epoch."""
    from spgan import augment
    seed, step = 0xdeadbeefcafef00d, (1 << 32) + 3
    assert np.array_equal(augment.philox_words(seed, 4, 0, step, 1001), am.words(seed, 4, 0, step, 1001))
    o0, o1 = augment.epoch_order(seed, 0, 40), augment.epoch_order(seed, 1, 40)
    assert sorted(o0.tolist()) == list(range(40)) and not np.array_equal(o0, o1)
    assert np.array_equal(o0, am.permutation(seed, 0, 0, 40, keys=am.words(seed, 4, 0, 0, 40)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def _close(got, want):
    assert got.shape == want.shape
    err = float(np.abs(got - want.astype(np.float64)).max())
    assert err <= 1e-6, err


def _per_cloud(gold, tag, key, fn):
    """fn(cloud index, draws of that cloud) -> (A, t); the recorded output is every cloud under its map."""
    x, d = gold[key], gold[tag + "|draws"]
    d = d.reshape(x.shape[0], -1)
    _close(np.stack([am.apply_map(x[k], *fn(k, d[k])) for k in range(x.shape[0])]), gold[tag + "|out0"])


def test_provider_rotations(gold):
    """pc @ R with provider's matrices; rotate_point_cloud_z's matrix is Rz transposed; normals are rotated, nothing else."""
    _per_cloud(gold, "provider.rotate_point_cloud", "xyz", lambda k, d: am.compose(rot=am.rot_axis(d[0] * TWO_PI, Y)))
    _per_cloud(gold, "provider.rotate_point_cloud_z", "xyz", lambda k, d: am.compose(rot=am.rot_axis(d[0] * TWO_PI, Z), transpose=1))
    _per_cloud(gold, "provider.rotate_point_cloud_with_normal", "xyzn", lambda k, d: am.compose(rot=am.rot_axis(d[0] * TWO_PI, Y)))
    pert = lambda k, d: am.compose(perturb=am.rot_euler(*am.clip_noise(d, 0.06, 0.18)))          # noqa: E731
    _per_cloud(gold, "provider.rotate_perturbation_point_cloud", "xyz", pert)
    _per_cloud(gold, "provider.rotate_perturbation_point_cloud_with_normal", "xyzn", pert)


def test_provider_scale_shift_jitter_dropout(gold):
    _per_cloud(gold, "provider.shift_point_cloud", "xyz", lambda k, d: am.compose(translate=d))
    _per_cloud(gold, "provider.random_scale_point_cloud", "xyz", lambda k, d: am.compose(scale=d[0]))
    x = gold["xyz"]
    g = gold["provider.jitter_point_cloud|draws"].reshape(x.shape)
    _close(x.astype(np.float64) + am.clip_noise(g, 0.01, 0.05), gold["provider.jitter_point_cloud|out0"])
    d = gold["provider.random_point_dropout|draws"].reshape(x.shape[0], 1 + x.shape[1])
    got = np.stack([am.drop_rows(x[k], d[k, 1:] <= d[k, 0] * 0.875) for k in range(x.shape[0])])
    assert (d[:, 1:] <= d[:, :1] * 0.875).any()                                                   # rows were dropped: they take row 0
    assert np.array_equal(got, gold["provider.random_point_dropout|out0"])


def test_point_operation_pairs(gold):
    """The *_and_gt functions: one draw, the same map on both clouds.  y_rotated keeps Ry of the three drawn angles; else Rz Ry Rx."""
    x, g = gold["xyz"][0], gold["gt"][0]
    for tag, fn in (("point_operation.rotate_point_cloud_and_gt.y", lambda d: am.compose(rot=am.rot_euler(0.0, d[1] * TWO_PI, 0.0))),
                    ("point_operation.rotate_point_cloud_and_gt.xyz", lambda d: am.compose(rot=am.rot_euler(*(d * TWO_PI)))),
                    ("point_operation.shift_point_cloud_and_gt", lambda d: am.compose(translate=d)),
                    ("point_operation.random_scale_point_cloud_and_gt", lambda d: am.compose(scale=d[0]))):
        A, t = fn(gold[tag + "|draws"])
        _close(am.apply_map(x, A, t), gold[tag + "|out0"])
        _close(am.apply_map(g, A, t), gold[tag + "|out1"])


def test_data_utils_classes(gold):
    """points @ R.T with angle_axis matrices (the other side from provider), per-axis scale and translation, PointcloudTranslate's one
    scalar for all three axes, dropped rows take row 0, PointcloudRotatebyAngle's pc @ Ry on xyz and normals."""
    x, xn = gold["xyz"], gold["xyzn"]
    d = gold["data_utils.PointcloudRotate|draws"]
    _close(am.apply_map(x[0], *am.compose(rot=am.rot_axis(d[0] * TWO_PI, Y), transpose=1)), gold["data_utils.PointcloudRotate|out0"])
    # the transposed convention is not the plain one: the pin distinguishes them
    assert np.abs(am.apply_map(x[0], *am.compose(rot=am.rot_axis(d[0] * TWO_PI, Y))) - gold["data_utils.PointcloudRotate|out0"]).max() > 1e-3
    d = gold["data_utils.PointcloudRotatePerturbation|draws"]
    A, t = am.compose(perturb=am.rot_euler(*am.clip_noise(d, 0.06, 0.18)), transpose=1)
    _close(am.apply_map(x[0], A, t), gold["data_utils.PointcloudRotatePerturbation|out0"])
    _per_cloud(gold, "data_utils.PointcloudRotatePerturbation_batch.normal", "xyzn",
               lambda k, d: am.compose(perturb=am.rot_euler(*am.clip_noise(d, 0.06, 0.18)), transpose=1))
    _per_cloud(gold, "data_utils.PointcloudScaleAndTranslate", "xyz", lambda k, d: am.compose(scale=d[:3], translate=d[3:]))
    d = gold["data_utils.PointcloudTranslate|draws"]
    assert d.shape == (1,)
    _close(am.apply_map(x[0], *am.compose(translate=d[0])), gold["data_utils.PointcloudTranslate|out0"])
    d = gold["data_utils.PointcloudRandomInputDropout|draws"]
    assert np.array_equal(am.drop_rows(x[0], d[1:] <= d[0] * 0.875), gold["data_utils.PointcloudRandomInputDropout|out0"])
    _close(np.stack([am.apply_map(c, *am.compose(rot=am.rot_euler(0.0, 0.7, 0.0))) for c in xn]), gold["data_utils.PointcloudRotatebyAngle|out0"])


def test_float32_evaluation_tracks_float64():
    """The model's float32 evaluation (the e_ref of the GPU tests) stays within a few float32 roundings of its float64 one."""
    cfg = am.make_cfg(permute=1, rotate=2, perturb=1, scale=2, translate=1, jitter=1, dropout=1)
    data = np.random.RandomState(1).uniform(-1, 1, (3, 40, 6)).astype(np.float32)
    r64 = am.run(data, [2, 0], 33, cfg, seed=11, step=5)
    r32 = am.run(data, [2, 0], 33, cfg, seed=11, step=5, dt=np.float32)
    assert np.array_equal(r64["mask"], r32["mask"]) and np.array_equal(r64["perm"], r32["perm"]) and r64["mask"].any()
    assert np.abs(r64["out"] - r32["out"]).max() < 2e-6
    assert np.array_equal(r64["out"][r64["mask"]], np.repeat(r64["out"][:, :1], 33, axis=1)[r64["mask"]])


def test_draw_moments():
    """2^16 draws of the model: uniform mean, normal mean and variance."""
    w = am.words(seed=0x9e3779b97f4a7c15, purpose=2, b=3, step=1 << 33, n=1 << 17)
    u = am.uni(w[:1 << 16])
    assert abs(u.mean() - 0.5) < 0.01 and u.min() >= 0.0 and u.max() < 1.0
    g0, g1 = am.normal2(w[0::2][:1 << 15], w[1::2][:1 << 15])
    g = np.concatenate([g0, g1])
    assert g.size == 1 << 16 and abs(g.mean()) < 0.02 and abs(g.var() - 1.0) < 0.02
