"""GPU: csrc/augment.hip through spgan.augment against the numpy model of tests/augment_model.py (written from the header): the Philox
words, the permutation and the dropout mask bit for bit, parameters and outputs against the float64 evaluation within
max(4 e_ref, 8 * 2^-24 * scale), e_ref the model's own float32 evaluation; the call counter eagerly, under spgan.CapturedBody and across
a mid-epoch resume of DeviceDataset."""
import numpy as np
import pytest
import torch

import augment_model as am

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDS = (0xdeadbeefcafef00d, 0x8000000000000001)            # high bits set in both halves of the key


def _aug(cfg, seed, **kw):
    from spgan.augment import BatchAugment
    return BatchAugment(
        seed, permute=bool(cfg["permute"]), rotate={0: None, 1: "axis", 2: "xyz"}[cfg["rotate"]], axis=cfg["axis"], transpose=bool(cfg["transpose"]),
        perturb=(cfg["perturb_sigma"], cfg["perturb_clip"]) if cfg["perturb"] else None,
        scale=(cfg["scale_lo"], cfg["scale_hi"]) if cfg["scale"] else None, scale_per_axis=cfg["scale"] == 2,
        translate=cfg["translate_range"] if cfg["translate"] else None, translate_scalar=cfg["translate"] == 2,
        jitter=(cfg["jitter_sigma"], cfg["jitter_clip"]) if cfg["jitter"] else None, dropout=cfg["dropout_max"] if cfg["dropout"] else None, **kw)


def _set_step(aug, step):
    aug.set_state({"seed": aug.seed, "step": step})


def _data(S, P, C, seed=0):
    rs = np.random.RandomState(seed)
    d = rs.uniform(-1, 1, (S, P, C)).astype(np.float32)
    if C == 6:
        d[..., 3:] /= np.linalg.norm(d[..., 3:], axis=-1, keepdims=True)
    return d


def _bnc(out, layout):
    return (out if layout == "bnc" else out.transpose(1, 2)).cpu().numpy()


def _keys_tensor(keys):
    return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).to(DEV)


def test_philox_words_equal_model():
    from spgan import _lib
    lib = _lib.load()
    step, n = (1 << 32) + 3, 4096
    out = torch.empty((n,), dtype=torch.int32, device=DEV)
    for seed in SEEDS:
        for purpose in (0, 1, 2, 3, 4):
            _lib.check(lib.spgan_philox_fill(seed, purpose, 7, step, n, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "philox_fill")
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, am.words(seed, purpose, 7, step, n)), (hex(seed), purpose)
    assert lib.spgan_philox_fill(1, 256, 0, 0, 4, out.data_ptr(), None) == -22 and lib.spgan_philox_fill(1, 0, 1 << 24, 0, 4, out.data_ptr(), None) == -22


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1000, 2048, 2049, 8192])
def test_permutation_equals_model(N):
    """Sizes on both sides of a wave, of the sort's power-of-two padding and of its 1024-thread workgroup, up to the limit."""
    seed, step = SEEDS[0], 5
    data = _data(4, N + (3 if N < 8192 else 0), 3, seed=N)
    aug = _aug(am.make_cfg(permute=1), seed, device=DEV)
    dd = torch.from_numpy(data).to(DEV)
    for B in (1, 3):
        index = [3, 0, 3][:B]
        want = np.stack([data[index[b]][:N][am.permutation(seed, step, b, N)] for b in range(B)])
        for layout in ("bnc", "bcn"):
            _set_step(aug, step)
            out, rec = aug(dd, torch.tensor(index, device=DEV), n=N, layout=layout)
            assert np.array_equal(_bnc(out, layout), want), (B, layout)
            assert aug.get_state()["step"] == step + 1


def test_injected_keys():
    """All-equal keys: ties go to the lower index, the identity.  Two distinct values: a stable partition.  A given order, encoded."""
    N, B = 300, 2
    data = _data(2, N, 3)
    dd, index = torch.from_numpy(data).to(DEV), torch.tensor([1, 0], device=DEV)
    aug = _aug(am.make_cfg(), 1, device=DEV)                                   # the permutation is off: keys turn it on for the call
    out, _ = aug(dd, index, keys=_keys_tensor(np.full((B, N), 0xfffffffe)))
    assert np.array_equal(out.cpu().numpy(), data[[1, 0]])
    two = np.random.RandomState(3).randint(0, 2, (B, N)).astype(np.uint32) * np.uint32(0x80000000) + np.uint32(5)
    out, _ = aug(dd, index, keys=_keys_tensor(two))
    want = np.stack([data[[1, 0][b]][np.argsort(two[b], kind="stable")] for b in range(B)])
    assert np.array_equal(out.cpu().numpy(), want)
    assert aug.get_state()["step"] == 0                                        # nothing was drawn
    out, _ = aug(dd, index, keys=torch.from_numpy(two.astype(np.int64)).to(DEV))          # int64 values are accepted as well
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("C", [3, 6])
def test_gather_only_is_exact(C):
    data = _data(6, 50, C, seed=C)
    dd = torch.from_numpy(data).to(DEV)
    index = [3, 3, 0, 5]
    aug = _aug(am.make_cfg(), 9, device=DEV)
    for layout in ("bnc", "bcn"):
        for n in (37, 50):
            out, rec = aug(dd, torch.tensor(index, device=DEV), n=n, layout=layout)
            assert np.array_equal(_bnc(out, layout), data[index][:, :n])
    r = rec.cpu().numpy()
    assert np.array_equal(r[:, :9], np.tile(np.eye(3, dtype=np.float32).reshape(-1), (4, 1))) and not r[:, 9:13].any()
    assert aug.get_state()["step"] == 0


ALL = dict(permute=1, rotate=1, perturb=1, scale=1, translate=1, jitter=1, dropout=1)
STAGE_CASES = {
    "rotate_y": dict(rotate=1),
    "rotate_axis_T": dict(rotate=1, axis=(1.0, 2.0, 3.0), transpose=1),
    "rotate_xyz": dict(rotate=2),
    "rotate_xyz_T": dict(rotate=2, transpose=1),
    "perturb": dict(perturb=1),
    "perturb_T": dict(perturb=1, transpose=1),
    "scale": dict(scale=1),
    "scale_axes": dict(scale=2, scale_lo=2. / 3., scale_hi=1.5),
    "translate": dict(translate=1, translate_range=0.2),
    "translate_scalar": dict(translate=2),
    "jitter": dict(jitter=1),
    "dropout": dict(dropout=1),
    "dropout_zero": dict(dropout=1, dropout_max=0.0),
    "all": dict(ALL),
    "all_T": dict(ALL, transpose=1, rotate=2, scale=2, translate=2),
}


def _bound(got, r64, r32):
    e_ref = float(np.abs(r32.astype(np.float64) - r64).max())
    scale = float(np.abs(r64).max())
    err = float(np.abs(got.astype(np.float64) - r64).max())
    return err, max(4 * e_ref, 8 * 2.0 ** -24 * scale)


@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("case", sorted(STAGE_CASES))
def test_stages_against_float64_model(case, C):
    B, N, seed, step = 5, 257, SEEDS[1], (1 << 32) + 3
    cfg = am.make_cfg(**STAGE_CASES[case])
    data = _data(7, N + 2, C, seed=17)
    index = [6, 0, 3, 3, 1]
    aug = _aug(cfg, seed, device=DEV)
    _set_step(aug, step)
    out, rec = aug(torch.from_numpy(data).to(DEV), torch.tensor(index, device=DEV), n=N)
    out, rec = out.cpu().numpy(), rec.cpu().numpy()
    r64 = am.run(data, index, N, cfg, seed, step)
    r32 = am.run(data, index, N, cfg, seed, step, dt=np.float32)
    # the record
    err, tol = _bound(rec[:, :9].reshape(B, 3, 3), r64["A"], r32["A"])
    print("%s C=%d A: err %.3e bound %.3e" % (case, C, err, tol))
    assert err <= tol
    err, tol = _bound(rec[:, 9:12], r64["t"], r32["t"])
    print("%s C=%d t: err %.3e bound %.3e" % (case, C, err, tol))
    assert err <= tol
    assert np.array_equal(rec[:, 12], r64["ratio"])
    bits = rec[:, 13:15].copy().view(np.uint32)
    assert (bits[:, 0] == (step & 0xffffffff)).all() and (bits[:, 1] == (step >> 32)).all() and not rec[:, 15].any()
    if not cfg["scale"]:
        A = rec[:, :9].reshape(B, 3, 3).astype(np.float64)
        assert np.abs(A @ A.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
    # the dropout mask, read off the output: a dropped row IS output row 0
    same = (out == out[:, :1]).all(axis=2)
    assert np.array_equal(same[:, 1:], r64["mask"][:, 1:])
    if case == "dropout":
        assert r64["mask"].any() and not r64["mask"].all()
    if case == "dropout_zero":
        assert not r64["mask"].any() and not rec[:, 12].any()
    # the output
    err, tol = _bound(out, r64["out"], r32["out"])
    print("%s C=%d out: err %.3e bound %.3e" % (case, C, err, tol))
    assert err <= tol
    assert aug.get_state()["step"] == step + 1


def test_apply_only_mode_equals_item_transform():
    from spgan.augment import BatchAugment
    from spgan.dataset import item_transform
    B, N = 4, 129
    rs = np.random.RandomState(5)
    data = _data(B, N, 3, seed=6)
    perm = np.stack([rs.permutation(N) for _ in range(B)])
    keys = np.empty((B, N), dtype=np.uint32)
    for b in range(B):
        keys[b, perm[b]] = np.arange(N, dtype=np.uint32) * np.uint32(7919)        # ascending along the wanted order
    angle = torch.from_numpy(rs.uniform(0, 2 * np.pi, B).astype(np.float32)).to(DEV)
    scale = torch.from_numpy(rs.uniform(0.8, 1.25, B).astype(np.float32)).to(DEV)
    dd = torch.from_numpy(data).to(DEV)
    aug = BatchAugment(3, device=DEV)
    params = BatchAugment.params_from(angle_y=angle, scale=scale)
    out, rec = aug(dd, torch.arange(B, device=DEV), keys=_keys_tensor(keys), params=params)
    assert torch.equal(rec[:, :12], params[:, :12]) and aug.get_state()["step"] == 0
    want = item_transform(dd, torch.from_numpy(perm).to(DEV), angle, scale).cpu().numpy()
    cfg, p = am.make_cfg(permute=1), params.cpu().numpy()
    r64 = am.run(data, list(range(B)), N, cfg, 3, 0, keys=keys, params=p)
    r32 = am.run(data, list(range(B)), N, cfg, 3, 0, keys=keys, params=p, dt=np.float32)
    assert np.array_equal(r64["perm"], perm)
    err, tol = _bound(out.cpu().numpy(), r64["out"], r32["out"])
    assert err <= tol, (err, tol)
    d = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
    print("apply-only vs item_transform: %.3e (bound %.3e)" % (d, tol))
    assert d <= tol
    # the same map on a second cloud (the gt of the *_and_gt functions), with normals
    gt = _data(B, 77, 6, seed=8)
    got = aug.apply(params, torch.from_numpy(gt).to(DEV)).cpu().numpy()
    g64 = np.stack([am.apply_map(gt[b], p[b, :9].reshape(3, 3), p[b, 9:12]) for b in range(B)])
    g32 = np.stack([am.apply_map(gt[b], p[b, :9].reshape(3, 3), p[b, 9:12], dt=np.float32) for b in range(B)])
    err, tol = _bound(got, g64, g32)
    assert err <= tol, (err, tol)


def test_counter_eager_resume_and_captured():
    import spgan
    cfg = am.make_cfg(**ALL)
    data = torch.from_numpy(_data(9, 130, 3, seed=2)).to(DEV)
    index = torch.tensor([4, 8, 0, 4], device=DEV)
    a = _aug(cfg, 77, device=DEV)
    eager = [a(data, index, n=128)[0].clone() for _ in range(3)]
    assert a.get_state() == {"seed": 77, "step": 3}
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[1], eager[2])
    b = _aug(cfg, 77, device=DEV)
    b.set_state({"seed": 77, "step": 2})
    assert torch.equal(b(data, index, n=128)[0], eager[2])
    c, d = _aug(cfg, 77, device=DEV), _aug(cfg, 77, device=DEV)               # equal state, equal bits
    d.set_state(c.get_state())
    oc, rc = c(data, index, n=128)
    od, rd = d(data, index, n=128)
    assert torch.equal(oc, od) and torch.equal(rc.view(torch.int32), rd.view(torch.int32)) and torch.equal(oc, eager[0])
    g = _aug(cfg, 77, device=DEV)
    body = spgan.CapturedBody(lambda idx: g(data, idx, n=128)[0], modules=(), warmup=0)
    for k in range(3):
        out = body(index)
        assert torch.equal(out, eager[k]), k
    assert not body.eager and g.get_state()["step"] == 3


def test_dataset_mid_epoch_resume():
    from spgan.augment import BatchAugment
    from spgan.dataset import DeviceDataset
    src = _data(40, 64, 3, seed=4)
    kw = dict(permute=True, rotate="axis", scale=(0.8, 1.25), jitter=(0.01, 0.05))

    def make():
        return DeviceDataset(src, num_points=64, batch_size=8, device=DEV, transform=BatchAugment(21, device=DEV, **kw))
    straight = [b.clone() for b in make()]
    assert len(straight) == 5
    first = make()
    it = iter(first)
    head = [next(it).clone(), next(it).clone()]
    state = first.get_state()
    assert state["batch"] == 2 and state["epoch"] == 0 and state["transform"] == {"seed": 21, "step": 2}
    resumed = make()
    resumed.set_state(state)
    tail = [b.clone() for b in resumed]
    assert len(tail) == 3 and resumed.epoch == 1 and resumed.batch == 0
    for got, want in zip(head + tail, straight):
        assert torch.equal(got, want)
    # the next epoch comes in another order, and every cloud is used once per epoch
    nxt = [b.clone() for b in resumed]
    assert len(nxt) == 5 and not torch.equal(nxt[0], straight[0])


def test_limits_raise_value_error():
    from spgan import _lib
    from spgan.augment import MAX_POINTS, BatchAugment
    assert _lib.load().spgan_augment_max_points() == MAX_POINTS == 8192
    aug = BatchAugment(1, permute=True, device=DEV)
    data = torch.zeros((1, MAX_POINTS + 8, 3), device=DEV)
    index = torch.zeros((1,), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        aug(data, index, n=0)
    with pytest.raises(ValueError, match="8192"):
        aug(data, index, n=MAX_POINTS + 1)
    with pytest.raises(ValueError):
        aug(torch.zeros((1, 16, 4), device=DEV), index)
    with pytest.raises(ValueError, match="GPU"):
        aug(torch.zeros((1, 16, 3)), index.cpu())
    # the C entry refuses the same sizes before any launch
    lib, cfg = _lib.load(), _lib.AugmentCfg()
    step = torch.zeros((1,), dtype=torch.int64, device=DEV)
    out, rec = torch.empty((MAX_POINTS + 8, 3), device=DEV), torch.empty((16,), device=DEV)
    args = lambda P, C, N: (data.data_ptr(), 1, P, C, index.data_ptr(), 1, N, 0, cfg, 1, step.data_ptr(), 0, None, None, None,   # noqa: E731
                            out.data_ptr(), rec.data_ptr(), None)
    assert lib.spgan_augment_batch(*args(MAX_POINTS + 8, 3, MAX_POINTS + 1)) == -22
    assert lib.spgan_augment_batch(*args(16, 3, 0)) == -22 and lib.spgan_augment_batch(*args(16, 4, 8)) == -22
    assert aug.get_state()["step"] == 0


def test_reference_named_wrappers():
    """Thin wrappers: a new tensor comes back, the argument stays, and each equals the BatchAugment configuration it stands for."""
    from spgan import augment as A
    pc = torch.from_numpy(_data(3, 96, 3, seed=12)).to(DEV)
    keep = pc.clone()
    A.manual_seed(5)
    got = A.augment_batch_data(pc)
    want = A.BatchAugment(5, permute=True, rotate="axis", perturb=(0.06, 0.18), scale=(0.8, 1.25), translate=0.1, jitter=(0.01, 0.05),
                          device=DEV).transform(pc)[0]
    assert torch.equal(got, want) and torch.equal(pc, keep) and got.data_ptr() != pc.data_ptr()
    assert A.default_generator.step == 1
    for fn in (A.rotate_point_cloud, A.rotate_point_cloud_z, A.rotate_perturbation_point_cloud, A.jitter_point_cloud, A.shift_point_cloud,
               A.random_scale_point_cloud, A.random_point_dropout, A.shuffle_points):
        assert fn(pc).shape == pc.shape
    for cls in (A.PointcloudRotate_batch, A.PointcloudRotatePerturbation_batch, A.PointcloudScale_batch, A.PointcloudTranslate_batch,
                A.PointcloudScaleAndTranslate, A.PointcloudJitter_batch, A.PointcloudRandomInputDropout_batch):
        one, two = cls(seed=3)(pc), cls(seed=3)(pc)
        assert torch.equal(one, two) and not torch.equal(one, pc)
    rot = A.PointcloudRotatebyAngle()(pc, 0.7).cpu().numpy()
    want = np.stack([am.apply_map(c, *am.compose(rot=am.rot_euler(0.0, 0.7, 0.0))) for c in keep.cpu().numpy()])
    assert np.abs(rot - want).max() <= 1e-6 and torch.equal(pc, keep)
