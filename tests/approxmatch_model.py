"""numpy model of the approxmatch earth mover's distance (spgan.approxmatch, csrc/approxmatch.hip): the definition of include/spgan_hip.h
written densely, one pair at a time, in float64 or (dtype=np.float32) with every elementwise result rounded to float32.

    approx_match(xyz1 [n,3], xyz2 [m,3], dtype) -> dict(match [n,m], ratioL [10,n], ratioR [10,m], remainL [n], remainR [m], cost,
                                                        grad1 [n,3], grad2 [m,3], multiL, multiR, dmax)
    batch(xyz1 [B,n,3], xyz2 [B,m,3], dtype)    -> the same, stacked; match in the kernels' layout [B,m,n]

The gradients are those of sum match * |xyz1 - xyz2| with match held constant (as in the original extensions).  clouds() builds the
test clouds of tests/test_approxmatch_gpu.py and tools/approxmatch_accuracy.py.
"""
import numpy as np

LEVELS = tuple(range(7, -3, -1))          # j = 7 .. -2


def level(j):
    return 0.0 if j == -2 else -(4.0 ** j)


def check_shapes(n, m):
    if n < 1 or m < 1 or max(n, m) % min(n, m) != 0:
        raise ValueError("the larger point count must be a multiple of the smaller, got n = %d, m = %d" % (n, m))


def approx_match(xyz1, xyz2, dtype=np.float64):
    a, b = np.asarray(xyz1, dtype=dtype), np.asarray(xyz2, dtype=dtype)
    n, m = a.shape[0], b.shape[0]
    check_shapes(n, m)
    one, eps = dtype(1), dtype(1e-9)
    diff = a[:, None, :] - b[None, :, :]
    d2 = (diff * diff).sum(-1, dtype=dtype)
    dist = np.sqrt(d2)
    multi_l, multi_r = dtype(max(n, m)) / dtype(n), dtype(max(n, m)) / dtype(m)
    remain_l, remain_r = np.full(n, multi_l, dtype=dtype), np.full(m, multi_r, dtype=dtype)
    match = np.zeros((n, m), dtype=dtype)
    rl, rr = np.zeros((len(LEVELS), n), dtype=dtype), np.zeros((len(LEVELS), m), dtype=dtype)
    with np.errstate(under="ignore"):
        for i, j in enumerate(LEVELS):
            e = np.exp(dtype(level(j)) * d2)
            ratio_l = remain_l / (eps + (e * remain_r[None, :]).sum(1, dtype=dtype))
            sumr = remain_r * (e * ratio_l[:, None]).sum(0, dtype=dtype)
            ratio_r = np.minimum(remain_r / (sumr + eps), one) * remain_r
            remain_r = np.maximum(dtype(0), remain_r - sumr)
            w = e * ratio_l[:, None] * ratio_r[None, :]
            match += w
            remain_l = np.maximum(dtype(0), remain_l - w.sum(1, dtype=dtype))
            rl[i], rr[i] = ratio_l, ratio_r
        cost = (match * dist).sum(dtype=dtype)
        unit = diff / np.maximum(dist, dtype(1e-20))[:, :, None]
        grad1 = (match[:, :, None] * unit).sum(1, dtype=dtype)
        grad2 = -(match[:, :, None] * unit).sum(0, dtype=dtype)
    return dict(match=match, ratioL=rl, ratioR=rr, remainL=remain_l, remainR=remain_r, cost=cost, grad1=grad1, grad2=grad2,
                multiL=float(multi_l), multiR=float(multi_r), dmax=float(dist.max()), d2=d2)


def plan_from_records(d2, rl, rr):
    """match [n,m] = sum_j E_j * ratioL_j[k] * ratioR_j[l]: what the fused backward and the dense-plan writer recompute."""
    dtype = d2.dtype.type
    with np.errstate(under="ignore"):
        return sum(np.exp(dtype(level(j)) * d2) * rl[i][:, None] * rr[i][None, :] for i, j in enumerate(LEVELS))


def grads_from_plan(xyz1, xyz2, match):
    a, b = np.asarray(xyz1, dtype=np.float64), np.asarray(xyz2, dtype=np.float64)
    diff = a[:, None, :] - b[None, :, :]
    dist = np.sqrt((diff * diff).sum(-1))
    unit = diff / np.maximum(dist, 1e-20)[:, :, None]
    return (match[:, :, None] * unit).sum(1), -(match[:, :, None] * unit).sum(0), float((match * dist).sum())


def batch(xyz1, xyz2, dtype=np.float64):
    rs = [approx_match(a, b, dtype) for a, b in zip(xyz1, xyz2)]
    out = {k: np.stack([np.asarray(r[k]) for r in rs]) for k in ("ratioL", "ratioR", "cost", "grad1", "grad2", "remainL", "remainR")}
    out["match"] = np.stack([r["match"].T for r in rs])                    # [B,m,n]
    out["multiL"], out["multiR"] = rs[0]["multiL"], rs[0]["multiR"]
    out["dmax"] = max(r["dmax"] for r in rs)
    return out


KINDS = ("cube", "sphere", "identical", "duplicates", "far", "scaled")


def clouds(kind, B, n, m, seed=0):
    """float32 (xyz1 [B,n,3], xyz2 [B,m,3]):
      cube        uniform in the unit cube              sphere      uniform on the unit sphere
      identical   xyz2 repeats / subsamples xyz1        duplicates  cube clouds in which every fourth point repeats its predecessor, and
      far         two cube clouds 10 units apart                    xyz2 shares xyz1's first points (d = 0 between and within the clouds)
      scaled      cube coordinates times 100"""
    g = np.random.default_rng(1000003 * seed + 7919 * n + 31 * m + B + 17 * KINDS.index(kind))
    a, b = g.random((B, n, 3)), g.random((B, m, 3))
    if kind == "sphere":
        a, b = g.standard_normal((B, n, 3)), g.standard_normal((B, m, 3))
        a, b = a / np.linalg.norm(a, axis=-1, keepdims=True), b / np.linalg.norm(b, axis=-1, keepdims=True)
    elif kind == "identical":
        b = np.stack([a[i][np.arange(m) % n] for i in range(B)])
    elif kind == "duplicates":
        a[:, 3::4] = a[:, 2::4][:, :a[:, 3::4].shape[1]]
        b[:, 3::4] = b[:, 2::4][:, :b[:, 3::4].shape[1]]
        s = min(n, m) // 2
        b[:, :s] = a[:, :s]
    elif kind == "far":
        b = b + np.array([10.0, 0.0, 0.0])
    elif kind == "scaled":
        a, b = a * 100.0, b * 100.0
    return a.astype(np.float32), b.astype(np.float32)
