"""numpy model of the device-side batch augmentation, written from the description in include/spgan_hip.h ("Device-side batch
augmentation") alone: Philox4x32-10 in uint64 arithmetic, the draw assignment, the permutation as an argsort of the 64-bit keys, the
parameters and their application.  Every function takes `dt`: np.float64 is the reference, np.float32 evaluates the same formulas in
single precision (the e_ref of the tolerance rule max(4 e_ref, 8 * 2^-24 * scale))."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
TWO_PI_F = np.float32(6.2831853)          # the constant of the header, a float32
CFG_DEFAULT = dict(permute=0, rotate=0, axis=(0.0, 1.0, 0.0), transpose=0, perturb=0, perturb_sigma=0.06, perturb_clip=0.18,
                   scale=0, scale_lo=0.8, scale_hi=1.25, translate=0, translate_range=0.1, jitter=0, jitter_sigma=0.01, jitter_clip=0.05,
                   dropout=0, dropout_max=0.875)


def make_cfg(**kw):
    c = dict(CFG_DEFAULT)
    for k in kw:
        assert k in c, k
    c.update(kw)
    return c


# ------------------------------------------------------------------------------------------ Philox4x32-10
def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (broadcastable), integers below 2^32 -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0               # < 2^64: both factors are below 2^32
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def block(seed, purpose, b, step, e):
    """X(purpose, b, e): uint32 [len(e), 4] (or [4] for a scalar e)."""
    e = np.asarray(e, dtype=np.uint64)
    ctr = np.stack([e, np.full_like(e, (int(purpose) << 24) | int(b)), np.full_like(e, int(step) & 0xFFFFFFFF),
                    np.full_like(e, int(step) >> 32)], axis=-1)
    return philox4x32_10(ctr, np.array([int(seed) & 0xFFFFFFFF, int(seed) >> 32], dtype=np.uint64))


def words(seed, purpose, b, step, n):
    """The first n words of the stream of (purpose, b)."""
    return block(seed, purpose, b, step, np.arange((n + 3) // 4)).reshape(-1)[:n]


def uni(x, dt=np.float64):
    return (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(dt) * dt(2.0 ** -24)


def normal2(xa, xb, dt=np.float64):
    u1 = ((np.asarray(xa, dtype=np.uint32) >> np.uint32(8)).astype(np.uint64) + np.uint64(1)).astype(dt) * dt(2.0 ** -24)
    r = np.sqrt(dt(-2.0) * np.log(u1))
    th = dt(TWO_PI_F) * uni(xb, dt)
    return r * np.cos(th), r * np.sin(th)


# ------------------------------------------------------------------------------------------ matrices
def rot_euler(ax, ay, az, dt=np.float64):
    """Rz Ry Rx (provider.py's matrices)."""
    ax, ay, az = dt(ax), dt(ay), dt(az)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]], dtype=dt)
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]], dtype=dt)
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]], dtype=dt)
    return (rz @ (ry @ rx)).astype(dt)


def rot_axis(a, axis, dt=np.float64):
    """data_utils.angle_axis for a unit axis."""
    a = dt(a)
    u = np.asarray(axis, dtype=dt)
    cross = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]], dtype=dt)
    return (np.cos(a) * np.eye(3, dtype=dt) + np.sin(a) * cross + (dt(1) - np.cos(a)) * np.outer(u, u)).astype(dt)


def compose(rot=None, perturb=None, scale=None, translate=None, transpose=0, dt=np.float64):
    """(A, t) of stages 3-6 in row-vector convention: xyz' = xyz A + t.  rot / perturb: rotation matrices R (applied as xyz @ R, or
    xyz @ R.T with transpose); scale: scalar or [3]; translate: scalar or [3]."""
    A = np.eye(3, dtype=dt)
    for R in (rot, perturb):
        if R is not None:
            R = np.asarray(R, dtype=dt)
            A = (A @ (R.T if transpose else R)).astype(dt)
    if scale is not None:
        A = (A * np.broadcast_to(np.asarray(scale, dtype=dt), (3,))[None, :]).astype(dt)
    t = np.zeros(3, dtype=dt) if translate is None else np.broadcast_to(np.asarray(translate, dtype=dt), (3,)).copy()
    return A, t


def unit_axis(axis):
    a = np.asarray(axis, dtype=np.float64)
    return (a / np.linalg.norm(a)).astype(np.float32)


def cloud_params(cfg, seed, step, b, dt=np.float64):
    """-> (A [3,3], t [3], ratio float32) of cloud b."""
    f = lambda v: dt(np.float32(v))                                        # noqa: E731  the configuration reaches the kernel as float32
    d0 = block(seed, 0, b, step, 0)
    rot = per = sc = tr = None
    if cfg["rotate"] == 1:
        rot = rot_axis(dt(TWO_PI_F) * uni(d0[0], dt), unit_axis(cfg["axis"]).astype(dt), dt)
    elif cfg["rotate"] == 2:
        rot = rot_euler(*(dt(TWO_PI_F) * uni(d0[i], dt) for i in range(3)), dt=dt)
    if cfg["perturb"]:
        d1 = block(seed, 0, b, step, 1)
        g0, g1 = normal2(d1[0], d1[1], dt)
        g2, _ = normal2(d1[2], d1[3], dt)
        s, c = f(cfg["perturb_sigma"]), f(cfg["perturb_clip"])
        per = rot_euler(*(np.clip(s * g, -c, c) for g in (g0, g1, g2)), dt=dt)
    if cfg["scale"]:
        d2 = block(seed, 0, b, step, 2)
        lo, hi = f(cfg["scale_lo"]), f(cfg["scale_hi"])
        sc = np.array([lo + (hi - lo) * uni(d2[i if cfg["scale"] == 2 else 0], dt) for i in range(3)], dtype=dt)
    if cfg["translate"]:
        d3 = block(seed, 0, b, step, 3)
        r = f(cfg["translate_range"])
        tr = np.array([(dt(2) * uni(d3[i if cfg["translate"] == 1 else 0], dt) - dt(1)) * r for i in range(3)], dtype=dt)
    A, t = compose(rot, per, sc, tr, cfg["transpose"], dt)
    ratio = np.float32(uni(d0[3], np.float32) * np.float32(cfg["dropout_max"])) if cfg["dropout"] else np.float32(0)
    return A, t, ratio


def permutation(seed, step, b, n, keys=None):
    """Point indices in ascending order of (draw << 32) | index."""
    d = words(seed, 1, b, step, n) if keys is None else np.asarray(keys, dtype=np.uint32)
    k = (d.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    return np.argsort(k, kind="stable")


def normal_map(A, dt=np.float64):
    A = np.asarray(A, dtype=dt)
    return (A / np.sqrt((A * A).sum(axis=0, keepdims=True))).astype(dt)


def apply_map(pts, A, t, dt=np.float64):
    """pts [N, 3 or 6] -> xyz A + t; normals by the column-normalised A."""
    p = np.asarray(pts, dtype=dt)
    out = p.copy()
    out[:, :3] = p[:, :3] @ np.asarray(A, dtype=dt) + np.asarray(t, dtype=dt)
    if p.shape[1] == 6:
        out[:, 3:] = p[:, 3:] @ normal_map(A, dt)
    return out.astype(dt)


def clip_noise(g, sigma, clip, dt=np.float64):
    """clip(sigma * g, -clip, clip) of standard normal draws g."""
    return np.clip(dt(sigma) * np.asarray(g, dtype=dt), -dt(clip), dt(clip)).astype(dt)


def jitter_noise(cfg, seed, step, b, n, dt=np.float64):
    d = block(seed, 2, b, step, np.arange(n))
    j0, j1 = normal2(d[:, 0], d[:, 1], dt)
    j2, _ = normal2(d[:, 2], d[:, 3], dt)
    return clip_noise(np.stack([j0, j1, j2], axis=1), np.float32(cfg["jitter_sigma"]), np.float32(cfg["jitter_clip"]), dt)


def dropout_mask(seed, step, b, n, ratio):
    return uni(words(seed, 3, b, step, n), np.float32) <= np.float32(ratio)


def drop_rows(pts, mask):
    """Every masked row takes row 0 (all channels)."""
    out = np.array(pts, copy=True)
    out[np.asarray(mask, dtype=bool)] = out[0]
    return out


def run(data, index, n, cfg, seed, step, keys=None, params=None, dt=np.float64):
    """-> dict(out [B,n,C], A [B,3,3], t [B,3], ratio [B] float32, mask [B,n] bool, perm [B,n])."""
    data = np.asarray(data)
    B = len(index)
    C = data.shape[2]
    out = np.zeros((B, n, C), dtype=dt)
    As, ts, ratios, masks, perms = [], [], [], [], []
    affine = params is not None or cfg["rotate"] or cfg["perturb"] or cfg["scale"] or cfg["translate"]
    for b in range(B):
        pts = data[index[b]][:n].astype(dt)
        perm = permutation(seed, step, b, n, None if keys is None else keys[b]) if cfg["permute"] else np.arange(n)
        pts = pts[perm]
        A, t, ratio = cloud_params(cfg, seed, step, b, dt)
        if params is not None:
            A, t = np.asarray(params[b][:9], dtype=dt).reshape(3, 3), np.asarray(params[b][9:12], dtype=dt)
        if affine:
            pts = apply_map(pts, A, t, dt)
        if cfg["jitter"]:
            pts[:, :3] = pts[:, :3] + jitter_noise(cfg, seed, step, b, n, dt)
        mask = dropout_mask(seed, step, b, n, ratio) if cfg["dropout"] else np.zeros(n, dtype=bool)
        out[b] = drop_rows(pts, mask)
        As.append(A); ts.append(t); ratios.append(ratio); masks.append(mask); perms.append(perm)
    return dict(out=out, A=np.stack(As), t=np.stack(ts), ratio=np.array(ratios, dtype=np.float32), mask=np.stack(masks), perm=np.stack(perms))
