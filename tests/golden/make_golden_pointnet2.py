#!/usr/bin/env python
"""Generate tests/golden/g22_pointnet2.npz by running the REAL reference modules of Common/pointnet_util.py:146-320 on the CPU
(PointNetSetAbstraction, its group_all form, PointNetSetAbstractionMsg, PointNetFeaturePropagation with coincident points and with
S == 1), each in float32 and again in float64 (`name|full` / `name|f64|full`).  Nothing of the reference is copied: its module is
imported and run.  The float64 pass reuses the float32 pass's FPS and ball-query indices (patched into the imported module), so that
the two differ by rounding alone.

Conditions asserted before anything is written (a seed that fails one is skipped, the conditions stay):
  * every point's 3rd and 4th nearest centre differ by a float64 relative gap >= 1e-4 and no two of its three nearest tie exactly;
  * every ball query finds at least one and, for at least a quarter of the centres, fewer than nsample neighbours;
  * no float32 reference distance of the propagation case equals exactly -1e-8 (finite weights).

    python tests/golden/make_golden_pointnet2.py          (SPGAN_REFERENCE = the reference checkout, default /root/reference)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SPGAN_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
torch.set_num_threads(8)

from Common import pointnet_util as R          # noqa: E402  (the reference)

B, N, S, K, D = 2, 256, 64, 16, 6      # (small: the whole fixture stays under 1 MiB)
OUT = {}


def put(name, t, f64=False):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.dtype == np.float64 and not f64:
        a = a.astype(np.float32)
    OUT[name + ("|f64" if f64 else "") + "|full"] = a


def inputs(seed, n=N, d=D):
    rng = np.random.default_rng(seed)
    xyz = rng.random((B, 3, n), dtype=np.float64).astype(np.float32)
    pts = rng.standard_normal((B, d, n)).astype(np.float32)
    return torch.from_numpy(xyz), torch.from_numpy(pts)


class Recorder:
    """Wraps the reference's index-producing functions: records their float32 results, replays them in the float64 pass."""

    def __init__(self):
        self.fps, self.ball, self.replay = [], [], False
        self._fps, self._ball = R.farthest_point_sample, R.query_ball_point

    def __enter__(self):
        def fps(xyz, npoint):
            if self.replay:
                return self.fps.pop(0)
            r = self._fps(xyz, npoint); self.fps.append(r); return r

        def ball(radius, nsample, xyz, new_xyz):
            if self.replay:
                return self.ball.pop(0)
            r = self._ball(radius, nsample, xyz, new_xyz); self.ball.append(r); return r
        R.farthest_point_sample, R.query_ball_point = fps, ball
        return self

    def __exit__(self, *exc):
        R.farthest_point_sample, R.query_ball_point = self._fps, self._ball


def run_case(tag, make, args32, seed, n_out, check_balls=None, store_inputs=True):
    """make() -> module; args32: dict name -> float32 tensor | None (forward order).  Gradients for loss = sum_i <out_i, gout_i>."""
    torch.manual_seed(seed)
    mod = make()
    sd0 = {k: v.clone() for k, v in mod.state_dict().items()}
    for k, v in sd0.items():
        OUT["%s|sd|%s" % (tag, k)] = v.numpy()
    torch.manual_seed(seed + 1000)
    n_pts = next(v for v in args32.values() if v is not None).shape[2]
    start = torch.randint(0, n_pts, (B,), dtype=torch.long)                 # the draw farthest_point_sample makes first (:75)
    OUT["%s|start" % tag] = start.numpy()
    gouts = None
    with Recorder() as rec:
        for f64 in (False, True):
            dt = torch.float64 if f64 else torch.float32
            torch.set_default_dtype(dt)
            m = make().to(dt)
            m.load_state_dict({k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd0.items()})
            m.train()
            xs = {k: (None if v is None else v.to(dt).clone().requires_grad_(not k.startswith("xyz_nograd"))) for k, v in args32.items()}
            torch.manual_seed(seed + 1000)
            rec.replay = f64
            outs = m(*xs.values())
            outs = outs if isinstance(outs, tuple) else (outs,)
            assert len(outs) == n_out
            if gouts is None:
                rng = np.random.default_rng(seed + 77)
                gouts = [torch.from_numpy(rng.standard_normal(tuple(o.shape)).astype(np.float16).astype(np.float32)) for o in outs]   # float16-exact: stored as float16
                for i, g in enumerate(gouts):
                    OUT["%s|gout%d" % (tag, i)] = g.numpy().astype(np.float16)
                if check_balls is not None:
                    check_balls(rec.ball)
                for i, r in enumerate(rec.fps):
                    OUT["%s|fps%d" % (tag, i)] = r.numpy().astype(np.int16)
                for i, r in enumerate(rec.ball):
                    OUT["%s|ball%d" % (tag, i)] = r.numpy().astype(np.int16)
            sum((o * g.to(dt)).sum() for o, g in zip(outs, gouts)).backward()
            for i, o in enumerate(outs):
                put("%s|out%d" % (tag, i), o, f64)
            for k, p in m.named_parameters():
                put("%s|grad|%s" % (tag, k), p.grad, f64)
            for k, v in xs.items():
                if v is not None and v.grad is not None:
                    put("%s|gin|%s" % (tag, k), v.grad, f64)
            for k, v in m.named_buffers():
                if v.is_floating_point():
                    put("%s|buf|%s" % (tag, k), v, f64)
                elif not f64:
                    OUT["%s|buf|%s" % (tag, k)] = v.numpy()
            torch.set_default_dtype(torch.float32)
    for k, v in args32.items():
        if v is not None and store_inputs:
            OUT["%s|in|%s" % (tag, k)] = v.numpy()


def balls_ok(nsample_list):
    def chk(balls):
        assert len(balls) == len(nsample_list)
        for idx, ns in zip(balls, nsample_list):
            assert int(idx.max()) < N, "a ball query found nothing"
            short = (idx[:, :, 1:] == idx[:, :, :1]).any(-1)          # padded with the first index: fewer than nsample neighbours
            assert short.float().mean().item() >= 0.25, short.float().mean().item()
    return chk


def nn_conditions(xyz1, xyz2):
    """xyz [B,n,3] float32.  -> (ok, float32 sorted distances, float32 sort indices)."""
    d64 = R.square_distance(xyz1.double(), xyz2.double()).sort(dim=-1)[0]
    if xyz2.shape[1] >= 4:
        gap = (d64[..., 3] - d64[..., 2]) / d64[..., 3].clamp_min(1e-300)
        if not bool((gap >= 1e-4).all()):
            return False, None, None
    if bool((d64[..., 1] == d64[..., 0]).any()) or bool((d64[..., 2] == d64[..., 1]).any()):
        return False, None, None
    d32, i32 = R.square_distance(xyz1, xyz2).sort(dim=-1)
    if bool((R.square_distance(xyz1, xyz2) == np.float32(-1e-8)).any()):
        return False, None, None
    # the float32 order of the three nearest must be the float64 one (else "indices equal" would not be well-defined)
    i64 = R.square_distance(xyz1.double(), xyz2.double()).sort(dim=-1)[1]
    if not torch.equal(i32[..., :3], i64[..., :3]):
        return False, None, None
    return True, d32, i32


def main():
    # ---- set abstraction, single scale / group_all / multi-scale
    xyz, pts = inputs(0)
    run_case("sa", lambda: R.PointNetSetAbstraction(S, 0.2, K, 3 + D, [32, 32, 64], False), {"xyz": xyz, "points": pts}, 11, 2, balls_ok([K]))
    xa, pa = inputs(1, n=160)
    run_case("sa_all", lambda: R.PointNetSetAbstraction(None, None, None, 3 + D, [32, 64], True), {"xyz": xa, "points": pa}, 12, 2)
    run_case("msg", lambda: R.PointNetSetAbstractionMsg(S, [0.12, 0.2], [8, K], D, [[16, 32], [32, 64]]), {"xyz": xyz, "points": pts}, 13, 2,
             balls_ok([8, K]), store_inputs=False)            # (the inputs of "sa")
    # ---- feature propagation: xyz2 = an FPS subset of xyz1 (coincident points), then S == 1
    for seed in range(0, 64):
        x1, p1 = inputs(seed)
        torch.manual_seed(seed)
        fps = R.farthest_point_sample(x1.permute(0, 2, 1), S)
        x2 = R.index_points(x1.permute(0, 2, 1), fps).permute(0, 2, 1).contiguous()
        ok, d32, i32 = nn_conditions(x1.permute(0, 2, 1).contiguous(), x2.permute(0, 2, 1).contiguous())
        if ok:
            break
    else:
        raise SystemExit("no seed met the three_nn conditions")
    print("feature propagation: seed %d meets the nearest-centre conditions" % seed)
    OUT["fp|seed"] = np.int64(seed)
    OUT["fp|nn_idx"] = i32[..., :3].numpy().astype(np.int16)
    OUT["fp|nn_dist4"] = d32[..., :4].numpy()
    rng = np.random.default_rng(500 + seed)
    p2 = torch.from_numpy(rng.standard_normal((B, 16, S)).astype(np.float32))
    run_case("fp", lambda: R.PointNetFeaturePropagation(D + 16, [32, 16]), {"xyz_nograd1": x1, "xyz_nograd2": x2, "points1": p1, "points2": p2}, 14, 1)
    p21 = torch.from_numpy(rng.standard_normal((B, 16, 1)).astype(np.float32))
    run_case("fp1", lambda: R.PointNetFeaturePropagation(D + 16, [16]), {"xyz_nograd1": x1, "xyz_nograd2": x2[:, :, :1].contiguous(), "points1": p1,
                                                                          "points2": p21}, 15, 1)
    path = os.path.join(HERE, "g22_pointnet2.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s: %d entries, %.2f MB" % (path, len(OUT), os.path.getsize(path) / 1e6))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
