#!/usr/bin/env python3
"""Generate tests/golden/g23_local_cd.npz (G23): the reference's local-shape Chamfer and GAN_metrics drivers on small inputs.
Runs only in the build container (it reads the read-only reference checkout); the tests read the .npz.

    python tests/golden/make_golden_local_cd.py

The real reference functions are compiled with `ast` (the modules import CUDA extensions and `evaluation.pointnet`, which do not
load here): get_local_pair, compute_mean_covariance and ChamferLoss from Common/loss_utils.py; local_CD, pairwise_local_CD,
pairwise_dists, pairwise_simple, pairwise_CD, COV, MMD, KNN, JSD, get_voxel_occ_dist, compute_all_metrics and
compute_all_metrics_train from Common/GAN_metrics.py (scipy.stats.entropy as there).  Two CUDA pieces are restated on the CPU:

  * pointops_util.Gen_QueryAndGroupXYZ(radius=None, nsample=K): knnquery (metrics/pointops/src/knnquery/knnquery_cuda_kernel.cu)
    then grouping.  The squared distances are ((dx*dx + dy*dy) + dz*dz) in the input's precision, the K smallest are taken by a
    stable sort (ascending, lower index first on ties, as the kernel's strict < insertion), and the grouped coordinates are a
    differentiable gather [B,3,M,K] of xyz.
  * distChamferCUDA (ChamferDistance.forward): both directions of the nearest squared distance, exact differences.

Every function runs in float32 (the reference's precision) and again in float64 from the same inputs, and the gradients of
get_local_pair's two terms w.r.t. both clouds are recorded from float32 autograd.  The lattice block holds knnquery's indices on
a 4x4x4 lattice plus duplicated points, where many distances tie exactly.
"""
import ast
import os

import numpy as np
import scipy.stats
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


class _QueryAndGroupXYZ(nn.Module):
    def __init__(self, radius=None, nsample=32, use_xyz=True):
        super().__init__()
        assert radius is None
        self.nsample = nsample

    def forward(self, xyz, new_xyz=None):
        new_xyz = xyz if new_xyz is None else new_xyz
        q, c = new_xyz.detach()[:, :, None, :], xyz.detach()[:, None, :, :]
        dx, dy, dz = q[..., 0] - c[..., 0], q[..., 1] - c[..., 1], q[..., 2] - c[..., 2]
        d = (dx * dx + dy * dy) + dz * dz
        idx = torch.from_numpy(np.argsort(d.numpy(), axis=-1, kind="stable")[..., :self.nsample].copy())
        B = xyz.shape[0]
        g = xyz[torch.arange(B)[:, None, None], idx]              # [B,M,K,3]
        return g.permute(0, 3, 1, 2)                              # [B,3,M,K]


class _PointopsUtil:
    Gen_QueryAndGroupXYZ = _QueryAndGroupXYZ


def _distChamferCUDA(x, y):
    d = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    return d.min(2)[0], d.min(1)[0]


def _compile(path, funcs, classes=()):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name in funcs) or (isinstance(n, ast.ClassDef) and n.name in classes)]
    mod = ast.Module(body=body, type_ignores=[])
    ns = {"torch": torch, "np": np, "nn": nn, "entropy": scipy.stats.entropy, "pointops_util": _PointopsUtil,
          "distChamferCUDA": _distChamferCUDA}
    exec(compile(mod, path, "exec"), ns)
    return ns


LU = _compile(os.path.join(REF, "Common/loss_utils.py"), {"get_local_pair", "compute_mean_covariance"}, {"ChamferLoss"})
GM = _compile(os.path.join(REF, "Common/GAN_metrics.py"),
              {"local_CD", "pairwise_local_CD", "pairwise_dists", "pairwise_simple", "pairwise_CD", "COV", "MMD", "KNN", "JSD",
               "get_voxel_occ_dist", "compute_all_metrics", "compute_all_metrics_train", "compute_mean_covariance"}, {"ChamferLoss"})


def cloud(g, shape, scale=0.2):
    return (torch.randn(shape, generator=g) * scale).clamp(-0.49, 0.49)


def main():
    g = torch.Generator().manual_seed(23)
    out = {}
    # get_local_pair: pt1 [B,3,M], pt2 [B,3,N]
    p1 = cloud(g, (3, 3, 256))
    p2 = (p1[:, :, :] + 0.03 * torch.randn((3, 3, 256), generator=g)).clone()
    p2 = torch.cat([p2, cloud(g, (3, 3, 64))], dim=2)                     # N = 320 > M
    out["glp_pt1"], out["glp_pt2"] = p1.numpy(), p2.numpy()
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        a, b = p1.to(dt).requires_grad_(True), p2.to(dt).requires_grad_(True)
        m, v = LU["get_local_pair"](a, b)
        out["glp_mu_" + tag], out["glp_var_" + tag] = m.item(), v.item()
        if tag == "32":
            ga1, ga2 = torch.autograd.grad(m, (a, b), retain_graph=True)
            gb1, gb2 = torch.autograd.grad(v, (a, b))
            out.update(glp_gmu_pt1=ga1.numpy(), glp_gmu_pt2=ga2.numpy(), glp_gvar_pt1=gb1.numpy(), glp_gvar_pt2=gb2.numpy())
    # ChamferLoss in 3-D and 9-D
    x3, y3 = torch.randn((2, 200, 3), generator=g), torch.randn((2, 150, 3), generator=g)
    x9, y9 = torch.randn((2, 120, 9), generator=g) * 0.1, torch.randn((2, 100, 9), generator=g) * 0.1
    out.update(cl_x3=x3.numpy(), cl_y3=y3.numpy(), cl_x9=x9.numpy(), cl_y9=y9.numpy())
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        out["cl3_" + tag] = GM["ChamferLoss"]()(x3.to(dt), y3.to(dt)).item()
        out["cl9_" + tag] = GM["ChamferLoss"]()(x9.to(dt), y9.to(dt)).item()
    # local_CD on [B,N,3]
    l1 = cloud(g, (2, 256, 3))
    l2 = l1 + 0.02 * torch.randn((2, 256, 3), generator=g)
    out.update(lcd_pt1=l1.numpy(), lcd_pt2=l2.numpy())
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        m, v = GM["local_CD"](l1.to(dt), l2.to(dt))
        out["lcd_mu_" + tag], out["lcd_var_" + tag] = m.item(), v.item()
    # pairwise and drivers: S = 8 samples, R = 10 references of 128 points; 16-D features for l2
    base = cloud(g, (1, 128, 3))
    sample = (base + 0.05 * torch.randn((8, 128, 3), generator=g)).clamp(-0.49, 0.49)
    ref = (base + 0.05 * torch.randn((10, 128, 3), generator=g)).clamp(-0.49, 0.49)
    fs, fr_ = torch.randn((8, 16), generator=g), torch.randn((10, 16), generator=g)
    out.update(pw_sample=sample.numpy(), pw_ref=ref.numpy(), pw_fs=fs.numpy(), pw_fr=fr_.numpy())
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        s_, r_ = sample.to(dt), ref.to(dt)
        for dist in ("CD_M", "CD_C"):
            out["plcd_%s_bs1_%s" % (dist, tag)] = GM["pairwise_local_CD"](s_, r_, 1, dist).numpy()
            out["plcd_%s_bs4_%s" % (dist, tag)] = GM["pairwise_local_CD"](s_, r_, 4, dist).numpy()
        for dist in ("CD", "CD_M", "CD_C"):
            res = GM["compute_all_metrics"](s_, r_, 1, dist)
            for k, val in res.items():
                out["cam_%s_%s_%s" % (dist, k, tag)] = float(val)
            res = GM["compute_all_metrics_train"](s_, r_, None, 1, dist, False)
            for k, val in res.items():
                out["camt_%s_%s_%s" % (dist, k, tag)] = float(val)
            sr = GM["pairwise_dists"](s_, r_, 1, dist)
            out["pd_%s_sr_%s" % (dist, tag)] = sr.numpy()
        res = GM["compute_all_metrics_train"](fs.to(dt), fr_.to(dt), None, 4, "l2", False)
        for k, val in res.items():
            out["camt_l2_%s_%s" % (k, tag)] = float(val)
        out["pd_l2_sr_" + tag] = GM["pairwise_dists"](fs.to(dt), fr_.to(dt), 4, "l2").numpy()
        out["ps_l1_sr_" + tag] = GM["pairwise_simple"](fs.to(dt), fr_.to(dt), 4, "l1").numpy()
    # JSD on clouds that partly leave the cube
    j1, j2 = torch.randn((6, 300, 3), generator=g) * 0.25, torch.randn((5, 300, 3), generator=g) * 0.2
    out.update(jsd_c1=j1.numpy(), jsd_c2=j2.numpy(), jsd=GM["JSD"](j1.numpy(), j2.numpy(), warning=False),
               voxel_c1=(GM["get_voxel_occ_dist"](j1.numpy(), warning=False)))
    # KNN: random blocks, and a constructed 3-3 tie at k = 6 (sample 0's six nearest others: 3 samples, 3 references)
    Mxx, Mxy, Myy = torch.rand((5, 5), generator=g), torch.rand((5, 4), generator=g), torch.rand((4, 4), generator=g)
    Mxx, Myy = (Mxx + Mxx.t()) / 2, (Myy + Myy.t()) / 2
    out.update(knn_xx=Mxx.numpy(), knn_xy=Mxy.numpy(), knn_yy=Myy.numpy())
    for k in (1, 3, 6):
        out["knn_k%d" % k] = GM["KNN"](Mxx, Mxy, Myy, k)
        out["knn_sqrt_k%d" % k] = GM["KNN"](Mxx - 0.5, Mxy, Myy, k, sqrt=True)
    tx = torch.full((4, 4), 9.0)
    ty = torch.full((3, 3), 9.0)
    txy = torch.full((4, 3), 9.0)
    tx[0, 1:4] = tx[1:4, 0] = torch.tensor([0.1, 0.2, 0.3])
    txy[0, :] = torch.tensor([0.15, 0.25, 0.35])
    out.update(tie_xx=tx.numpy(), tie_xy=txy.numpy(), tie_yy=ty.numpy(), tie_k6=GM["KNN"](tx, txy, ty, 6))
    # lattice with exact ties, plus duplicated points: knnquery indices for K = 8, 20, 32
    ax = torch.arange(4, dtype=torch.float32) * 0.125 - 0.1875
    lat = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, 64, 3)
    lat = torch.cat([lat, lat[:, :8]], dim=1)                            # 72 points, the first 8 twice
    out["lat"] = lat.numpy()
    for K in (8, 20, 32):
        gx = _QueryAndGroupXYZ(None, K)(lat, lat)                        # [1,3,72,K]
        q, c = lat[:, :, None, :], lat[:, None, :, :]
        d = ((q[..., 0] - c[..., 0]) ** 2 + (q[..., 1] - c[..., 1]) ** 2) + (q[..., 2] - c[..., 2]) ** 2
        out["lat_idx_k%d" % K] = np.argsort(d.numpy(), axis=-1, kind="stable")[..., :K].astype(np.int64)
        out["lat_grouped_k%d" % K] = gx.numpy()
    path = os.path.join(HERE, "g23_local_cd.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
