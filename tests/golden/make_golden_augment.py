#!/usr/bin/env python3
"""Generate tests/golden/augment_ref.npz by running the REAL reference augmentations on B = 2 clouds of N = 16 points under a
seeded np.random, recording for every case its inputs, the random draws in call order and its outputs (data only).

    python tests/golden/make_golden_augment.py <path to the reference checkout>

Executed from the reference, never copied: the functions of Common/provider.py and Common/point_operation.py and the classes of
Common/data_utils.py named below.  Those modules do not import here (h5py, the CD/EMD extensions), so the definitions are compiled
straight from the reference files with `ast` and run with `.cuda()` patched to the identity, as make_golden.py does.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SPGAN_REFERENCE", "")
torch.Tensor.cuda = lambda self, *a, **k: self                        # reference hard-codes .cuda()

B, N = 2, 16
LOG = []


def _recording(fn):
    def wrapped(*a, **k):
        r = fn(*a, **k)
        LOG.append(np.asarray(r, dtype=np.float64).reshape(-1))
        return r
    return wrapped


def extract(path, names):
    """Compile the named top-level functions / classes of a reference file."""
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    ns = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    if not os.path.isdir(os.path.join(REF, "Common")):
        raise SystemExit("usage: make_golden_augment.py <reference checkout>")
    prov = extract(os.path.join(REF, "Common/provider.py"),
                   ["rotate_point_cloud", "rotate_point_cloud_z", "rotate_point_cloud_with_normal", "rotate_perturbation_point_cloud",
                    "rotate_perturbation_point_cloud_with_normal", "jitter_point_cloud", "shift_point_cloud", "random_scale_point_cloud",
                    "random_point_dropout"])
    pop = extract(os.path.join(REF, "Common/point_operation.py"),
                  ["rotate_point_cloud_and_gt", "shift_point_cloud_and_gt", "random_scale_point_cloud_and_gt"])
    du = extract(os.path.join(REF, "Common/data_utils.py"),
                 ["angle_axis", "PointcloudRotate", "PointcloudRotatePerturbation", "PointcloudRotatePerturbation_batch", "PointcloudScaleAndTranslate",
                  "PointcloudTranslate", "PointcloudRandomInputDropout", "PointcloudRotatebyAngle"])

    rs = np.random.RandomState(20240607)
    xyz = rs.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    gt = rs.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    nrm = rs.normal(size=(B, N, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    xyzn = np.concatenate([xyz, nrm], axis=-1)
    out = {"xyz": xyz, "gt": gt, "xyzn": xyzn}

    np.random.seed(7)
    for name in ("uniform", "randn", "random"):
        setattr(np.random, name, _recording(getattr(np.random, name)))

    def case(tag, fn, *args):
        del LOG[:]
        res = fn(*[a.copy() if isinstance(a, np.ndarray) else (a.clone() if isinstance(a, torch.Tensor) else a) for a in args])
        res = res if isinstance(res, tuple) else (res,)
        out[tag + "|draws"] = np.concatenate(LOG) if LOG else np.zeros(0)
        for i, r in enumerate(res):
            out["%s|out%d" % (tag, i)] = r.detach().numpy() if isinstance(r, torch.Tensor) else np.asarray(r)

    T = torch.from_numpy
    case("provider.rotate_point_cloud", prov["rotate_point_cloud"], xyz)
    case("provider.rotate_point_cloud_z", prov["rotate_point_cloud_z"], xyz)
    case("provider.rotate_point_cloud_with_normal", prov["rotate_point_cloud_with_normal"], xyzn)
    case("provider.rotate_perturbation_point_cloud", prov["rotate_perturbation_point_cloud"], xyz)
    case("provider.rotate_perturbation_point_cloud_with_normal", prov["rotate_perturbation_point_cloud_with_normal"], xyzn)
    case("provider.jitter_point_cloud", prov["jitter_point_cloud"], xyz)
    case("provider.shift_point_cloud", prov["shift_point_cloud"], xyz)
    case("provider.random_scale_point_cloud", prov["random_scale_point_cloud"], xyz)
    case("provider.random_point_dropout", prov["random_point_dropout"], xyz)
    case("point_operation.rotate_point_cloud_and_gt.y", pop["rotate_point_cloud_and_gt"], xyz[0], gt[0], True)
    case("point_operation.rotate_point_cloud_and_gt.xyz", pop["rotate_point_cloud_and_gt"], xyz[0], gt[0], False)
    case("point_operation.shift_point_cloud_and_gt", pop["shift_point_cloud_and_gt"], xyz[0], gt[0])
    case("point_operation.random_scale_point_cloud_and_gt", lambda p, g: pop["random_scale_point_cloud_and_gt"](p, g)[:2], xyz[0], gt[0])
    # the two *_batch rotations take the point count for the channel count (data_utils.py:218, 282) and fail on [B,N,3] with N > 3:
    # the per-cloud classes stand in for them on xyz; the batch class runs on xyz + normal
    case("data_utils.PointcloudRotate", du["PointcloudRotate"](), T(xyz[0]))
    case("data_utils.PointcloudRotatePerturbation", du["PointcloudRotatePerturbation"](), T(xyz[0]))
    case("data_utils.PointcloudRotatePerturbation_batch.normal", du["PointcloudRotatePerturbation_batch"](), T(xyzn))
    case("data_utils.PointcloudScaleAndTranslate", du["PointcloudScaleAndTranslate"](), T(xyz))
    case("data_utils.PointcloudTranslate", du["PointcloudTranslate"](), T(xyz[0]))
    case("data_utils.PointcloudRandomInputDropout", du["PointcloudRandomInputDropout"](), xyz[0])
    case("data_utils.PointcloudRotatebyAngle", du["PointcloudRotatebyAngle"](), T(xyzn), 0.7)
    np.savez_compressed(os.path.join(HERE, "augment_ref.npz"), **out)
    print("wrote augment_ref.npz: %d arrays" % len(out))


if __name__ == "__main__":
    main()
