"""Inputs of tests/test_expansion_gpu.py, built on the CPU (so their margins can be inspected without a GPU)."""
import numpy as np

import expansion_model as em

# (B, n, p, seed): random clouds in [0,1)^3.  A seed is replaced, never a margin loosened, when a case misses the margins the GPU test asserts
# (p = 512: seed 0 has an edge 1.3e-5 from its threshold, seed 6 has none within 1.7e-4).
RANDOM_CASES = [(1, 64, 64, 0), (3, 384, 128, 0), (2, 1024, 512, 6), (2, 195, 65, 0), (1, 12, 3, 0), (2, 16, 2, 0),
                (1, 512, 256, 0), (1, 600, 300, 0)]      # the last two: four vertices per lane; a workgroup-per-primitive size that is no multiple of 64
ALPHAS = (1.0, 1.5)


def random_cloud(B, n, seed):
    return np.random.default_rng(seed).random((B, n, 3)).astype(np.float32)


def lattice(nx, ny, nz):
    """Small integers times 0.25: squared lengths are exact in float32, so both sides round the same square roots."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return (g.astype(np.float32) * np.float32(0.25))[None]


def collinear(p=512):
    x = np.zeros((1, p, 3), dtype=np.float32)
    x[0, :, 0] = np.arange(p, dtype=np.float32) * np.float32(0.25)
    return x


def pair():
    return np.array([[[0.0, 0.0, 0.0], [0.75, 0.0, 0.0]]], dtype=np.float32)


# name -> (xyz, p, alpha)
EXACT_CASES = {
    "lattice4x4": (lattice(4, 4, 1), 16, 0.5),
    "lattice4x4x4": (lattice(4, 4, 4), 64, 0.5),
    "pair": (pair(), 2, 0.5),
    "collinear512": (collinear(512), 512, 0.5),
}

# (B, n, npoint, L per cloud, split): clouds in [0, 10 min L)^3, so that A = max d / (5 L^2) <= 3 * 100 / 5 = 60
MDS_CASES = {
    "all": (1, 70, 70, (0.1,), 8192),
    "percloud": (3, 300, 64, (0.06, 0.08, 0.1), 8192),
    "default_split": (1, 8200, 48, (0.05,), 8192),
    "split100": (1, 300, 64, (0.08,), 100),
}


def mds_cloud(name):
    B, n, npoint, L, split = MDS_CASES[name]
    rng = np.random.default_rng(7)
    x = (rng.random((B, n, 3)) * (10.0 * min(L))).astype(np.float32)
    if name == "default_split":
        # only 8 points lie behind the default split: move the points the equal-weight run picks first there, so that doubling their
        # weight changes the sequence (the GPU test asserts that it does)
        first = em.mds(x[0], 12, L[0], split=n)[0][1:9]
        perm = np.arange(n)
        perm[first], perm[split:split + 8] = perm[split:split + 8].copy(), perm[first].copy()
        x = np.ascontiguousarray(x[:, perm])
    return x, npoint, np.asarray(L, dtype=np.float32), split
