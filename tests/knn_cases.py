"""Inputs with a known answer for the kNN graph kernels (csrc/graph.hip, csrc/knn_pipe.hip), and the float64 reference they are
compared with.  Shared by tests/test_knn_exact_gpu.py (the kernels) and tests/test_knn_cases_cpu.py (the cases themselves).

Three kinds of cloud, all drawn from spgan.fixture_rng by name:

* lattice    -- every coordinate a small integer (|v| <= 3).  Such a value is exactly a bfloat16 (its mid and lo planes are zero), every
                product and partial sum is an integer far below 2^24, so the expanded form |x|^2 + |y|^2 - 2xy is EXACT in fp32 in any
                summation order, on the VALU, the fp32 MFMA and the split-bf16 MFMA alike.  Distances tie massively; the output is then
                defined by the order contract alone: stable ascending (distance, index), rank 0 dropped positionally.  Rows 0..N/8 of
                shape 0 are copied onto rows N/2..N/2+N/8: a query of the second block has a twin with a LOWER index at distance 0, so it
                is not rank 0 of its own list -- the twin is what gets dropped, the query itself is returned first.
* prototype  -- row i = proto[i % m] for m well-separated fp32 rows.  Identical operands give identical distances whatever the rounding,
                so query q expects the indices = q (mod m) in ascending order, the first one dropped.  m = 1 is a fully collapsed cloud.
* offset     -- x = 8 + 0.5 * normal: |x|^2 is two orders of magnitude above the neighbour distances, the regime where the expanded form
                cancels and a dropped low-order term of the split shows.  Checked tie-aware against offset_tol().

Run as a script (`python tests/knn_cases.py mfma-child`) this module is the child process of
test_knn_exact_gpu.py::test_fp32_mfma_kernel_in_a_child_process: the switch SPGAN_KNN_BF16X3 is read once per process.
"""
import collections
import functools
import os
import sys

import torch

if __name__ == "__main__":                                   # the child process has no conftest: same path set-up
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_ROOT, os.path.join(_ROOT, "sp-gan_amd"), os.path.join(_ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from spgan import fixture_rng as fr

# ----------------------------------------------------------------------------- float64 reference


def sorted_dist_f64(x_pm, B, N):
    """Direct differences in float64 -> (sorted distances [B,N,N], stable order [B,N,N])."""
    C = x_pm.shape[1]
    x = x_pm.detach().cpu().double().view(B, N, C)
    d = torch.zeros((B, N, N), dtype=torch.float64)
    for c0 in range(0, C, 16):                               # channel chunks: [B,N,N,16] instead of [B,N,N,C]
        t = x[:, :, None, c0:c0 + 16] - x[:, None, :, c0:c0 + 16]
        d += (t * t).sum(-1)
    return torch.sort(d, dim=2, stable=True)


def stable_knn_f64(x_pm, B, N, k):
    """The contract, independent of the expanded form the kernels and kernel_model.knn(mode=0) use: float64 direct differences,
    stable sort, columns 1..k, global row numbers.  -> int32 [B*N, k]."""
    order = sorted_dist_f64(x_pm, B, N)[1][:, :, 1:k + 1]
    off = (torch.arange(B) * N).view(B, 1, 1)
    return (order + off).reshape(B * N, k).to(torch.int32)


# ----------------------------------------------------------------------------- lattice clouds
# route: which launch of spgan_knn / spgan_knn_ws the shape reaches with the default environment.  R: integer range [-R, R].
LatticeCase = collections.namedtuple("LatticeCase", "route C N k B R mode")

LATTICE_F64 = [            # knn_f64_kernel<KP, C> (mode 1): KP 11 / 21 / 11 / 33
    LatticeCase("f64", 1, 11, 10, 2, 3, 1),
    LatticeCase("f64", 2, 257, 20, 3, 3, 1),
    LatticeCase("f64", 3, 300, 10, 2, 3, 1),
    LatticeCase("f64", 4, 65, 32, 3, 3, 1),
]
LATTICE_F32 = [            # knn_f32_kernel<KP, CP>
    LatticeCase("f32<11,8>", 5, 300, 10, 2, 3, 0),
    LatticeCase("f32<21,16>", 9, 65, 20, 3, 2, 0),
    LatticeCase("f32<33,16>", 16, 77, 32, 2, 2, 0),
    LatticeCase("f32<21,32>", 20, 97, 20, 3, 2, 0),
    LatticeCase("f32<21,64>", 64, 130, 11, 2, 1, 0),
    LatticeCase("f32<33,128>", 100, 65, 32, 3, 1, 0),
    LatticeCase("f32<21,128>", 128, 130, 20, 2, 1, 0),
    LatticeCase("f32<33,64>", 33, 33, 32, 3, 2, 0),          # k + 1 == N
]
LATTICE_MATRIX = [         # k <= 10, 16 < C <= 64: knn_split_kernel + knn_pipe_kernel (ops.KNN_PIPELINED) or knn_mfma3_kernel<11,64> (not)
    LatticeCase("mc", 17, 11, 10, 2, 2, 0),                  #  1 tile, k + 1 == N
    LatticeCase("mc", 40, 31, 7, 3, 1, 0),                   #  1 tile, ragged
    LatticeCase("mc", 64, 32, 10, 2, 1, 0),                  #  1 tile, full
    LatticeCase("mc", 17, 33, 1, 3, 1, 0),                   #  2 tiles (one pair), one candidate in the second
    LatticeCase("mc", 40, 64, 10, 2, 1, 0),                  #  2 tiles, full
    LatticeCase("mc", 64, 65, 7, 3, 1, 0),                   #  3 tiles: a pair + a last single tile; every ring slot once
    LatticeCase("mc", 17, 96, 10, 2, 2, 0),                  #  3 tiles, full
    LatticeCase("mc", 40, 97, 1, 3, 1, 0),                   #  4 tiles, the ring wraps
    LatticeCase("mc", 64, 129, 10, 2, 1, 0),                 #  5 tiles, two query groups (the second with one query)
    LatticeCase("mc", 17, 161, 7, 3, 2, 0),                  #  6 tiles
    LatticeCase("mc", 40, 257, 10, 2, 1, 0),                 #  9 tiles, three query groups
    LatticeCase("mc", 64, 257, 1, 2, 1, 0),
]
LATTICE_MFMA3_128 = [      # k <= 10, 64 < C <= 128: knn_mfma3_kernel<11,128>
    LatticeCase("mfma3<11,128>", 65, 97, 10, 2, 1, 0),
    LatticeCase("mfma3<11,128>", 100, 33, 3, 3, 1, 0),
    LatticeCase("mfma3<11,128>", 128, 130, 10, 2, 1, 0),
]
LATTICE_CASES = LATTICE_F64 + LATTICE_F32 + LATTICE_MATRIX + LATTICE_MFMA3_128
# With SPGAN_KNN_BF16X3=0 and the single-launch route these reach knn_mfma_kernel<11,64> (two) and knn_mfma_kernel<11,128> (two).
MFMA_CHILD_CASES = [LATTICE_MATRIX[8], LATTICE_MATRIX[9], LATTICE_MFMA3_128[0], LATTICE_MFMA3_128[2]]


def case_id(c):
    return "C%d-N%d-k%d" % (c.C, c.N, c.k)


@functools.lru_cache(maxsize=None)
def lattice(case):
    """-> (x [B*N, C] fp32 on the CPU, stable_knn_f64 of it).  Cached: computed once, shared, never modified."""
    B, N, C, R = case.B, case.N, case.C, case.R
    x = fr.uniform("knnx.lat.%d.%d.%d" % (C, N, case.k), (B * N, C), -(R + 0.5), R + 0.5).round().clamp(-R, R) + 0.0   # + 0.0: no -0
    n8 = N // 8
    x[N // 2:N // 2 + n8] = x[:n8].clone()                   # exact twins inside shape 0
    x = x.contiguous()
    return x, stable_knn_f64(x, B, N, case.k)


# ----------------------------------------------------------------------------- prototype clouds
PROTO_M = (1, 2, 5)


def prototype_cloud(B, N, C, m, lattice_protos=False):
    """Row i of shape b = proto[b][i % m]; other prototypes per shape."""
    name = "knnx.proto.%d.%d.%d" % (N, C, m)
    if lattice_protos:
        proto = fr.uniform(name, (B, m, C), -3.5, 3.5).round().clamp(-3, 3) + 0.0
    else:
        proto = fr.normal(name, (B, m, C), 0.5)
    if m > 1:                                                # well separated: squared distance >= 1 between any two of a shape
        d = ((proto[:, :, None, :].double() - proto[:, None, :, :].double()) ** 2).sum(-1) + torch.eye(m) * 1e9
        assert d.min().item() >= 1.0, "prototypes too close (%.3g): pick another name" % d.min().item()
    return proto[:, torch.arange(N) % m, :].reshape(B * N, C).contiguous()


def prototype_expected(B, N, m, k):
    """Query q: the rows = q (mod m) ascending are q % m, q % m + m, ...; the first is dropped positionally.  -> int32 [B*N, k]."""
    assert (k + 1) * m <= N
    loc = (torch.arange(N) % m)[:, None] + m * torch.arange(1, k + 1)[None, :]
    off = (torch.arange(B) * N).view(B, 1, 1)
    return (loc[None] + off).reshape(B * N, k).to(torch.int32)


# ----------------------------------------------------------------------------- offset clouds
def offset_cloud(B, N, C):
    return fr.normal("knnx.off.%d.%d" % (N, C), (B * N, C), 0.5, 8.0)


ALIGNED_LO_SHAPE = (2, 97, 17, 10)       # (B, N, C, k): the smallest C of the matrix-core routes, where the worst-case bound is tightest


def aligned_lo_cloud(B, N, C):
    """An offset cloud whose third bfloat16 plane is the same in every channel of a row: x = hi + mid + lo with hi = 10 +- 1.5 on a
    2^-4 grid, mid = +-(65..127) * 2^-12 and lo = +2^-14 on even rows, -2^-14 on odd rows (the split of csrc/split_bf16.hpp reproduces
    exactly these planes).  A product that loses the lo plane moves every distance to an even candidate against every distance to an
    odd one by 4 * C * 10 * 2^-14 -- 0.04 at C = 17, four times offset_tol() -- in one direction in all channels, where random low
    planes average out: neighbours of different parity closer than that swap, and the swap is a rank error above the bound."""
    name = "knnx.alo.%d.%d" % (N, C)
    hi = ((10.0 + fr.normal(name + ".hi", (B * N, C), 0.5).clamp(-1.5, 1.5)) * 16).round() / 16
    u = fr.uniform(name + ".mid", (B * N, C), -63.0, 63.0)
    mid = torch.where(u < 0, u.floor() - 64, u.floor() + 65).clamp(-127, 127) * 2.0 ** -12
    lo = torch.where(torch.arange(B * N) % 2 == 0, 1.0, -1.0)[:, None] * 2.0 ** -14
    return ((hi + mid) + lo).contiguous()


def split_bf16(x):
    """hi, mid, lo of the split-bf16 scheme (round to nearest even at every step), as fp32."""
    hi = x.bfloat16().float()
    mid = (x - hi).bfloat16().float()
    lo = ((x - hi) - mid).bfloat16().float()
    return hi, mid, lo


def offset_tol(x_pm):
    """Derived, not measured: the worst-case error of the expanded form (-2 x.y + |x|^2) + |y|^2 in fp32, any summation order, with
       u = 2^-24 and M = max_i |x_i|^2:
         two length-C dots / norms at gamma_C on each side        <= 4 C u M
         the split-bf16 product's dropped cross terms              <= 6 u M
         the two final additions                                   <= 7 u M
       rounded up to (4 C + 16) u M."""
    C = x_pm.shape[1]
    M = (x_pm.double() ** 2).sum(1).max().item()
    return (4 * C + 16) * 2.0 ** -24 * M


def rank_error(idx, x_pm, B, N, k, sd=None):
    """max |exact distance of the returned rank-r neighbour - exact (r+1)-th smallest distance| (what knn_tie_aware bounds)."""
    C = x_pm.shape[1]
    x = x_pm.detach().cpu().double().view(B, N, C)
    if sd is None:
        sd = sorted_dist_f64(x_pm, B, N)[0]
    loc = idx.cpu().long().view(B, N, k) - (torch.arange(B) * N).view(B, 1, 1)
    nb = torch.gather(x[:, None].expand(B, N, N, C), 2, loc[..., None].expand(B, N, k, C))
    got = ((x[:, :, None, :] - nb) ** 2).sum(-1)
    return (got - sd[:, :, 1:k + 1]).abs().max().item()


# ----------------------------------------------------------------------------- child process: knn_mfma_kernel
def first_difference(got, ref):
    """None when equal, else a one-line description of the first differing row."""
    got, ref = got.cpu(), ref.cpu()
    if torch.equal(got, ref):
        return None
    row = int((got != ref).any(dim=1).nonzero()[0])
    return "row %d: got %s expected %s" % (row, got[row].tolist(), ref[row].tolist())


def _mfma_child():
    assert os.environ.get("SPGAN_KNN_BF16X3") == "0", "start this with SPGAN_KNN_BF16X3=0"
    from spgan import _lib, ops
    _lib.load()
    ops.KNN_PIPELINED[0] = False                             # spgan_knn: with the switch at 0 its k <= 10, C > 16 launch is knn_mfma_kernel
    for c in MFMA_CHILD_CASES:
        x, ref = lattice(c)
        diff = first_difference(ops.knn(x.cuda(), c.B, c.N, c.k, mode=0), ref)
        if diff is not None:
            print("MFMA-CHILD DIFF %s %s" % (case_id(c), diff))
            return 1
    print("MFMA-CHILD OK %d cases" % len(MFMA_CHILD_CASES))
    return 0


if __name__ == "__main__":
    if sys.argv[1:] != ["mfma-child"]:
        sys.exit("usage: knn_cases.py mfma-child")
    sys.exit(_mfma_child())
