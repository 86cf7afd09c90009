"""numpy model of the MST expansion penalty and of minimum-density sampling, written from their stated semantics (include/spgan_hip.h,
"MST expansion penalty and minimum-density sampling"), in float64 or -- for the exact-arithmetic cases -- in float32 with every operation
rounded on its own and the sums in the kernel's documented order.

Expansion penalty, per primitive (a run of p consecutive points):
  * Prim's algorithm from local point 0 on edge lengths sqrt((dx*dx + dy*dy) + dz*dz); a candidate's parent changes only on a strictly
    smaller distance; the next vertex is the unvisited one of least distance, the highest local index among exact ties;
  * mean = (sum of the p-1 edge lengths) / (p-1); mean_mst_length = mean of the cloud's primitive means;
  * synchronous leaf peeling: the leaves of a round are the vertices of remaining degree 1 at its start; leaf t with remaining neighbour
    u takes the edge when cnt_start[u] > 1, or cnt_start[u] == 1 and t > u; then both counts drop;
  * an owned edge longer than mean * alpha gives dist = length, assignment = base_in_cloud + u at the owner; all else 0 / -1;
  * backward: grad_xyz[j] = 2 * grad_dist[j] * (xyz[j] - xyz[assignment[j]]) where assignment != -1, else 0.
Sampling, per cloud: t = 5 L^2, the first pick is 0, a density T starts at 0 (1e9 once selected), every step adds w_k exp(-d_k / t) with
d_k the squared distance to the last pick and w_k = 1 for k < split else 2, and selects the least T, the lowest index among exact ties.
"""
import numpy as np


def wave_sum(vals, dtype):
    """Sum in the kernel's order: s_l = ((v[l] + v[64+l]) + v[128+l]) + .. for l < 64 (missing entries 0), then for o = 32 .. 1:
    s_l = s_l + s_(l xor o) on all l at once; the result is s_0.  In float64 this is just a sum in some order."""
    v = np.asarray(vals, dtype=dtype)
    rows = -(-v.size // 64)
    pad = np.zeros(rows * 64, dtype=dtype)
    pad[:v.size] = v
    pad = pad.reshape(rows, 64)
    s = pad[0].copy()
    for r in range(1, rows):
        s = (s + pad[r]).astype(dtype)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[lanes ^ o]).astype(dtype)
    return s[0]


def edge_lengths(pts, q):
    d = pts - q
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def prim(pts, dtype=np.float64):
    """pts [p,3] -> (parent [p], w [p] with w[0] = 0, gaps): gaps = (least relative gap between a step's best and runner-up candidate,
    least relative gap between the chosen vertex's nearest and second nearest tree vertex), both +inf where there is no second."""
    pts = np.asarray(pts, dtype=dtype)
    p = pts.shape[0]
    cur = np.full(p, np.inf, dtype=dtype)
    par = np.zeros(p, dtype=np.int64)
    vis = np.zeros(p, dtype=bool)
    vis[0] = True
    cur[0] = 0
    last = 0
    step_gap, parent_gap = np.inf, np.inf
    for _ in range(p - 1):
        d = edge_lengths(pts, pts[last])
        upd = ~vis & (d < cur)
        cur[upd] = d[upd]
        par[upd] = last
        cand = np.where(vis, np.inf, cur)
        best = cand.min()
        nxt = int(np.flatnonzero(cand == best).max())
        rest = np.delete(cand, nxt)
        rest = rest[np.isfinite(rest)]
        if rest.size:
            step_gap = min(step_gap, (rest.min() - best) / max(best, np.finfo(dtype).tiny))
        intree = np.sort(edge_lengths(pts[vis], pts[nxt]))
        if intree.size > 1:
            parent_gap = min(parent_gap, (intree[1] - intree[0]) / max(intree[0], np.finfo(dtype).tiny))
        vis[nxt] = True
        last = nxt
    return par, cur, (float(step_gap), float(parent_gap))


def peel(par):
    """Synchronous leaf peeling of the tree given by parent[1:].  -> (other [p]: the other endpoint of the edge vertex t owns, -1 if it
    owns none; rounds)."""
    p = len(par)
    adj = [set() for _ in range(p)]
    for v in range(1, p):
        adj[v].add(int(par[v]))
        adj[int(par[v])].add(v)
    other = -np.ones(p, dtype=np.int64)
    rounds = 0
    left = p - 1
    while left > 0:
        rounds += 1
        cnt = [len(a) for a in adj]
        gone = []
        for t in range(p):
            if cnt[t] != 1:
                continue
            (u,) = adj[t]
            if cnt[u] > 1 or (cnt[u] == 1 and t > u):
                assert other[t] == -1
                other[t] = u
            gone.append((t, u))
        assert gone, "no leaf in a tree with edges left"
        for t, u in gone:
            if u in adj[t]:
                adj[t].discard(u)
                adj[u].discard(t)
                left -= 1
    return other, rounds


def expansion_forward(xyz, p, alpha, dtype=np.float64):
    """xyz [B,n,3] -> dict(dist [B,n], assignment [B,n] int32, mean_mst_length [B], prim_mean [B,n/p], step_gap, parent_gap, thr_margin,
    rounds): the margins are the least over all primitives (thr_margin: least |c - mean*alpha| / (mean*alpha) over the owned edges of the
    primitives with more than one edge)."""
    xyz = np.asarray(xyz, dtype=dtype)
    B, n, _ = xyz.shape
    assert 2 <= p <= 512 and n % p == 0
    dist = np.zeros((B, n), dtype=dtype)
    assign = -np.ones((B, n), dtype=np.int32)
    means = np.zeros((B, n // p), dtype=dtype)
    step_gap = parent_gap = thr_margin = np.inf
    rounds = 0
    alpha = dtype(alpha)
    for b in range(B):
        for j in range(n // p):
            base = j * p
            par, w, (sg, pg) = prim(xyz[b, base:base + p], dtype)
            step_gap, parent_gap = min(step_gap, sg), min(parent_gap, pg)
            mean = dtype(wave_sum(w, dtype) / dtype(p - 1))
            means[b, j] = mean
            thr = dtype(mean * alpha)
            other, r = peel(par)
            rounds = max(rounds, r)
            for t in range(p):
                u = int(other[t])
                if u < 0:
                    continue
                c = w[t] if (t > 0 and u == par[t]) else w[u]
                if p > 2:       # p == 2: the mean IS the edge (c / 1), so c against c * alpha is the same comparison in any precision
                    thr_margin = min(thr_margin, abs(float(c) - float(thr)) / float(thr))
                if c > thr:
                    dist[b, base + t] = c
                    assign[b, base + t] = base + u
    mml = np.array([dtype(wave_sum(means[b], dtype) / dtype(n // p)) for b in range(B)], dtype=dtype)
    return dict(dist=dist, assignment=assign, mean_mst_length=mml, prim_mean=means, step_gap=float(step_gap), parent_gap=float(parent_gap),
                thr_margin=float(thr_margin), rounds=rounds)


def expansion_backward(xyz, grad_dist, assignment):
    """float64 closed form on a given assignment."""
    xyz = np.asarray(xyz, dtype=np.float64)
    g = np.asarray(grad_dist, dtype=np.float64)
    a = np.asarray(assignment)
    B = xyz.shape[0]
    out = np.zeros_like(xyz)
    for b in range(B):
        own = a[b] >= 0
        out[b, own] = 2.0 * g[b, own, None] * (xyz[b, own] - xyz[b, a[b, own]])
    return out


def mds(xyz, npoint, L, split=8192, dtype=np.float64, follow=None):
    """One cloud xyz [n,3] -> (picks [npoint], picked [npoint], least [npoint], A): the density of the point picked at step j and the least
    density at that step (entry 0 unused), A = max d / t over the steps.  follow: a pick sequence to run along in place of the model's own
    arg-min (lowest index on ties)."""
    x = np.asarray(xyz, dtype=dtype)
    n = x.shape[0]
    L = np.float64(np.float32(L))
    t = dtype(np.float32(5.0 * L * L)) if dtype == np.float32 else dtype(5.0 * L * L)
    w = np.where(np.arange(n) < split, dtype(1), dtype(2)).astype(dtype)
    T = np.zeros(n, dtype=dtype)
    T[0] = dtype(1e9)
    picks = np.zeros(npoint, dtype=np.int64)
    picked = np.zeros(npoint, dtype=np.float64)
    least = np.zeros(npoint, dtype=np.float64)
    last, A = 0, 0.0
    for j in range(1, npoint):
        d = x - x[last]
        d = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        A = max(A, float(d.max() / t))
        T = (T + w * np.exp(-d / t).astype(dtype)).astype(dtype)
        sel = int(np.argmin(T)) if follow is None else int(follow[j])
        picks[j], picked[j], least[j] = sel, T[sel], T.min()
        T[sel] = dtype(1e9)
        last = sel
    return picks, picked, least, A
