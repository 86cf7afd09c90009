"""A plain torch model of the double backward of the max-aggregation edge convolution (spgan.edgeConv(double_backward=True),
csrc/edge_max.hip's dbl passes), on top of tests/edgeconv_model.py's forward_pq / backward_pq.

The scalar differentiated is L = <v, dx>, v the cotangent on the first backward's input gradient.  With VPQ = v Wst^T = [VP | VQ] the
edge value of v is t_e = VQ_i + VP_n(e), gathered like z_e = Q_i + P_n(e), and L = a * A with A = S - s1 T1/E - s2 T2/E:

    T1 = sum_e t_e,   T2 = sum_e t_e xhat_e,   S = sum_i r_i t_{e*(i)},   s1 = sum r,   s2 = sum r_i xhat_{e*(i)},   c = a invstd / E
    ghat_i  = 1[out_i > 0] a (t_{e*(i)} - T1/E - xhat_{e*(i)} T2/E)                                  (cotangent of g)
    gammabar = invstd A
    zbar_e  = -c A xhat_e - c T2 [r_i d(e = e*(i)) - s1/E - xhat_e s2/E] - c s2 [t_e - T1/E - xhat_e T2/E]
    Qbar_i = sum_j zbar_(i,j),   Pbar_m = sum_{e -> m} zbar_e,   VPbar = dP,   VQbar = dQ  (the first backward's)
and in eval mode (statistics constant) ghat_i = 1[out_i > 0] a t_{e*(i)}, gammabar = invstd S, zbar = 0.

Like the first-order model this one DOES materialise the per-edge tensors ([B,N,k,F]): zbar is formed edge by edge from the formula
above, not from the per-point expansion the kernels use, so the two are independent.  The selection and the ReLU mask may be handed in
(the kernel's), as in backward_pq."""
import torch

import edgeconv_model as ecm


def double_backward_pq(f, g_pm, VP, VQ, sel=None, active=None):
    """f = forward_pq's dict, g_pm [B,N,F] the cotangent of out, VP / VQ [B,N,F] the direction's per-point products.
    -> dict(ghat [B,N,F], gammabar [F], Pbar, Qbar [B,N,F] (zeros in eval mode), dP, dQ (the first backward's), T1, T2, S, A [F])."""
    P, Q, Pn, a, mean, invstd, k, idx = (f[n] for n in ("P", "Q", "Pn", "a", "mean", "invstd", "k", "idx"))
    B, N, F = P.shape
    E = B * N * k
    sel = f["sel"] if sel is None else sel
    active = (f["out_pm"] > 0) if active is None else active
    first = ecm.backward_pq(f, g_pm, sel, active)
    r, s1, s2 = first["r"], first["dbeta"], first["dgamma"]
    act = active.to(P.dtype)
    t = VQ.unsqueeze(2) + ecm.gather_neighbours(VP, idx, k)                       # [B,N,k,F]
    xhat = (Q.unsqueeze(2) + Pn - mean) * invstd
    pick = sel.unsqueeze(2)
    t_sel, x_sel = torch.gather(t, 2, pick).squeeze(2), torch.gather(xhat, 2, pick).squeeze(2)
    T1, T2, S = t.sum(dim=(0, 1, 2)), (t * xhat).sum(dim=(0, 1, 2)), (r * t_sel).sum(dim=(0, 1))
    o = dict(dP=first["dP"], dQ=first["dQ"], r=r, T1=T1, T2=T2, S=S)
    if not f["training"]:
        o.update(ghat=act * a * t_sel, gammabar=invstd * S, Pbar=torch.zeros_like(P), Qbar=torch.zeros_like(P), A=S)
        return o
    A = S - s1 * T1 / E - s2 * T2 / E
    c = a * invstd / E
    onehot = (torch.arange(k, device=P.device).view(1, 1, k, 1) == pick).to(P.dtype)
    zbar = (-c * A * xhat - c * T2 * (r.unsqueeze(2) * onehot - s1 / E - xhat * s2 / E) - c * s2 * (t - T1 / E - xhat * T2 / E))
    Pbar = torch.zeros_like(P).scatter_add_(1, idx.unsqueeze(2).expand(B, N * k, F), zbar.reshape(B, N * k, F))
    o.update(ghat=act * a * (t_sel - T1 / E - x_sel * T2 / E), gammabar=invstd * A, Pbar=Pbar, Qbar=zbar.sum(dim=2), A=A)
    return o


def double_backward(f, g, v, sel=None, active=None):
    """f = forward's dict, g [B,F,N] the cotangent of out, v [B,Fin,N] the cotangent of dx
    -> dict(ghat [B,F,N], xbar [B,Fin,N] (zeros in eval mode), Wbar [F,2Fin,1,1], gammabar [F]) and double_backward_pq's entries."""
    x, W2 = f["x"], f["W2"]
    F, Fin = W2.shape[0], x.shape[1]
    Wc, Wd = W2[:, :Fin], W2[:, Fin:]
    xp, vp = x.transpose(1, 2), v.transpose(1, 2)
    o = double_backward_pq(f, g.transpose(1, 2), vp @ Wd.t(), vp @ (Wc - Wd).t(), sel, active)
    # Wst = [Wd ; Wc - Wd] meets L through PQ = x Wst^T (cotangent PQbar) and through VPQ = v Wst^T (cotangent dPQ)
    WP = torch.einsum("bnf,bnc->fc", o["Pbar"], xp) + torch.einsum("bnf,bnc->fc", o["dP"], vp)
    WQ = torch.einsum("bnf,bnc->fc", o["Qbar"], xp) + torch.einsum("bnf,bnc->fc", o["dQ"], vp)
    o.update(xbar=(o["Pbar"] @ Wd + o["Qbar"] @ (Wc - Wd)).transpose(1, 2), Wbar=torch.cat([WQ, WP - WQ], dim=1).view(F, 2 * Fin, 1, 1))
    o["ghat"] = o["ghat"].transpose(1, 2)
    return o


def brute_force_graph(x, k):
    """x [B,C,N] -> int64 [B, N*k]: the k nearest other points by squared distance (float64, stable order), the reference's convention"""
    xp = x.double().transpose(1, 2)
    d = torch.cdist(xp, xp) ** 2
    d.diagonal(dim1=1, dim2=2).fill_(-1.0)
    return d.argsort(dim=2, stable=True)[:, :, 1:k + 1].reshape(x.shape[0], -1)
