"""Float64 restatement (plain torch, any device) of the layers of spgan.gan_layers, written from the formulas of DESIGN 36 and not from the
kernels: grouped spectral normalisation, the minibatch-stddev channel, and the layer epilogue
y = gamma * IN(PN(act(x + w * noise))) + beta.  Gradients come from autograd over these float64 expressions (`vjp`), with the power
iteration's u and v held constant as the layers define it.  `ref32_*` are the REFERENCE's float32 formulations composed from torch ops
(Generation/modules.py), used by the GPU tests to measure e_ref, the error float32 torch itself makes against this model.

tests/test_gan_layers_cpu.py pins this model to tests/golden/gan_layers.npz (the reference's own classes run in float64)."""
import torch
import torch.nn.functional as F

RULE_L2NORMALIZE, RULE_F_NORMALIZE = 0, 1
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
PN_NONE, PN_RSQRT, PN_SQRT_DIV = 0, 1, 2
STATS_NONE, STATS_CHANNEL, STATS_JOINT = 0, 1, 2

# the cases of the issue
SN_SHAPES = [(1, 64), (64, 3), (128, 64), (5, 7), (16, 128, 1, 1), (8, 6, 1, 4), (1024, 256)]
MBSTD_CASES = [(8, 5, 70, 4, 1), (3, 4, 1, 4, 1), (8, 6, 2048, 4, 2), (4, 1, 65, 2, 1)]          # (B, C, N, group, F)
EPILOGUE_SHAPES = [(3, 5, 70), (2, 128, 257), (2, 1024, 3)]


def d(t):
    return None if t is None else t.detach().double()


def normalise(x, rule, eps):
    n = x.norm()
    return x / (n + eps) if rule == RULE_L2NORMALIZE else x / torch.clamp(n, min=eps)


def sn_forward(W, u, v, n_iter, rule=RULE_F_NORMALIZE, eps=1e-12):
    """-> (W / sigma, sigma, u', v'); W differentiable, u', v' constants"""
    Wm = W.reshape(W.shape[0], -1)
    u, v = u.detach(), v.detach()
    with torch.no_grad():
        for _ in range(n_iter):
            v = normalise(Wm.t().mv(u), rule, eps)
            u = normalise(Wm.mv(v), rule, eps)
    sigma = u.dot(Wm.mv(v))
    return W / sigma, sigma, u, v


def sn_backward(G, W, sigma, u, v):
    """dW = G / sigma - (<G,W> / sigma^2) u v^T"""
    return G / sigma - ((G * W).sum() / sigma ** 2) * torch.outer(u, v).reshape(W.shape)


def mbstd_forward(x, group_size=4, num_new=1, alpha=1e-8):
    B, C, N = x.shape
    G = min(group_size, B)
    M, Cp = B // G, C // num_new
    y = x.reshape(G, M, num_new, Cp, N)
    std = ((y - y.mean(0, keepdim=True)).pow(2).mean(0) + alpha).sqrt()          # [M,F,C',N]
    stat = std.mean(dim=(2, 3))                                                  # [M,F]
    new = stat.reshape(1, M, num_new, 1).expand(G, M, num_new, N).reshape(B, num_new, N)
    return torch.cat([x, new], 1)


def act_fn(z, act, slope):
    return z if act == ACT_NONE else (z.clamp(min=0) if act == ACT_RELU else torch.where(z > 0, z, z * slope))


def epilogue_forward(x, noise=None, w=None, act=ACT_NONE, slope=0.2, pn=PN_NONE, pn_eps=1e-8, stats=STATS_NONE, in_eps=1e-5, gamma=None,
                     beta=None):
    """x [B,C,L]; noise [B,L]; w [C]; gamma, beta [B,C]"""
    t = x
    if noise is not None:
        t = t + w.reshape(1, -1, 1) * noise.reshape(x.shape[0], 1, -1)
    t = act_fn(t, act, slope)
    if pn != PN_NONE:
        t = t / (t.pow(2).mean(1, keepdim=True) + pn_eps).sqrt()
    if stats != STATS_NONE:
        dims = (2,) if stats == STATS_CHANNEL else (1, 2)
        mu = t.mean(dims, keepdim=True)
        var = (t - mu).pow(2).mean(dims, keepdim=True)
        t = (t - mu) / (var + in_eps).sqrt()
    if gamma is not None:
        t = gamma.unsqueeze(2) * t + beta.unsqueeze(2)
    return t


def truncation_forward(x, avg, max_layer, thr):
    keep = (torch.arange(x.shape[1], device=x.device) < max_layer).view(1, -1, 1)
    return torch.where(keep, avg + thr * (x - avg), x)


def vjp(fn, inputs, g):
    """gradients of sum(fn(*inputs) * g) with respect to the inputs that are not None"""
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    grads = torch.autograd.grad((out * g).sum(), [t for t in leaves if t is not None], allow_unused=True)
    it = iter(grads)
    return out.detach(), [None if t is None else next(it) for t in leaves]


# ------------------------------------------------------------------------------------------------ the reference's float32 formulations
def ref32_sn(W, u, v, n_iter, rule, eps):
    """SpectralNorm._update_u_v (rule 0) / torch.nn.utils.spectral_norm's compute_weight (rule 1) in W's dtype"""
    Wm = W.reshape(W.shape[0], -1)
    u, v = u.detach().clone(), v.detach().clone()
    with torch.no_grad():
        for _ in range(n_iter):
            if rule == RULE_L2NORMALIZE:
                v = torch.mv(Wm.t(), u); v = v / (v.norm() + eps)
                u = torch.mv(Wm, v); u = u / (u.norm() + eps)
            else:
                v = F.normalize(torch.mv(Wm.t(), u), dim=0, eps=eps)
                u = F.normalize(torch.mv(Wm, v), dim=0, eps=eps)
    sigma = torch.dot(u, torch.mv(Wm, v))
    return W / sigma, sigma, u, v


def ref32_mbstd(x, group_size, num_new, alpha=1e-8):
    """StddevLayer.forward (MinibatchStdDev's is its num_new = 1 case)"""
    B, C, N = x.shape
    G = min(group_size, B)
    y = x.reshape([G, -1, num_new, C // num_new, N])
    y = y - y.mean(0, keepdim=True)
    y = (y ** 2).mean(0, keepdim=True)
    y = (y + alpha) ** 0.5
    y = y.mean([3, 4], keepdim=True).squeeze(3)
    y = y.expand(G, -1, -1, N).clone().reshape(B, num_new, N)
    return torch.cat([x, y], dim=1)


def ref32_epilogue(x, noise, w, act, slope, pn, pn_eps, stats, gamma, beta):
    """the chain NoiseLayer -> activation -> PixelNorm / PixelwiseNorm -> nn.InstanceNorm2d -> gamma * . + beta in x's dtype"""
    t = x
    if noise is not None:
        t = t + w.view(1, -1, 1) * noise.view(x.shape[0], 1, -1)
    if act == ACT_RELU:
        t = F.relu(t)
    elif act == ACT_LRELU:
        t = F.leaky_relu(t, slope)
    if pn == PN_RSQRT:
        t = t * torch.rsqrt(torch.mean(t ** 2, dim=1, keepdim=True) + pn_eps)
    elif pn == PN_SQRT_DIV:
        t = t / t.pow(2.0).mean(dim=1, keepdim=True).add(pn_eps).sqrt()
    if stats == STATS_JOINT:
        t = F.instance_norm(t.unsqueeze(0), eps=1e-5).squeeze(0)          # what nn.InstanceNorm2d makes of an unbatched [B,C,N]
    elif stats == STATS_CHANNEL:
        t = F.instance_norm(t, eps=1e-5)
    if gamma is not None:
        t = gamma.unsqueeze(2) * t + beta.unsqueeze(2)
    return t
