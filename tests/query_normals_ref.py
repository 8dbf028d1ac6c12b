"""Reference for the density gradient and unit normal at query points (csrc/planes_query_normals.hip,
csrc/planes_query_normals_bwd.hip, `sample_mixed(normals=True)`, `synthesis(query_normals=True)`), in whatever dtype it is asked
for (float64: the ground truth; float32: the oracle's own error).

  forward    tests/normals_ref.sample_normals: autograd of the oracle's osg_decoder(sample_from_planes(...)) w.r.t. the points.
  backward   second-order autograd through tests/normal_grad_ref.gather_from_planes (grid_sample has no double backward): the
             loss <n, G_n> + <g, G_g> differentiated w.r.t. the planes and the four decoder tensors.
The inputs are tests/query_ref.base_case(): B = 2, planes 20 x 28, M = 149 points that keep 1e-3 texel clear of every texel edge,
so every point is compared.  Shared by tests/test_query_normals_cpu.py and tests/test_gpu_query_normals.py."""
import functools
import types

import torch

from tests import normal_grad_ref as NG
from tests import normals_ref as N
from tests import query_ref as Q

DEC_KEYS = Q.DEC_KEYS
G_SEED = 17
UPSTREAM = {"normal": (False, True), "grad": (True, False), "both": (True, True)}        # (G_g used, G_n used)


def _cfg(axes, box_warp, lr_mul):
    return types.SimpleNamespace(plane_axes=axes, box_warp=box_warp, decoder_lr_mul=lr_mul)


def forward(P, planes_nchw, coords, axes, box_warp=Q.BOX_WARP, lr_mul=Q.LR_MUL, dtype=torch.float64):
    """planes [B,3,32,H,W] (the oracle's layout), coords [Bc,M,3] -> dict(sigma [B,M,1], g [B,M,3], n [B,M,3]) in `dtype`."""
    P = {k: P[k].detach().to(dtype) for k in DEC_KEYS}
    pl = planes_nchw.detach().to(dtype)
    x = coords.detach().to(dtype).expand(pl.shape[0], -1, -1).contiguous()
    sigma, g, n = N.sample_normals(P, _cfg(axes, box_warp, lr_mul), pl, x)
    return dict(sigma=sigma, g=g.detach(), n=n.detach())


def backward(P, planes_nchw, coords, g_grad, g_normal, axes, box_warp=Q.BOX_WARP, lr_mul=Q.LR_MUL, dtype=torch.float64):
    """Autograd of <g, g_grad> + <n, g_normal> (either upstream may be None) -> dict(planes [B,3,32,H,W], dec (four tensors))."""
    from oracle import eg3d_oracle as O
    P = {k: P[k].detach().to(dtype).requires_grad_(True) for k in DEC_KEYS}
    pl = planes_nchw.detach().to(dtype).requires_grad_(True)
    x = coords.detach().to(dtype).expand(pl.shape[0], -1, -1).contiguous().requires_grad_(True)
    with torch.enable_grad():
        _, sigma = O.osg_decoder(P, NG.gather_from_planes(axes, pl, x, box_warp), lr_mul)
        g, = torch.autograd.grad(sigma.sum(), x, create_graph=True)
        n = -g * torch.rsqrt((g * g).sum(-1, keepdim=True) + 1e-12)
        loss = 0.0
        if g_grad is not None:
            loss = loss + (g * g_grad.to(dtype)).sum()
        if g_normal is not None:
            loss = loss + (n * g_normal.to(dtype)).sum()
        wrt = [pl] + [P[k] for k in DEC_KEYS]
        grads = torch.autograd.grad(loss, wrt, allow_unused=True)
    grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, wrt)]
    return dict(planes=grads[0], dec=tuple(grads[1:]), g=g.detach(), n=n.detach())


@functools.lru_cache(maxsize=None)
def upstream():
    """(G_g, G_n) [B,M,3] for the base case (random, seeded)."""
    g = torch.Generator().manual_seed(G_SEED)
    return torch.randn(Q.B, Q.M, 3, generator=g), torch.randn(Q.B, Q.M, 3, generator=g)


@functools.lru_cache(maxsize=None)
def base_forward(axes, broadcast=False, dtype=torch.float64):
    cs = Q.base_case()
    return forward(cs["P"], cs["pn"], cs["coords"][:1] if broadcast else cs["coords"], axes, dtype=dtype)


@functools.lru_cache(maxsize=None)
def base_backward(axes, which, dtype=torch.float64):
    """`backward` on the base case (computed once per configuration and left unchanged)."""
    cs = Q.base_case()
    use_g, use_n = UPSTREAM[which]
    gg, gn = upstream()
    return backward(cs["P"], cs["pn"], cs["coords"], gg if use_g else None, gn if use_n else None, axes, dtype=dtype)


def worst(got, ref, what):
    """NG.bar_ratio of one tensor, printed."""
    r = NG.bar_ratio(got, ref)
    print(f"{what}: err / bound {r:.3f} (ref max {float(ref.abs().max()):.3e})")
    return r


def rho(got_planes_nchw, got_dec, ref, what):
    """The worst bar ratio over d_planes and the four decoder gradients; prints every figure."""
    parts = {"planes": NG.bar_ratio(got_planes_nchw, ref["planes"])}
    for k, a, b in zip(DEC_KEYS, got_dec if got_dec is not None else (), ref["dec"]):
        parts[k] = NG.bar_ratio(a, b)
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in parts.items()))
    return max(parts.values())
