"""The arithmetic of hfagp_trace_rays (csrc/surface_trace.hip, include/hfagp.h) restated in torch, against a density callable
``sigma(x)``: x [..., 3] -> [...] — an analytic field, the float64 oracle, or `ops.planes_query` on the device.  Every operation is a
separate torch op in the dtype of the rays, so that in fp32 on the device, fed the kernel's own densities, it reproduces the kernel's
decisions: `cell` and `hit` exactly, `t` to the last bits.  Also the shared ray sets and the implicit-function gradient of the root
in float64.  Shared by tests/test_trace_rays_cpu.py and tests/test_gpu_trace_rays.py."""
import functools

import torch

from tests import query_ref as Q


def live_rays(t_near, t_far):
    return torch.isfinite(t_near) & torch.isfinite(t_far) & (t_far > t_near)


def _nodes(o, d, t_near, t_far, steps):
    live = live_rays(t_near, t_far)
    zero = torch.zeros_like(t_near)
    tn, tf = torch.where(live, t_near, zero), torch.where(live, t_far, zero)
    o = torch.where(live[..., None], o, torch.zeros_like(o))
    d = torch.where(live[..., None], d, torch.zeros_like(d))
    dt = (tf - tn) / steps
    return live, tn, tf, o, d, dt


def node_t(tn, tf, dt, i, steps):
    return tn + i * dt if i < steps else tf                 # (two ops: the product is rounded before the sum)


def point(o, d, t):
    return o + t[..., None] * d


def node_sigmas(sigma, o, d, t_near, t_far, steps):
    """[..., steps + 1] densities of every node of every ray (NaN for an empty ray): to choose a level."""
    live, tn, tf, o, d, dt = _nodes(o, d, t_near, t_far, steps)
    s = torch.stack([sigma(point(o, d, node_t(tn, tf, dt, i, steps))) for i in range(steps + 1)], -1)
    return torch.where(live[..., None], s, torch.full_like(s, float("nan")))


def trace(sigma, o, d, t_near, t_far, level, steps, refine):
    """-> dict(hit bool, cell int32, t, lo, hi, s_lo, s_hi): the final bracket next to the kernel's three outputs."""
    live, tn, tf, o, d, dt = _nodes(o, d, t_near, t_far, steps)
    level = torch.as_tensor(level, dtype=o.dtype, device=o.device)
    cell = torch.full(tn.shape, -1, dtype=torch.int32, device=o.device)
    lo, hi, s_lo, s_hi = (torch.zeros_like(tn) for _ in range(4))
    open_ = live.clone()
    for i in range(steps + 1):
        if not bool(open_.any()):
            break
        ti = node_t(tn, tf, dt, i, steps)
        s = sigma(point(o, d, ti))
        inside = s >= level                                   # (False for a NaN)
        take, stay = open_ & inside, open_ & ~inside
        cell = torch.where(take, torch.full_like(cell, i), cell)
        hi, s_hi = torch.where(take, ti, hi), torch.where(take, s, s_hi)
        lo, s_lo = torch.where(stay, ti, lo), torch.where(stay, s, s_lo)
        open_ = stay
    bracket = cell > 0
    for _ in range(refine if bool(bracket.any()) else 0):
        mid = torch.where(bracket, 0.5 * (lo + hi), torch.zeros_like(lo))
        s = sigma(point(o, d, mid))
        inside = s >= level
        take, stay = bracket & inside, bracket & ~inside
        hi, s_hi = torch.where(take, mid, hi), torch.where(take, s, s_hi)
        lo, s_lo = torch.where(stay, mid, lo), torch.where(stay, s, s_lo)
    den = s_hi - s_lo
    sec = lo + (level - s_lo) / den * (hi - lo)
    sec = torch.minimum(torch.maximum(sec, lo), hi)
    t = torch.where(den > 0, sec, hi)
    t = torch.where(bracket, t, torch.where(cell == 0, tn, torch.zeros_like(tn)))
    return dict(hit=cell >= 0, cell=cell, t=t, lo=lo, hi=hi, s_lo=s_lo, s_hi=s_hi)


def bracket_width(t_near, t_far, steps, refine):
    return (t_far - t_near) / (steps * 2.0 ** refine)


# ----------------------------------------------------------------------------- the analytic field sigma = a - b |x|
def sphere_sigma(a, b):
    return lambda x: a - b * x.norm(dim=-1)


def sphere_root(a, b, level, o, d):
    """The first crossing of |o + t d| = (a - level) / b from outside, in closed form (NaN where the ray misses the sphere)."""
    rho = (a - level) / b
    od, dd, oo = (o * d).sum(-1), (d * d).sum(-1), (o * o).sum(-1)
    return (-od - torch.sqrt(od * od - dd * (oo - rho * rho))) / dd


# ----------------------------------------------------------------------------- the oracle's density on given planes
def oracle_sigma(P, pn, axes, box_warp=Q.BOX_WARP, lr_mul=Q.LR_MUL):
    """sigma(x) for x [B, ..., 3] in the dtype of `pn` [B,3,32,H,W] through oracle.sample_from_planes + osg_decoder."""
    from oracle import eg3d_oracle as O
    P = {k: P[k].to(pn.dtype) for k in Q.DEC_KEYS}

    def sigma(x):
        b = pn.shape[0]
        flat = x.reshape(b, -1, 3)
        s = O.osg_decoder(P, O.sample_from_planes(O.plane_axes(axes), pn, flat, box_warp), lr_mul)[1]
        return s.reshape(x.shape[:-1])
    return sigma


def sphere_rays(g, b, r, box_warp=Q.BOX_WARP, dtype=torch.float32):
    """Rays that start on a sphere outside the cube and aim at random points inside it; direction lengths from 0.5 to 2; limits
    from `cam_utils.ray_limits_box`.  -> (o, d, t_near, t_far), [b, r, 3] and [b, r]."""
    from hfa_gp_amd.cam_utils import ray_limits_box
    u = torch.randn(b, r, 3, generator=g, dtype=torch.float64)
    o = 1.2 * box_warp * u / u.norm(dim=-1, keepdim=True)                 # radius 1.2 > sqrt(3) / 2: outside the cube
    aim = (torch.rand(b, r, 3, generator=g, dtype=torch.float64) - 0.5) * (0.9 * box_warp)
    d = aim - o
    d = d / d.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * torch.rand(b, r, 1, generator=g, dtype=torch.float64))
    o, d = o.to(dtype), d.to(dtype)
    tn, tf = ray_limits_box(o, d, box_warp)
    return o, d, tn, tf


@functools.lru_cache(maxsize=None)
def planes_case(hw=(Q.H, Q.W), seed=61):
    """Planes [B,3,32,H,W] for a trace: `query_ref.base_case()`'s at its size (and its decoder always), seeded ones at another."""
    cs = Q.base_case()
    if hw == (Q.H, Q.W):
        return cs["P"], cs["pn"]
    return cs["P"], torch.randn(Q.B, 3, 32, hw[0], hw[1], generator=torch.Generator().manual_seed(seed))


def implicit_grads(sig_of, params, o, d, t_star, mask, c_t, c_p, slope_floor=0.01):
    """float64 gradients of  L = sum c_t t + sum c_p . (o + t d)  w.r.t. `params` (tensors that `sig_of(x)` depends on) and the rays,
    with t the root of sigma(o + t d) = level near the given t_star, by the implicit function theorem:
        dt = -(d sigma|_x + g . (do + t dd)) / (g . d),   g = d sigma / dx at x = o + t_star d
    for the rays of `mask` whose slope passes the floor; every other ray is a constant.  -> (grads of params, d_o, d_d, carries)."""
    o = o.detach().double().requires_grad_(True)
    d = d.detach().double().requires_grad_(True)
    t_star = t_star.detach().double()
    with torch.enable_grad():
        x = o + t_star[..., None] * d
        s = sig_of(x)
        g, = torch.autograd.grad(s.sum(), x, retain_graph=True)
        gd = (g * d.detach()).sum(-1)
        carries = mask & (gd >= slope_floor * g.norm(dim=-1) * d.detach().norm(dim=-1)) & (gd > 0)
        step = (s - s.detach()) / torch.where(carries, gd, torch.ones_like(gd))
        t = t_star - torch.where(carries, step, torch.zeros_like(step))
        pt = torch.where(carries[..., None], o + t[..., None] * d, x.detach())
        loss = (c_t.double() * t).sum() + (c_p.double() * pt).sum()
        grads = torch.autograd.grad(loss, list(params) + [o, d], allow_unused=True)
    grads = [torch.zeros_like(p) if gr is None else gr for gr, p in zip(grads, list(params) + [o, d])]
    cos = gd / (g.norm(dim=-1) * d.detach().norm(dim=-1)).clamp_min(1e-300)
    return grads[:-2], grads[-2], grads[-1], carries, cos
