"""Reference for surface normals along ray lists (hfagp_raymarch_rays_normals*, `render_rays(normals=, normal_grad=,
normal_ray_grad=)`): the bodies of normals_ref.reference, normal_grad_ref.reference / edge_mask and normal_camera_ref.reference with
the sample points o + t d built from given (o, d) instead of the oracle's ray sampler, and with the coarse depths of
ray_limits_ref.coarse_depths when the list carries per-ray limits.  Pure torch on the CPU; float64 unless asked otherwise.

An EMPTY ray (limits not finite, or far <= near) has normal 0, takes no part in any gradient (its upstream gradient is dropped and
its depths — whatever the caller read from an unwritten state — are replaced by a placeholder), and is out of the edge mask.
The backward references take the sorted depths as an INPUT (GPU tests pass the device's own, read from `state`); the rays' gradient
is autograd w.r.t. o and d with those depths fixed.
Shared by tests/test_rays_normals_cpu.py and tests/test_gpu_rays_normals.py."""
import dataclasses
import functools

import torch

from tests import normal_grad_ref as G
from tests import normals_ref as N
from tests import ray_limits_ref as RL
from tests.util import perturb_state, state_cpu

B, R = RL.B, RL.R                      # 2 x 101: the last 4-ray block of a workgroup is partial
PLANE_SEED = 8                         # the planes and uniforms of the cases (the caps below are conditions on it)


def points(o, d, depths):
    """o, d [B,R,3], depths [B,R,S,1] -> the sample points [B,R*S,3]."""
    return (o[:, :, None] + depths * d[:, :, None]).reshape(o.shape[0], -1, 3)


def _cast(P, dtype, *tensors):
    P = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
    return (P,) + tuple(t.detach().to(dtype) for t in tensors)


def reference(P, cfg, planes, o, d, u_strat, u_imp, dtype=torch.float64, limits=None, fine_depths=None):
    """planes [B,3,32,H,W] (the oracle's layout), o / d [B,R,3], u_strat [B,R,Sc,1], u_imp [B*R,Sf], limits None or (t_near, t_far)
    [B,R] -> dict(normal [B,R,3], wsum [B,R], fine_depths [B,R,Sf,1], depths [B,R,S,1] sorted, g [B,R,S,3], valid [B,R]) in `dtype`."""
    from oracle import eg3d_oracle as O
    P, planes, o, d, u_strat, u_imp = _cast(P, dtype, planes, o, d, u_strat, u_imp)
    axes = O.plane_axes(cfg.plane_axes)
    b, r, _ = o.shape
    with torch.no_grad():
        if limits is None:
            valid = torch.ones(b, r, dtype=torch.bool)
            d_c = O.sample_stratified(b, r, cfg.ray_start, cfg.ray_end, cfg.depth_resolution, u_strat)
        else:
            t_near, t_far = (t.detach().to(dtype) for t in limits)
            valid = RL.valid_rays(t_near, t_far)
            # (an empty ray is computed on a placeholder interval and its outputs are replaced below)
            d_c = RL.coarse_depths(torch.where(valid, t_near, torch.zeros_like(t_near)),
                                   torch.where(valid, t_far, torch.ones_like(t_far)), u_strat)
        rgb, sigma = O.osg_decoder(P, O.sample_from_planes(axes, planes, points(o, d, d_c), cfg.box_warp), cfg.decoder_lr_mul)
        k = d_c.shape[2]
        _, _, w = O.ray_march(rgb.reshape(b, r, k, -1), sigma.reshape(b, r, k, 1), d_c, cfg.white_back)
        d_f = O.sample_importance(d_c, w, u_imp) if fine_depths is None else fine_depths.detach().to(dtype)
        d_all, _ = torch.sort(torch.cat([d_c, d_f], -2), dim=-2)
    s = d_all.shape[2]
    sigma, g, n = N.sample_normals(P, cfg, planes, points(o, d, d_all))
    with torch.no_grad():
        ncol, _, weights = O.ray_march(n.reshape(b, r, s, 3), sigma.reshape(b, r, s, 1), d_all, False)
        normal = (ncol + 1) / 2                          # ray_march returns sum_e w_e n_mid_e * 2 - 1
        normal = torch.where(valid[..., None], normal, torch.zeros_like(normal))
        wsum = torch.where(valid, weights.sum(2)[..., 0], torch.zeros_like(weights.sum(2)[..., 0]))
    return dict(normal=normal, wsum=wsum, fine_depths=d_f, depths=d_all, g=g.reshape(b, r, s, 3), valid=valid)


def _fixed_depths(depths, valid):
    """The depths with those of the empty rays (unwritten state: anything) replaced by a placeholder interval."""
    if valid is None:
        return depths
    s = depths.shape[2]
    place = torch.linspace(1.0, 2.0, s, dtype=depths.dtype).reshape(1, 1, s, 1).expand_as(depths)
    return torch.where(valid[..., None, None], depths, place)


def edge_mask(cfg, hw, o, d, depths, valid=None):
    """normal_grad_ref.edge_mask for given rays: [B,R] bool (float64), the valid rays none of whose samples has a pixel coordinate
    within G.EDGE of an integer on any plane."""
    o, d, depths = o.detach().double(), d.detach().double(), _fixed_depths(depths.double(), valid)
    b, r, s, _ = depths.shape
    ix, iy = G._pixels(G._project(cfg.plane_axes, points(o, d, depths), cfg.box_warp), hw[0], hw[1])
    near = ((ix - ix.round()).abs() < G.EDGE) | ((iy - iy.round()).abs() < G.EDGE)       # [B,3,R*S]
    mask = ~near.reshape(b, 3, r, s).any(3).any(1)
    return mask if valid is None else mask & valid


def kept(mask, valid=None):
    """The fraction of the valid rays the edge mask keeps."""
    n = mask.numel() if valid is None else int(valid.sum())
    return float(mask.sum()) / max(n, 1)


def grad_reference(P, cfg, planes, o, d, depths, g_hat, dtype=torch.float64, valid=None):
    """planes [B,3,32,H,W], o / d [B,R,3], depths [B,R,S,1] sorted, g_hat [B,R,3] = dL/dN, valid None or [B,R] bool ->
    dict(normal [B,R,3], g [B,R,S,3], planes = dL/dplanes, dec = the four decoder gradients (G.DEC_KEYS order),
    rays [B,R,6] = (dL/d origin, dL/d direction) with the depths held fixed) in `dtype`."""
    from oracle import eg3d_oracle as O
    P, planes, o, d, depths, g_hat = _cast(P, dtype, planes, o, d, depths, g_hat)
    depths = _fixed_depths(depths, valid)
    if valid is not None:
        g_hat = torch.where(valid[..., None], g_hat, torch.zeros_like(g_hat))
    b, r, s, _ = depths.shape
    with torch.enable_grad():
        leaves = [planes] + [P[k] for k in G.DEC_KEYS] + [o, d]
        for t in leaves:
            t.requires_grad_(True)
        x = points(o, d, depths)
        _, sigma = O.osg_decoder(P, G.gather_from_planes(cfg.plane_axes, planes, x, cfg.box_warp), cfg.decoder_lr_mul)
        g, = torch.autograd.grad(sigma.sum(), x, create_graph=True)
        n = -g * torch.rsqrt((g * g).sum(-1, keepdim=True) + 1e-12)
        ncol, _, _ = O.ray_march(n.reshape(b, r, s, 3), sigma.reshape(b, r, s, 1), depths, False)
        normal = (ncol + 1) / 2                                   # ray_march returns sum_e w_e n_mid_e * 2 - 1
        grads = torch.autograd.grad((normal * g_hat).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, leaves)]
    normal = normal.detach()
    if valid is not None:
        normal = torch.where(valid[..., None], normal, torch.zeros_like(normal))
    return dict(normal=normal, g=g.detach().reshape(b, r, s, 3), planes=grads[0], dec=tuple(grads[1:5]),
                rays=torch.cat(grads[5:], -1))


def upstream(b, r, seed=G.G_SEED):
    """G^ [B,R,3] (random, seeded); the tests multiply it by the edge mask."""
    return torch.randn(b, r, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ----------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def case(preset, axes="eg3d_original", hw=(20, 20), rays="r27", limits=None, r=R, seed=PLANE_SEED):
    """The first r rays of a list of ray_limits_ref.LISTS ("r27": the 2 x 101 list of tests/test_gpu_render_rays.py, directions not
    of unit length; "mixed" / "miss": ray_limits_ref's), random planes [B,3,32,H,W] and uniforms of `seed`,
    perturb_state(TriPlaneGenerator(cfg, seed=0)).  limits: None = the config's interval, "box" = cam_utils.ray_limits_box at
    cfg.box_warp."""
    from hfa_gp_amd.cam_utils import ray_limits_box
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = dataclasses.replace(PRESETS[preset](), plane_axes=axes)
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False)
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(B, 3, 32, hw[0], hw[1], generator=g)
    us = torch.rand(B, R, cfg.depth_resolution, 1, generator=g)[:, :r].contiguous()
    ui = torch.rand(B, R, cfg.depth_resolution_importance, generator=g)[:, :r].reshape(B * r, -1).contiguous()
    o, d = (t[:, :r].contiguous() for t in RL.LISTS[rays]())
    lim = ray_limits_box(o, d, cfg.box_warp) if limits == "box" else None
    return dict(cfg=cfg, gen=gen, P=state_cpu(gen), planes=planes, us=us, ui=ui, o=o, d=d, lim=lim, b=B, r=r, hw=hw)


@functools.lru_cache(maxsize=None)
def case_reference(*key, dtype=torch.float64):
    """The reference of a case (computed once and left unchanged)."""
    cs = case(*key)
    return reference(cs["P"], cs["cfg"], cs["planes"], cs["o"], cs["d"], cs["us"], cs["ui"], dtype=dtype, limits=cs["lim"])


def masked_upstream(cs, depths, valid=None):
    """(G^ times the edge mask [B,R,3] float64, mask) for the case's rays at the given sorted depths; asserts G.MIN_KEPT."""
    mask = edge_mask(cs["cfg"], cs["hw"], cs["o"], cs["d"], depths, valid)
    frac = kept(mask, valid)
    assert frac >= G.MIN_KEPT, f"only {int(mask.sum())} rays kept ({frac:.3f} of the valid ones)"
    return upstream(cs["b"], cs["r"]) * mask[..., None], mask
