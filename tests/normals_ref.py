"""Reference for the per-ray surface normals of the ray marcher (csrc/raymarch_normals.hip, `synthesis(normals=True)`), through the
CPU oracle's own functions in whatever dtype it is asked for (float64: the ground truth; float32: the oracle's own error):
coarse pass -> sample_importance -> merge and sort -> sample_from_planes + osg_decoder at all samples ->
torch.autograd.grad(sigma.sum(), xyz) -> n = -g rsqrt(g.g + 1e-12) -> ray_march with n as the colours -> sum_e w_e n_mid_e.
Shared by tests/test_normals_cpu.py and tests/test_gpu_normals.py; the cases are those of tests/test_gpu_camera_grad.py."""
import dataclasses
import functools

import torch

from tests.util import look_at_label, perturb_state, state_cpu

SEED = 4
# (preset, plane axes, plane (H, W), box_warp or None = the preset's): tests/test_gpu_camera_grad.py CASES
CASES = [("tiny64", "eg3d_original", (20, 20), None), ("small128", "eg3d_original", (20, 20), None),
         ("ffhq512_128", "eg3d_original", (20, 20), None), ("small128", "eg3d_fixed", (36, 20), None),
         ("small128", "eg3d_fixed", (24, 24), None), ("small128", "eg3d_original", (20, 36), 0.6),
         ("small128", "eg3d_original", (40, 72), 0.45)]
CASE_IDS = [f"{p}-{a}-{h[0]}x{h[1]}-{b}" for p, a, h, b in CASES]
MAX_EDGE_RAYS_ORACLE = 1     # of 200: the fp32 oracle against the float64 reference
MAX_EDGE_RAYS = 4            # of 200: the device kernel against the float64 reference (tests/test_gpu_camera_grad.py's cap)


def sample_normals(P, cfg, planes, xyz):
    """(sigma [B,M,1], g = d sigma / d xyz [B,M,3], n = -g rsqrt(g.g + 1e-12)) at the points xyz [B,M,3], autograd through the oracle."""
    from oracle import eg3d_oracle as O
    with torch.enable_grad():
        x = xyz.detach().requires_grad_(True)
        _, sigma = O.osg_decoder(P, O.sample_from_planes(O.plane_axes(cfg.plane_axes), planes, x, cfg.box_warp), cfg.decoder_lr_mul)
        g, = torch.autograd.grad(sigma.sum(), x)
    return sigma.detach(), g, -g * torch.rsqrt((g * g).sum(-1, keepdim=True) + 1e-12)


def reference(P, cfg, planes, c, u_strat, u_imp, dtype=torch.float64, fine_depths=None):
    """planes [B,3,32,H,W] (the oracle's layout), c [B,25], u_strat [B,R,Sc,1], u_imp [B*R,Sf] ->
    dict(normal [B,R,3], wsum [B,R], fine_depths [B,R,Sf,1], g [B,R,S,3] per sorted sample) in `dtype`."""
    from oracle import eg3d_oracle as O
    P = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
    planes, c, u_strat, u_imp = (t.detach().to(dtype) for t in (planes, c, u_strat, u_imp))
    res = cfg.neural_rendering_resolution
    axes = O.plane_axes(cfg.plane_axes)
    with torch.no_grad():
        o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:25].reshape(-1, 3, 3), res)
        b, r, _ = o.shape

        def points(depths):
            return (o[:, :, None] + depths * d[:, :, None]).reshape(b, -1, 3)

        d_c = O.sample_stratified(b, r, cfg.ray_start, cfg.ray_end, cfg.depth_resolution, u_strat)
        rgb, sigma = O.osg_decoder(P, O.sample_from_planes(axes, planes, points(d_c), cfg.box_warp), cfg.decoder_lr_mul)
        k = d_c.shape[2]
        _, _, w = O.ray_march(rgb.reshape(b, r, k, -1), sigma.reshape(b, r, k, 1), d_c, cfg.white_back)
        d_f = O.sample_importance(d_c, w, u_imp) if fine_depths is None else fine_depths.detach().to(dtype)
        d_all, _ = torch.sort(torch.cat([d_c, d_f], -2), dim=-2)
    s = d_all.shape[2]
    sigma, g, n = sample_normals(P, cfg, planes, points(d_all))
    with torch.no_grad():
        ncol, _, weights = O.ray_march(n.reshape(b, r, s, 3), sigma.reshape(b, r, s, 1), d_all, False)
        normal = (ncol + 1) / 2                          # ray_march returns sum_e w_e n_mid_e * 2 - 1
        n_mid = (n.reshape(b, r, s, 3)[:, :, :-1] + n.reshape(b, r, s, 3)[:, :, 1:]) / 2
        assert torch.allclose(normal, (weights * n_mid).sum(2), rtol=0, atol=1e-6 if dtype == torch.float32 else 1e-14)
    return dict(normal=normal, wsum=weights.sum(2)[..., 0], fine_depths=d_f, g=g.reshape(b, r, s, 3))


@functools.lru_cache(maxsize=None)
def case(preset, axes="eg3d_original", hw=(20, 20), box_warp=None, seed=SEED):
    """tests/test_gpu_camera_grad.py's set-up: neural_rendering_resolution 10 (100 rays per frame: the last 4-ray block of a
    workgroup is partial), B = 2, random planes, look_at_label cameras."""
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = dataclasses.replace(PRESETS[preset](), neural_rendering_resolution=10, img_resolution=40, plane_axes=axes)
    if box_warp is not None:
        cfg = dataclasses.replace(cfg, box_warp=box_warp)
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False)
    c = look_at_label(torch.tensor([1.3, 1.8]), torch.tensor([1.5, 1.7]))
    g = torch.Generator().manual_seed(seed)
    b, r = 2, cfg.neural_rendering_resolution ** 2
    planes = torch.randn(b, 3, 32, hw[0], hw[1], generator=g)
    us = torch.rand(b, r, cfg.depth_resolution, 1, generator=g)
    ui = torch.rand(b * r, cfg.depth_resolution_importance, generator=g)
    return dict(cfg=cfg, gen=gen, P=state_cpu(gen), c=c, planes=planes, us=us, ui=ui, b=b, r=r)


@functools.lru_cache(maxsize=None)
def case_reference(preset, axes="eg3d_original", hw=(20, 20), box_warp=None, seed=SEED):
    """The float64 reference of a case (computed once and left unchanged)."""
    cs = case(preset, axes, hw, box_warp, seed)
    return reference(cs["P"], cs["cfg"], cs["planes"], cs["c"], cs["us"], cs["ui"])


def rays_beyond(got, ref, what):
    """The project's close_grad bar (atol 2e-5 max(1, max|ref|), rtol 1e-3) per ray over its 3 components -> number of rays beyond
    it; every ray must be finite.  Prints the figures."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    atol, rtol = 2e-5 * max(1.0, float(ref.abs().max())), 1e-3
    err = (got - ref).abs()
    bad = (err > atol + rtol * ref.abs()).flatten(2).any(-1)
    good = ~bad[..., None].expand_as(err)
    worst = float((err / (atol + rtol * ref.abs()))[good].max()) if bool(good.any()) else 0.0
    print(f"{what}: {int(bad.sum())} of {bad.numel()} rays beyond the bar; ref max {float(ref.abs().max()):.3e}, "
          f"max err {float(err.max()):.3e}, worst err / bound of the other rays {worst:.3f}")
    return int(bad.sum())
