"""Reference for the per-sample outputs of ray lists (hfagp_raymarch_rays_samples_fwd / _samples_bwd,
TriPlaneGenerator.render_rays(samples=True)): the oracle's importance_renderer restated so that it RETURNS what it drops — the
depth-sorted sample depths [B,R,S] and MipRayMarcher2's weights [B,R,S-1] — with optional per-ray limits, and the decoder +
compositing at given sorted depths (`weights_at`).  Pure torch on the CPU, fp32 or float64.

The restatement reuses O.sample_from_planes, O.osg_decoder, O.ray_march and O.sample_importance; coarse depths are
O.sample_stratified, or ray_limits_ref.coarse_depths with limits; an empty ray (ray_limits_ref.valid_rays) has zeros in both.
Inputs are test_gpu_render_rays.case's (B = 2, R = 101, 20 x 20 planes of seed 8, MIN_OPACITY asserted there), or
ray_limits_ref.case's for a list with limits.

Matching depths.  The importance depths are an inverse-CDF draw: a last-bit difference of the coarse weights can move a fine sample
into the neighbouring CDF bin, and its depth by a bin's width (~1e-2) instead of a rounding error (~1e-7).  Two references MATCH
on a ray when every fine sample lies in the same bin of the coarse midpoints in both (`fine_bins`); a device result, of which only
the sorted depths are seen, matches the fp32 reference on a ray when all S depths agree within the configuration's TOL_T (`tol_t`).
"""
import functools

import torch

from tests import ray_limits_ref as RL
from tests import test_gpu_render_rays as TR
from tests.test_gpu_geometry_grad import DEC_KEYS

# TOL_T of a configuration is 4 x the largest per-ray deviation of the sorted depths between its fp32 and its float64 reference
# over their matched rays (`tol_t`, from `self_check`: computed where the tests run, on the CPU; the factor 4 allows for the kernel's
# different operation order and its fast exp).  Measured (tests/test_ray_losses_cpu.py::test_reference_depths_self_check prints them):
#   tiny64 5.618e-07, small128 7.045e-07, ffhq512_128 8.579e-07 (depths in [2.25, 3.3]: one to three fp32 ulps),
#   small128 with box limits on the miss list 1.468e-06 (depths up to 5.7) — TOL_T 2.2e-06, 2.8e-06, 3.4e-06 and 5.9e-06;
#   no ray of any of the four is left unmatched.  No deviation may exceed MAX_DEV_T: beyond a few ulps the references are broken.
MAX_DEV_T = 1e-5
MAX_UNMATCHED_REF = 0.01       # of the valid rays: fp32 reference against float64 reference (a condition on the inputs)
MAX_UNMATCHED_DEV = 0.02       # of the valid rays: device against fp32 reference
CONFIGS = (("tiny64", None), ("small128", None), ("ffhq512_128", None), ("small128", "box"))


def to_dtype(P, dtype):
    return {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in P.items()}


def render(P, cfg, planes, o, d, us, ui, lim=None):
    """O.importance_renderer in the dtype of `planes`, returning dict(feat [B,R,32], t [B,R,S] sorted, w [B,R,S-1], wsum [B,R],
    depth [B,R] unclamped, d_c / d_f [B,R,Sc / Sf] by sample id, valid [B,R]).  Depths are constants; the rest hangs on planes, the
    decoder parameters of P, o and d."""
    from oracle import eg3d_oracle as O
    axes = O.plane_axes(cfg.plane_axes)
    b, r, _ = o.shape
    dt = planes.dtype
    us, ui = us.to(dt), ui.to(dt)
    with torch.no_grad():
        if lim is None:
            valid = torch.ones(b, r, dtype=torch.bool)
            d_c = O.sample_stratified(b, r, cfg.ray_start, cfg.ray_end, cfg.depth_resolution, us)
        else:
            tn, tf = (t.detach().to(dt) for t in lim)
            valid = RL.valid_rays(tn, tf)
            d_c = RL.coarse_depths(torch.where(valid, tn, torch.zeros_like(tn)), torch.where(valid, tf, torch.ones_like(tf)), us)

    def run(depths):
        xyz = (o[:, :, None] + depths * d[:, :, None]).reshape(b, -1, 3)
        rgb, sigma = O.osg_decoder(P, O.sample_from_planes(axes, planes, xyz, cfg.box_warp), cfg.decoder_lr_mul)
        k = depths.shape[2]
        return rgb.reshape(b, r, k, -1), sigma.reshape(b, r, k, 1)

    c_c, s_c = run(d_c)
    _, _, w = O.ray_march(c_c, s_c, d_c, cfg.white_back)
    d_f = O.sample_importance(d_c, w, ui)
    c_f, s_f = run(d_f)
    d_all, c_all, s_all = torch.cat([d_c, d_f], -2), torch.cat([c_c, c_f], -2), torch.cat([s_c, s_f], -2)
    _, idx = torch.sort(d_all, dim=-2)
    d_all = torch.gather(d_all, -2, idx)
    c_all = torch.gather(c_all, -2, idx.expand(-1, -1, -1, c_all.shape[-1]))
    s_all = torch.gather(s_all, -2, idx.expand(-1, -1, -1, 1))
    rgb, _, w = O.ray_march(c_all, s_all, d_all, cfg.white_back)
    v = valid[..., None]
    w = torch.where(v, w[..., 0], torch.zeros_like(w[..., 0]))
    t = torch.where(v, d_all[..., 0], torch.zeros_like(d_all[..., 0]))
    t_mid = (t[..., :-1] + t[..., 1:]) / 2
    wsum = w.sum(-1)
    return dict(feat=torch.where(v, rgb, torch.full_like(rgb, 1.0 if cfg.white_back else -1.0)), t=t.detach(), w=w, wsum=wsum,
                depth=(w * t_mid).sum(-1) / wsum, d_c=d_c[..., 0], d_f=d_f[..., 0], valid=valid)


def weights_at(P, cfg, planes, o, d, t_sorted):
    """Decoder and compositing at the given sorted depths [B,R,S], held constant -> weights [B,R,S-1] in the dtype of `planes`;
    differentiable w.r.t. planes, the decoder parameters of P, o and d.  A ray of equal depths (an empty ray's zeros) gets zeros."""
    from oracle import eg3d_oracle as O
    b, r, s = t_sorted.shape
    depths = t_sorted.detach().to(planes.dtype)[..., None]
    xyz = (o[:, :, None] + depths * d[:, :, None]).reshape(b, -1, 3)
    rgb, sigma = O.osg_decoder(P, O.sample_from_planes(O.plane_axes(cfg.plane_axes), planes, xyz, cfg.box_warp), cfg.decoder_lr_mul)
    _, _, w = O.ray_march(rgb.reshape(b, r, s, -1), sigma.reshape(b, r, s, 1), depths, False)
    return w[..., 0]


def fine_bins(out):
    """[B,R,Sf]: the bin of the coarse midpoints every fine sample of `render`'s result lies in."""
    z_mid = 0.5 * (out["d_c"][..., :-1] + out["d_c"][..., 1:])
    return torch.searchsorted(z_mid.contiguous(), out["d_f"].contiguous(), right=True)


def inputs(preset, limits=None, r=TR.R, white_back=False):
    """The case both references and the device run on: test_gpu_render_rays.case, or with limits="box" ray_limits_ref.case on the
    miss list (40 of its 202 rays are empty)."""
    if limits is None:
        return TR.case(preset, white_back=white_back, r=r)
    return RL.case(preset, white_back=white_back, r=r, rays="miss")


@functools.lru_cache(maxsize=None)
def reference(preset, limits=None, r=TR.R, dtype=torch.float32):
    """`render` of the case in `dtype`, no graph: t [B,R,S] and w [B,R,S-1] among its entries."""
    cs = inputs(preset, limits, r)
    o, d = (t.detach().to(dtype) for t in cs["od"])
    with torch.no_grad():
        return render(to_dtype(cs["P"], dtype), cs["cfg"], cs["planes"].detach().to(dtype), o, d, cs["us"], cs["ui"], cs.get("lim"))


@functools.lru_cache(maxsize=None)
def self_check(preset, limits=None, r=TR.R):
    """fp32 reference against float64 reference -> (valid rays, rays left unmatched, largest depth deviation over the matched rays,
    largest |weights_at fp32 - weights_at float64| at the fp32 reference's depths)."""
    a, b = reference(preset, limits, r), reference(preset, limits, r, torch.float64)
    assert torch.equal(a["valid"], b["valid"])
    match = (fine_bins(a) == fine_bins(b)).all(-1) & a["valid"]
    dev_t = (a["t"].double() - b["t"]).abs().amax(-1)
    cs = inputs(preset, limits, r)
    o, d = (t.detach() for t in cs["od"])
    with torch.no_grad():
        w32 = weights_at(to_dtype(cs["P"], torch.float32), cs["cfg"], cs["planes"].detach(), o, d, a["t"])
        w64 = weights_at(to_dtype(cs["P"], torch.float64), cs["cfg"], cs["planes"].detach().double(), o.double(), d.double(), a["t"])
    return int(a["valid"].sum()), int((a["valid"] & ~match).sum()), float(dev_t[match].max()), float((w32.double() - w64).abs().max())


def tol_t(preset, limits=None, r=TR.R):
    return 4 * self_check(preset, limits, r)[2]


def tol_w(preset, limits=None, r=TR.R):
    """4 x the largest |weights_at fp32 - weights_at float64| at the fp32 reference's depths, not below the forward bar."""
    return max(TR.ATOL_FWD, 4 * self_check(preset, limits, r)[3])


def weights64(cs, t_sorted, grad=False):
    """float64 `weights_at` of a case at the given depths (a device's own) -> (w, leaves): with `grad` the leaves — planes, the four
    decoder parameters, origins, directions — require grad and w carries the graph."""
    P = to_dtype(cs["P"], torch.float64)
    leaves = [cs["planes"].detach().double()] + [P[k] for k in DEC_KEYS] + [t.detach().double() for t in cs["od"]]
    if grad:
        leaves = [t.requires_grad_(True) for t in leaves]
        for k, t in zip(DEC_KEYS, leaves[1:5]):
            P[k] = t
    with torch.set_grad_enabled(grad):
        w = weights_at(P, cs["cfg"], leaves[0], leaves[5], leaves[6], t_sorted.detach().cpu())
    return w, leaves


def weight_grads(cs, t_sorted, g_w):
    """float64 autograd of sum(g_w * w) through `weights_at` at the given depths -> (d planes, (d decoder parameters), [B,R,6])."""
    w, leaves = weights64(cs, t_sorted, grad=True)
    grads = torch.autograd.grad((w * g_w.detach().cpu().double()).sum(), leaves)
    return grads[0].float(), tuple(g.float() for g in grads[1:5]), torch.cat(grads[5:], -1).float()
