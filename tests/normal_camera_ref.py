"""Reference for the camera gradient of the per-ray surface normals (csrc/raymarch_normals_camera.hip,
`synthesis(normal_camera_grad=True)`).

`reference` is float64 autograd: the body of normal_grad_ref.reference with the label requiring grad and the rays taken from the
oracle's ray sampler, so the gradient reaches the label through the sample positions alone (the sorted depths are an input and
carry none, as everywhere in the renderer).  `closed_form` is normal_grad_ref.closed_form extended by the positional derivative
the kernel computes (include/hfagp.h, hfagp_raymarch_normals_bwd_camera): gather_position_grad of dF plus the mixed second
derivative of the bilinear weights, then camera_ref.ray_sums and camera_ref.ray_setup_adjoint.
Shared by tests/test_normal_camera_cpu.py and tests/test_gpu_normal_camera_grad.py; the cases and the edge mask are those of
tests/normal_grad_ref.py (masked_case: EDGE 1e-4, MIN_KEPT 0.9)."""
import functools

import torch

from tests import camera_ref as CR
from tests import normal_grad_ref as G

ZERO_COLUMNS = [k for k in range(25) if k not in CR.NONZERO_COLUMNS]


def reference(P, cfg, planes, c, depths, g_hat, dtype=torch.float64):
    """planes [B,3,32,H,W] (the oracle's layout), c [B,25], depths [B,R,S,1] sorted, g_hat [B,R,3] = dL/dN ->
    (dL/dc [B,25], dL/dx [B,R,S,3]) in `dtype`."""
    from oracle import eg3d_oracle as O
    P = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
    planes, c, depths, g_hat = (t.detach().to(dtype) for t in (planes, c, depths, g_hat))
    with torch.enable_grad():
        c = c.clone().requires_grad_(True)
        o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:25].reshape(-1, 3, 3), cfg.neural_rendering_resolution)
        b, r, s, _ = depths.shape
        x = (o[:, :, None] + depths * d[:, :, None]).reshape(b, r * s, 3)
        _, sigma = O.osg_decoder(P, G.gather_from_planes(cfg.plane_axes, planes, x, cfg.box_warp), cfg.decoder_lr_mul)
        g, = torch.autograd.grad(sigma.sum(), x, create_graph=True)
        n = -g * torch.rsqrt((g * g).sum(-1, keepdim=True) + 1e-12)
        ncol, _, _ = O.ray_march(n.reshape(b, r, s, 3), sigma.reshape(b, r, s, 1), depths, False)
        normal = (ncol + 1) / 2                                   # ray_march returns sum_e w_e n_mid_e * 2 - 1
        dc, dx = torch.autograd.grad((normal * g_hat).sum(), [c, x])
    return dc, dx.reshape(b, r, s, 3)


def closed_form(P, cfg, planes, c, depths, g_hat, dtype=torch.float64, parts=False):
    """The same by the formulas of include/hfagp.h, no autograd: what the kernel computes -> (dL/dc, dL/dx); with `parts` also the
    per-ray records ray_grad [B,R,6]."""
    Pd, planes, depths, g_hat, pts, (b, r, s) = G._setup(P, cfg, planes, c, depths, g_hat, dtype)
    c = c.detach().to(dtype)
    _, npl, ch, h, w = planes.shape
    lr = cfg.decoder_lr_mul
    w0 = Pd[G.DEC_KEYS[0]] * (lr / 32 ** 0.5)
    b0 = Pd[G.DEC_KEYS[1]] * lr
    wsig = Pd[G.DEC_KEYS[2]][0] * (lr / 64 ** 0.5)
    cs_ = 2.0 / cfg.box_warp
    m = r * s
    proj = G._project(cfg.plane_axes, pts, cfg.box_warp)
    ix, iy = G._pixels(proj, h, w)
    x0, y0 = ix.floor(), iy.floor()
    fx, fy = ix - x0, iy - y0
    flat = planes.reshape(b, npl, ch, h * w)
    taps = []                         # (idx, w, dw/dgx, dw/dgy, d2w/dgx dgy) for nw, ne, sw, se
    for dy, wy, dwy in ((0, 1 - fy, -1.0), (1, fy, 1.0)):
        for dx, wx, dwx in ((0, 1 - fx, -1.0), (1, fx, 1.0)):
            xi, yi = x0 + dx, y0 + dy
            ok = ((xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)).to(dtype)
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()
            taps.append((idx, wy * wx * ok, dwx * wy * ok * (w / 2), dwy * wx * ok * (h / 2), dwx * dwy * ok * (w / 2) * (h / 2)))
    tex = [torch.gather(flat, 3, t[0][:, :, None, :].expand(-1, -1, ch, -1)) for t in taps]
    F = sum(tx * t[1][:, :, None] for tx, t in zip(tex, taps)).sum(1) / 3
    hp = torch.einsum("hc,bcm->bhm", w0, F) + b0[None, :, None]
    sg = torch.sigmoid(hp)
    sigma = torch.einsum("h,bhm->bm", wsig, torch.nn.functional.softplus(hp)) + Pd[G.DEC_KEYS[3]][0] * lr
    dH = wsig[None, :, None] * sg
    a = torch.einsum("hc,bhm->bcm", w0, dH)
    eye = torch.eye(3, dtype=dtype)[None]
    route = G._project(cfg.plane_axes, eye, 2.0)[0]                # [3 planes, 3 axes, 2]: d (gx, gy) / d q_axis
    Pk = [torch.einsum("bcm,bpcm->bpm", a, tx) for tx in tex]
    dix = sum(pk * t[2] for pk, t in zip(Pk, taps)) / 3
    diy = sum(pk * t[3] for pk, t in zip(Pk, taps)) / 3
    gq = torch.einsum("bpm,pk->bmk", dix, route[..., 0]) + torch.einsum("bpm,pk->bmk", diy, route[..., 1])
    g = cs_ * gq
    rr = torch.sqrt((g * g).sum(-1, keepdim=True) + 1e-12)
    n = (-g / rr).reshape(b, r, s, 3)
    sig = sigma.reshape(b, r, s)
    t = depths[..., 0]
    dl = t[..., 1:] - t[..., :-1]
    sbar = (sig[..., :-1] + sig[..., 1:]) / 2 - 1
    al = 1 - torch.exp(-torch.nn.functional.softplus(sbar) * dl)
    sh = 1 - al + 1e-10
    T = torch.cat([torch.ones_like(al[..., :1]), torch.cumprod(sh, -1)[..., :-1]], -1)
    wgt = al * T
    zero = torch.zeros_like(wgt[..., :1])
    om = (torch.cat([zero, wgt], -1) + torch.cat([wgt, zero], -1)) / 2
    gn = (n * g_hat[:, :, None]).sum(-1)
    Gm = (gn[..., :-1] + gn[..., 1:]) / 2
    gw = Gm * wgt
    suf = gw.sum(-1, keepdim=True) - torch.cumsum(gw, -1)
    dsb = (Gm * T - suf / sh) * dl * (1 - al) * torch.sigmoid(sbar)
    dsig = ((torch.cat([zero, dsb], -1) + torch.cat([dsb, zero], -1)) / 2).reshape(b, m)
    nn_ = n.reshape(b, m, 3)
    gh = g_hat[:, :, None].expand(-1, -1, s, -1).reshape(b, m, 3)
    gamma = -(om.reshape(b, m, 1) / rr) * (gh - nn_ * (nn_ * gh).sum(-1, keepdim=True))
    gmq = cs_ * gamma
    cx = torch.einsum("bmk,pk->bpm", gmq, route[..., 0])           # the component of gamma_q each plane's gx / gy carries
    cy = torch.einsum("bmk,pk->bpm", gmq, route[..., 1])
    dws = [cx * tp[2] + cy * tp[3] for tp in taps]
    u = sum(tx * dw[:, :, None] for tx, dw in zip(tex, dws)).sum(1) / 3
    v = torch.einsum("hc,bcm->bhm", w0, u)
    e = dH * (1 - sg) * v
    xx = dH * dsig[:, None] + e
    dF = torch.einsum("hc,bhm->bcm", w0, xx)
    # the positional derivative: gather_position_grad of dF, and the mixed second derivative of the tap weights with a
    Qk = [torch.einsum("bcm,bpcm->bpm", dF, tx) for tx in tex]
    pgx = sum(qk * tp[2] for qk, tp in zip(Qk, taps)) / 3
    pgy = sum(qk * tp[3] for qk, tp in zip(Qk, taps)) / 3
    mm = sum(pk * tp[4] for pk, tp in zip(Pk, taps)) / 3
    pgx = pgx + mm * cy
    pgy = pgy + mm * cx
    dq = torch.einsum("bpm,pk->bmk", pgx, route[..., 0]) + torch.einsum("bpm,pk->bmk", pgy, route[..., 1])
    dx = (cs_ * dq).reshape(b, r, s, 3)
    ray_grad = CR.ray_sums(dx, t)
    dc = CR.ray_setup_adjoint(c, cfg.neural_rendering_resolution, ray_grad)
    return (dc, dx, ray_grad) if parts else (dc, dx)


def ray_records(dx, depths):
    """dL/dx [B,R,S,3] and the depths [B,R,S,1] -> ray_grad [B,R,6] (camera_ref.ray_sums)."""
    return CR.ray_sums(dx, depths[..., 0].to(dx.dtype))


@functools.lru_cache(maxsize=None)
def oracle_rho(preset, axes="eg3d_original", hw=(20, 20), box_warp=None):
    """rho of the fp32 reference against the float64 one under the mask, with the oracle's own depths (once per case):
    the worst normal_grad_ref.bar_ratio over dL/dx and dL/dc."""
    cs, depths, g_hat, _ = G.masked_case(preset, axes, hw, box_warp)
    dc, dx = reference(cs["P"], cs["cfg"], cs["planes"], cs["c"], depths, g_hat)
    dc32, dx32 = reference(cs["P"], cs["cfg"], cs["planes"], cs["c"], depths, g_hat, dtype=torch.float32)
    r_x, r_c = G.bar_ratio(dx32, dx), G.bar_ratio(dc32, dc)
    print(f"{preset}/{axes}/{hw}/{box_warp}: fp32 reference: d x {r_x:.3f}, d c {r_c:.3f}; ref max |d c| {float(dc.abs().max()):.3e}")
    return max(r_x, r_c)
