"""Reference for the gradient of the per-ray surface normals (csrc/raymarch_normals_bwd.hip, `synthesis(normal_grad=True)`).

PyTorch cannot differentiate grid_sample's backward ("derivative for aten::grid_sampler_2d_backward is not implemented"), so the
bilinear gather is written with index arithmetic here — `sample_from_planes` of the oracle with floor, four torch.gather calls,
zeros padding and align_corners=False — and everything else is the oracle's own: osg_decoder, autograd.grad(sigma.sum(), x,
create_graph=True), n = -g rsqrt(g.g + 1e-12), ray_march with n as the colours, autograd.grad((N . G^).sum(), [planes, decoder]).
The sorted sample depths are an INPUT (GPU tests pass the device's own, so importance sampling drops out of the comparison).

The gradient of sigma jumps across texel edges: a sample whose pixel coordinate rounds to the other side in fp32 moves its ray's
whole contribution.  `reference` therefore returns a ray mask (float64: no sample of the ray has a pixel coordinate, on any plane,
within EDGE of an integer); the tests multiply G^ by it.

`closed_form` is the adjoint as the kernel computes it (include/hfagp.h, hfagp_raymarch_normals_bwd), written out in torch.
Shared by tests/test_normal_grad_cpu.py and tests/test_gpu_normal_grad.py; the cases are those of tests/normals_ref.py."""
import functools

import torch

from tests import normals_ref as N

DEC_KEYS = ("decoder.net.0.weight", "decoder.net.0.bias", "decoder.net.2.weight", "decoder.net.2.bias")
EDGE = 1e-4                 # pixels
MIN_KEPT = 0.9              # of the rays, in every case
G_SEED = 11


def _project(axes_name, coords, box_warp):
    """coords [B,M,3] -> the three planes' grid coordinates [B,3,M,2], as oracle.sample_from_planes projects them."""
    from oracle import eg3d_oracle as O
    inv = torch.linalg.inv(O.plane_axes(axes_name)).to(coords.dtype)                 # [3,3,3]
    return torch.einsum("bmk,pkj->bpmj", (2.0 / box_warp) * coords, inv)[..., :2]


def _pixels(proj, h, w):
    return (proj[..., 0] + 1) * (w / 2) - 0.5, (proj[..., 1] + 1) * (h / 2) - 0.5


def gather_from_planes(axes_name, planes, coords, box_warp):
    """oracle.sample_from_planes (planes [B,3,C,H,W], coords [B,M,3] -> [B,3,M,C]) by index arithmetic: differentiable twice."""
    b, npl, c, h, w = planes.shape
    m = coords.shape[1]
    ix, iy = _pixels(_project(axes_name, coords, box_warp), h, w)                    # [B,3,M]
    x0, y0 = ix.detach().floor(), iy.detach().floor()
    fx, fy = ix - x0, iy - y0
    flat = planes.reshape(b, npl, c, h * w)
    out = 0
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()
            vals = torch.gather(flat, 3, idx[:, :, None, :].expand(-1, -1, c, -1))   # [B,3,C,M]
            out = out + vals * (wy * wx * ok.to(planes.dtype))[:, :, None, :]
    return out.permute(0, 1, 3, 2)


def edge_mask(cfg, hw, c, depths):
    """[B,R] bool (float64): the rays none of whose samples has a pixel coordinate within EDGE of an integer on any plane."""
    from oracle import eg3d_oracle as O
    c, depths = c.double(), depths.double()
    o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:25].reshape(-1, 3, 3), cfg.neural_rendering_resolution)
    b, r, s, _ = depths.shape
    pts = (o[:, :, None] + depths * d[:, :, None]).reshape(b, r * s, 3)
    ix, iy = _pixels(_project(cfg.plane_axes, pts, cfg.box_warp), hw[0], hw[1])
    near = ((ix - ix.round()).abs() < EDGE) | ((iy - iy.round()).abs() < EDGE)       # [B,3,R*S]
    return ~near.reshape(b, 3, r, s).any(3).any(1)


def _setup(P, cfg, planes, c, depths, g_hat, dtype):
    from oracle import eg3d_oracle as O
    P = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
    planes, c, depths, g_hat = (t.detach().to(dtype) for t in (planes, c, depths, g_hat))
    o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:25].reshape(-1, 3, 3), cfg.neural_rendering_resolution)
    b, r, s, _ = depths.shape
    pts = (o[:, :, None] + depths * d[:, :, None]).reshape(b, r * s, 3)
    return P, planes, depths, g_hat, pts, (b, r, s)


def reference(P, cfg, planes, c, depths, g_hat, dtype=torch.float64):
    """planes [B,3,32,H,W] (the oracle's layout), c [B,25], depths [B,R,S,1] sorted, g_hat [B,R,3] = dL/dN ->
    dict(normal [B,R,3], g [B,R,S,3], planes = dL/dplanes, dec = the four decoder gradients (DEC_KEYS order)) in `dtype`."""
    from oracle import eg3d_oracle as O
    P, planes, depths, g_hat, pts, (b, r, s) = _setup(P, cfg, planes, c, depths, g_hat, dtype)
    with torch.enable_grad():
        planes.requires_grad_(True)
        for k in DEC_KEYS:
            P[k].requires_grad_(True)
        x = pts.requires_grad_(True)
        _, sigma = O.osg_decoder(P, gather_from_planes(cfg.plane_axes, planes, x, cfg.box_warp), cfg.decoder_lr_mul)
        g, = torch.autograd.grad(sigma.sum(), x, create_graph=True)
        n = -g * torch.rsqrt((g * g).sum(-1, keepdim=True) + 1e-12)
        ncol, _, _ = O.ray_march(n.reshape(b, r, s, 3), sigma.reshape(b, r, s, 1), depths, False)
        normal = (ncol + 1) / 2                                   # ray_march returns sum_e w_e n_mid_e * 2 - 1
        grads = torch.autograd.grad((normal * g_hat).sum(), [planes] + [P[k] for k in DEC_KEYS], allow_unused=True)
    grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, [planes] + [P[k] for k in DEC_KEYS])]
    return dict(normal=normal.detach(), g=g.detach().reshape(b, r, s, 3), planes=grads[0], dec=tuple(grads[1:]))


def closed_form(P, cfg, planes, c, depths, g_hat, dtype=torch.float64):
    """The same gradients by the formulas of include/hfagp.h (hfagp_raymarch_normals_bwd), no autograd: what the kernel computes."""
    P, planes, depths, g_hat, pts, (b, r, s) = _setup(P, cfg, planes, c, depths, g_hat, dtype)
    _, npl, ch, h, w = planes.shape
    lr = cfg.decoder_lr_mul
    w0 = P[DEC_KEYS[0]] * (lr / 32 ** 0.5)                                        # W0' [64,32]
    b0 = P[DEC_KEYS[1]] * lr
    wsig = P[DEC_KEYS[2]][0] * (lr / 64 ** 0.5)                                   # [64]
    cs_ = 2.0 / cfg.box_warp
    m = r * s
    proj = _project(cfg.plane_axes, pts, cfg.box_warp)                             # [B,3,M,2]
    ix, iy = _pixels(proj, h, w)
    x0, y0 = ix.floor(), iy.floor()
    fx, fy = ix - x0, iy - y0
    flat = planes.reshape(b, npl, ch, h * w)
    taps = []                                                                      # (idx [B,3,M], w, dw/dix, dw/diy) for nw, ne, sw, se
    for dy, wy, dwy in ((0, 1 - fy, -1.0), (1, fy, 1.0)):
        for dx, wx, dwx in ((0, 1 - fx, -1.0), (1, fx, 1.0)):
            xi, yi = x0 + dx, y0 + dy
            ok = ((xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)).to(dtype)
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()
            taps.append((idx, wy * wx * ok, dwx * wy * ok * (w / 2), dwy * wx * ok * (h / 2)))

    def texels(idx):
        return torch.gather(flat, 3, idx[:, :, None, :].expand(-1, -1, ch, -1))    # [B,3,C,M]

    tex = [texels(t[0]) for t in taps]
    F = sum(tx * t[1][:, :, None] for tx, t in zip(tex, taps)).sum(1) / 3          # [B,C,M]
    hp = torch.einsum("hc,bcm->bhm", w0, F) + b0[None, :, None]
    sg = torch.sigmoid(hp)
    sp = torch.nn.functional.softplus(hp)
    sigma = torch.einsum("h,bhm->bm", wsig, sp) + P[DEC_KEYS[3]][0] * lr
    dH = wsig[None, :, None] * sg
    a = torch.einsum("hc,bhm->bcm", w0, dH)                                        # d sigma / dF [B,C,M]
    # which world axis each plane's (gx, gy) reads: d proj / d q, from the projection itself
    eye = torch.eye(3, dtype=dtype)[None]
    route = _project(cfg.plane_axes, eye, 2.0)[0]                                  # [3 planes, 3 axes, 2]: d (gx, gy) / d q_axis
    # g = coord_scale J^T a
    Pk = [torch.einsum("bcm,bpcm->bpm", a, tx) for tx in tex]
    dix = sum(pk * t[2] for pk, t in zip(Pk, taps)) / 3                            # [B,3,M]  d sigma / d gx
    diy = sum(pk * t[3] for pk, t in zip(Pk, taps)) / 3
    gq = torch.einsum("bpm,pk->bmk", dix, route[..., 0]) + torch.einsum("bpm,pk->bmk", diy, route[..., 1])
    g = cs_ * gq
    rr = torch.sqrt((g * g).sum(-1, keepdim=True) + 1e-12)
    n = (-g / rr).reshape(b, r, s, 3)
    # compositing (ray_march) and its adjoint with G_e = G^ . (n_e + n_{e+1}) / 2
    sig = sigma.reshape(b, r, s)
    t = depths[..., 0]
    dl = t[..., 1:] - t[..., :-1]
    sbar = (sig[..., :-1] + sig[..., 1:]) / 2 - 1
    al = 1 - torch.exp(-torch.nn.functional.softplus(sbar) * dl)
    sh = 1 - al + 1e-10
    T = torch.cat([torch.ones_like(al[..., :1]), torch.cumprod(sh, -1)[..., :-1]], -1)
    wgt = al * T
    zero = torch.zeros_like(wgt[..., :1])
    om = (torch.cat([zero, wgt], -1) + torch.cat([wgt, zero], -1)) / 2              # [B,R,S]
    normal = (om[..., None] * n).sum(2)
    gn = (n * g_hat[:, :, None]).sum(-1)
    G = (gn[..., :-1] + gn[..., 1:]) / 2
    gw = G * wgt
    suf = gw.sum(-1, keepdim=True) - torch.cumsum(gw, -1)
    dsb = (G * T - suf / sh) * dl * (1 - al) * torch.sigmoid(sbar)
    dsig = ((torch.cat([zero, dsb], -1) + torch.cat([dsb, zero], -1)) / 2).reshape(b, m)
    # through the normals
    nn_ = n.reshape(b, m, 3)
    gh = g_hat[:, :, None].expand(-1, -1, s, -1).reshape(b, m, 3)
    gamma = -(om.reshape(b, m, 1) / rr) * (gh - nn_ * (nn_ * gh).sum(-1, keepdim=True))
    gmq = cs_ * gamma                                                              # [B,M,3]
    cx = torch.einsum("bmk,pk->bpm", gmq, route[..., 0])                           # the component each plane's gx / gy carries
    cy = torch.einsum("bmk,pk->bpm", gmq, route[..., 1])
    dws = [cx * tp[2] + cy * tp[3] for tp in taps]                                 # w'_k [B,3,M]
    u = sum(tx * dw[:, :, None] for tx, dw in zip(tex, dws)).sum(1) / 3            # [B,C,M]
    v = torch.einsum("hc,bcm->bhm", w0, u)
    e = dH * (1 - sg) * v
    xx = dH * dsig[:, None] + e
    dF = torch.einsum("hc,bhm->bcm", w0, xx)
    d_flat = torch.zeros_like(flat)
    for tp, dw in zip(taps, dws):
        val = (tp[1][:, :, None] * dF[:, None] + dw[:, :, None] * a[:, None]) / 3   # [B,3,C,M]
        d_flat.scatter_add_(3, tp[0][:, :, None, :].expand(-1, -1, ch, -1), val)
    d_w0 = (torch.einsum("bhm,bcm->hc", xx, F) + torch.einsum("bhm,bcm->hc", dH, u)) * (lr / 32 ** 0.5)
    d_b0 = xx.sum((0, 2)) * lr
    d_w1 = torch.zeros_like(P[DEC_KEYS[2]])
    d_w1[0] = (torch.einsum("bm,bhm->h", dsig, sp) + (sg * v).sum((0, 2))) * (lr / 64 ** 0.5)
    d_b1 = torch.zeros_like(P[DEC_KEYS[3]])
    d_b1[0] = dsig.sum() * lr
    return dict(normal=normal, g=g.reshape(b, r, s, 3), planes=d_flat.reshape(planes.shape), dec=(d_w0, d_b0, d_w1, d_b1))


# ----------------------------------------------------------------------------- the cases of tests/normals_ref.py
@functools.lru_cache(maxsize=None)
def oracle_depths(preset, axes="eg3d_original", hw=(20, 20), box_warp=None):
    """The oracle's own sorted depths [B,R,S,1] of a case in float64 (coarse + its importance draw)."""
    from oracle import eg3d_oracle as O
    cs, ref = N.case(preset, axes, hw, box_warp), N.case_reference(preset, axes, hw, box_warp)
    cfg = cs["cfg"]
    d_c = O.sample_stratified(cs["b"], cs["r"], cfg.ray_start, cfg.ray_end, cfg.depth_resolution, cs["us"].double())
    return torch.sort(torch.cat([d_c, ref["fine_depths"]], -2), dim=-2).values


def upstream(cs):
    """G^ [B,R,3] of a case (random, seeded); the tests multiply it by the edge mask."""
    return torch.randn(cs["b"], cs["r"], 3, generator=torch.Generator().manual_seed(G_SEED), dtype=torch.float64)


def bar_ratio(got, ref):
    """Worst err / (2e-5 max(1, max|ref|) + 1e-3 |ref|) of one tensor: the project's gradient bar."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all())
    atol = 2e-5 * max(1.0, float(ref.abs().max()))
    return float(((got - ref).abs() / (atol + 1e-3 * ref.abs())).max())


def rho(got, ref, what=""):
    """The worst bar_ratio over d_planes and the four decoder gradients of two result dicts; prints every figure."""
    parts = {"planes": bar_ratio(got["planes"], ref["planes"])}
    for k, a, b in zip(DEC_KEYS, got["dec"], ref["dec"]):
        parts[k] = bar_ratio(a, b)
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in parts.items()) +
          f"; ref max |d planes| {float(ref['planes'].abs().max()):.3e}")
    return max(parts.values()), parts


def masked_case(preset, axes="eg3d_original", hw=(20, 20), box_warp=None, depths=None):
    """(case, sorted depths, G^ times the edge mask, mask) — with the oracle's own depths unless `depths` (the device's) is given."""
    cs = N.case(preset, axes, hw, box_warp)
    if depths is None:
        depths = oracle_depths(preset, axes, hw, box_warp)
    mask = edge_mask(cs["cfg"], hw, cs["c"], depths)
    assert float(mask.double().mean()) >= MIN_KEPT, f"only {int(mask.sum())} of {mask.numel()} rays kept"
    return cs, depths, upstream(cs) * mask[..., None], mask


@functools.lru_cache(maxsize=None)
def oracle_rho(preset, axes="eg3d_original", hw=(20, 20), box_warp=None):
    """rho of the fp32 reference against the float64 one under the mask, with the oracle's own depths (computed once per case)."""
    cs, depths, g_hat, _ = masked_case(preset, axes, hw, box_warp)
    ref = reference(cs["P"], cs["cfg"], cs["planes"], cs["c"], depths, g_hat)
    got = reference(cs["P"], cs["cfg"], cs["planes"], cs["c"], depths, g_hat, dtype=torch.float32)
    return rho(got, ref, f"{preset}/{axes}/{hw}/{box_warp}: fp32 reference")[0]
