"""Closed forms of the camera gradient of the ray marcher (csrc/raymarch_camera.hip, include/hfagp.h
hfagp_raymarch_bwd_camera) in plain torch, dtype-generic: the positional derivative of the tri-plane bilinear gather, its sums
along a ray, and the adjoint of the ray generation down to the 25-float label.  tests/test_camera_grad_cpu.py checks them against
autograd through the oracle in float64; the GPU tests use them as the description of what the kernels compute."""
import torch

# (ax, ay): the coordinates of the normalised sample point q that plane pl projects (raymarch_common.h plane_coords)
PLANE_AXES = {"eg3d_original": ((0, 1), (0, 2), (2, 0)), "eg3d_fixed": ((0, 1), (0, 2), (2, 1))}
# columns of the label that carry a gradient: rows 0-2 of cam2world; fx, skew, cx, fy, cy
NONZERO_COLUMNS = list(range(12)) + [16, 17, 18, 20, 21]


def gather_position_grad(planes, coords, g, axes="eg3d_original", box_warp=1.0):
    """planes [N,3,C,H,W], sample points coords [N,M,3], g [N,M,C] = dL/d(mean over the planes of the bilinear samples)
    -> dL/dcoords [N,M,3].  grid_sample(bilinear, zeros, align_corners=False): pixel = (q + 1) size / 2 - 0.5; a tap
    outside the plane is a zero texel."""
    n, _, c, h, w = planes.shape
    m = coords.shape[1]
    q = (2.0 / box_warp) * coords
    dq = torch.zeros_like(q)
    bidx = torch.arange(n)[:, None].expand(n, m)
    for pl, (ax, ay) in enumerate(PLANE_AXES[axes]):
        ix = (q[..., ax] + 1) * (w / 2) - 0.5
        iy = (q[..., ay] + 1) * (h / 2) - 0.5
        x0f, y0f = torch.floor(ix), torch.floor(iy)
        fx, fy = ix - x0f, iy - y0f
        x0 = x0f.clamp(-2, w + 1).long()
        y0 = y0f.clamp(-2, h + 1).long()
        tex = planes[:, pl].permute(0, 2, 3, 1)          # [N,H,W,C]

        def tap(yy, xx):
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            t = tex[bidx, yy.clamp(0, h - 1), xx.clamp(0, w - 1)]       # [N,M,C]
            return torch.where(ok, (t * g).sum(-1), torch.zeros_like(ix))

        p_nw, p_ne, p_sw, p_se = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
        dix = ((p_ne - p_nw) * (1 - fy) + (p_se - p_sw) * fy) * (w / 2) / 3
        diy = ((p_sw - p_nw) * (1 - fx) + (p_se - p_ne) * fx) * (h / 2) / 3
        dq[..., ax] += dix
        dq[..., ay] += diy
    return (2.0 / box_warp) * dq


def ray_sums(dp, t):
    """dp [B,R,S,3] = dL/d(sample point), t [B,R,S] sample depths -> ray_grad [B,R,6] = (dL/d origin, dL/d direction): the
    point is o + t d and the depths carry no gradient."""
    return torch.cat((dp.sum(2), (t[..., None] * dp).sum(2)), -1)


def ray_setup_adjoint(c, res, ray_grad):
    """Label c [B,25] (cam2world row-major, then the 3x3 intrinsics), ray_grad [B,R,6] with ray n = row * res + column
    -> dL/dc [B,25].  v = M (xl, yl, 1, 1) - o, d = v / |v|, o = M[:, 3]."""
    b = c.shape[0]
    M = c[:, :16].reshape(b, 4, 4)
    K = c[:, 16:25].reshape(b, 3, 3)
    fx, sk, cx, fy, cy = (K[:, 0, 0, None], K[:, 0, 1, None], K[:, 0, 2, None], K[:, 1, 1, None], K[:, 1, 2, None])
    ar = (torch.arange(res, dtype=c.dtype, device=c.device) + 0.5) / res
    yc = ar[:, None].expand(res, res).reshape(1, -1)
    xc = ar[None, :].expand(res, res).reshape(1, -1)
    xl = (xc - cx + cy * sk / fy - sk * yc / fy) / fx              # [B,R]
    yl = (yc - cy) / fy
    v = M[:, None, :3, 0] * xl[..., None] + M[:, None, :3, 1] * yl[..., None] + M[:, None, :3, 2]      # [B,R,3]
    nrm = v.norm(dim=-1, keepdim=True)
    d = v / nrm
    g_o, g_d = ray_grad[..., :3], ray_grad[..., 3:]
    gv = (g_d - d * (d * g_d).sum(-1, keepdim=True)) / nrm
    dM = torch.zeros(b, 4, 4, dtype=c.dtype, device=c.device)
    dM[:, :3, 0] = (gv * xl[..., None]).sum(1)
    dM[:, :3, 1] = (gv * yl[..., None]).sum(1)
    dM[:, :3, 2] = gv.sum(1)
    dM[:, :3, 3] = g_o.sum(1)                                       # (column 3 enters v as w - o: the two contributions cancel)
    dxl = (gv * M[:, None, :3, 0]).sum(-1)
    dyl = (gv * M[:, None, :3, 1]).sum(-1)
    dn = dxl / fx                                                   # xl = (xc - cx - sk yl) / fx
    dyl_t = dyl - sk * dn
    dK = torch.zeros(b, 3, 3, dtype=c.dtype, device=c.device)
    dK[:, 0, 0] = -(dn * xl).sum(1)
    dK[:, 0, 1] = -(dn * yl).sum(1)
    dK[:, 0, 2] = -dn.sum(1)
    dK[:, 1, 1] = -(dyl_t * yl / fy).sum(1)
    dK[:, 1, 2] = -(dyl_t / fy).sum(1)
    return torch.cat((dM.reshape(b, 16), dK.reshape(b, 9)), 1)
