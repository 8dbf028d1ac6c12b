"""Camera label synthesis — counterpart of /root/reference/code/cam_utils.py:12-80 and of the
intrinsics literal in code/trainer_rgb.py:32.  A label is 16 cam2world floats (row-major 4x4)
followed by 9 normalised intrinsics.  Pinned by tests/golden (cam_* vectors)."""
from __future__ import annotations

import math
import random
from typing import Tuple

import torch

FFHQ_INTRINSICS = (4.2647, 0.0, 0.5, 0.0, 4.2647, 0.5, 0.0, 0.0, 1.0)   # trainer_rgb.py:32


def normalize_vecs(v: torch.Tensor) -> torch.Tensor:
    return v / torch.norm(v, dim=-1, keepdim=True)


def _angles(device, n, h_std, v_std, h_mean, v_mean, mode) -> Tuple[torch.Tensor, torch.Tensor]:
    def uni(scale):
        return (torch.rand((n, 1), device=device) - 0.5) * 2 * scale

    def gauss(scale):
        return torch.randn((n, 1), device=device) * scale

    if mode == "uniform":
        return uni(h_std) + h_mean, uni(v_std) + v_mean
    if mode in ("normal", "gaussian"):
        return gauss(h_std) + h_mean, gauss(v_std) + v_mean
    if mode == "hybrid":
        if random.random() < 0.5:
            return uni(h_std * 2) + h_mean, uni(v_std * 2) + v_mean
        return gauss(h_std) + h_mean, gauss(v_std) + v_mean
    if mode == "truncated_gaussian":
        # the reference calls an undefined `truncated_normal_` here (cam_utils.py:36-37)
        raise NotImplementedError("mode 'truncated_gaussian' is not runnable in the reference either")
    if mode == "spherical_uniform":
        theta = uni(h_std) + h_mean
        v = torch.clamp(uni(v_std / math.pi) + v_mean / math.pi, 1e-5, 1 - 1e-5)
        return theta, torch.arccos(1 - 2 * v)
    ones = torch.ones((n, 1), device=device, dtype=torch.float)
    return ones * h_mean, ones * v_mean


def sample_camera_positions(device, n=1, r=1, horizontal_stddev=1, vertical_stddev=1,
                            horizontal_mean=math.pi * 0.5, vertical_mean=math.pi * 0.5, mode="normal"):
    """n points on the sphere of radius r.  theta = yaw, phi = pitch (clamped to (0, pi)).
    Returns (points [n,3], phi, theta) like the reference."""
    theta, phi = _angles(device, n, horizontal_stddev, vertical_stddev, horizontal_mean, vertical_mean, mode)
    phi = torch.clamp(phi, 1e-5, math.pi - 1e-5)
    pts = torch.zeros((n, 3), device=device)
    pts[:, 0:1] = r * torch.sin(phi) * torch.cos(theta)
    pts[:, 2:3] = r * torch.sin(phi) * torch.sin(theta)
    pts[:, 1:2] = r * torch.cos(phi)
    return pts, phi, theta


def create_cam2world_matrix(forward_vector: torch.Tensor, origin: torch.Tensor, device=None) -> torch.Tensor:
    """Look-at matrix from a viewing direction and a camera position: columns (-left, up, -forward)."""
    fwd = normalize_vecs(forward_vector)
    up0 = torch.tensor([0, 1, 0], dtype=torch.float, device=device).expand_as(fwd)
    left = normalize_vecs(torch.cross(up0, fwd, dim=-1))
    up = normalize_vecs(torch.cross(fwd, left, dim=-1))
    n = fwd.shape[0]
    rot = torch.eye(4, device=device).unsqueeze(0).repeat(n, 1, 1)
    rot[:, :3, :3] = torch.stack((-left, up, -fwd), dim=-1)
    trans = torch.eye(4, device=device).unsqueeze(0).repeat(n, 1, 1)
    trans[:, :3, 3] = origin
    return trans @ rot


def make_label(cam2world: torch.Tensor, intrinsics=FFHQ_INTRINSICS) -> torch.Tensor:
    n = cam2world.shape[0]
    k = torch.tensor(intrinsics, dtype=cam2world.dtype, device=cam2world.device).reshape(1, -1).repeat(n, 1)
    return torch.cat((cam2world.reshape(n, -1), k), -1)


def cam_sampler(batch: int, device, horizontal_mean=0.5, vertical_mean=0.5, horizontal_stddev=0.3,
                vertical_stddev=0.155, r=2.7) -> torch.Tensor:
    """trainer_rgb.py:27-42 (`cam_sampler`, `cam_sampler_pose`): gaussian poses around the mean, label [B,25]."""
    pts, _, _ = sample_camera_positions(device, n=batch, r=r, horizontal_mean=horizontal_mean * math.pi,
                                        vertical_mean=vertical_mean * math.pi, horizontal_stddev=horizontal_stddev,
                                        vertical_stddev=vertical_stddev, mode="gaussian")
    return make_label(create_cam2world_matrix(-pts, pts, device=device))


def orbit_labels(n: int, r: float = 2.7, yaw_range: float = 0.35, pitch_range: float = 0.25, pitch_offset: float = -0.05,
                 intrinsics=FFHQ_INTRINSICS, device=None) -> torch.Tensor:
    """The n cameras of a turntable around the head, labels [n,25] (un-flipped, as `sample_camera_positions` gives them): camera i
    stands on the sphere of radius r at yaw h_i = π/2 + yaw_range·sin(2πi/n) and pitch v_i = π/2 + pitch_offset +
    pitch_range·cos(2πi/n) — `sample_camera_positions`' angles: p = r·(sin v cos h, cos v, sin v sin h) — and looks at the origin.
    `synthesis(ws, orbit_labels(V)[None].expand(B, -1, -1))` renders the V views of every latent on one backbone pass."""
    if int(n) != n or n < 1:
        raise ValueError(f"orbit_labels: n must be a positive integer, got {n!r}")
    t = 2.0 * math.pi * torch.arange(int(n), dtype=torch.float, device=device) / int(n)
    h = 0.5 * math.pi + yaw_range * torch.sin(t)
    v = 0.5 * math.pi + pitch_offset + pitch_range * torch.cos(t)
    pts = r * torch.stack((torch.sin(v) * torch.cos(h), torch.cos(v), torch.sin(v) * torch.sin(h)), dim=-1)
    return make_label(create_cam2world_matrix(-normalize_vecs(pts), pts, device=device), intrinsics)


def ray_grid(c: torch.Tensor, res: int, window=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """EG3D's RaySampler for a label, in plain torch: c [B,25] → (origins, directions), each [B, res*res, 3], pixel centres of a
    res x res image in row order, unit directions — the rays `synthesis` marches when res is the rendering resolution, and the rays
    `TriPlaneGenerator.render_rays` takes at any res.  ``window`` = (u0, v0, u1, v1) in normalised image coordinates (u along a
    row, v down the rows; the whole image is (0, 0, 1, 1)): the res x res pixel centres of that rectangle instead — a crop, or a zoom
    at a higher ray density.  Differentiable w.r.t. c."""
    n = c.shape[0]
    ar = torch.arange(res, dtype=c.dtype, device=c.device)
    uv = torch.stack(torch.meshgrid(ar, ar, indexing="ij")) * (1.0 / res) + (0.5 / res)
    uv = uv.flip(0).reshape(2, -1).transpose(1, 0)[None].repeat(n, 1, 1)
    xc, yc = uv[:, :, 0], uv[:, :, 1]
    if window is not None:
        u0, v0, u1, v1 = (float(t) for t in window)
        xc, yc = u0 + xc * (u1 - u0), v0 + yc * (v1 - v0)
    return _rays_through(c, xc, yc)


def _rays_through(c: torch.Tensor, xc: torch.Tensor, yc: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The rays of the labels c [B,25] through the image points (xc, yc), each [B,P], in normalised image coordinates: the one
    formula behind `ray_grid` and `pixel_rays`."""
    n = c.shape[0]
    c2w, intr = c[:, :16].reshape(n, 4, 4), c[:, 16:25].reshape(n, 3, 3)
    cam = c2w[:, :3, 3]
    fx, fy = intr[:, 0, 0], intr[:, 1, 1]
    cx, cy = intr[:, 0, 2], intr[:, 1, 2]
    sk = intr[:, 0, 1]
    zc = torch.ones_like(xc)
    xl = (xc - cx[:, None] + cy[:, None] * sk[:, None] / fy[:, None] - sk[:, None] * yc / fy[:, None]) / fx[:, None] * zc
    yl = (yc - cy[:, None]) / fy[:, None] * zc
    pts = torch.stack((xl, yl, zc, torch.ones_like(zc)), dim=-1)
    world = torch.bmm(c2w, pts.permute(0, 2, 1)).permute(0, 2, 1)[:, :, :3]
    dirs = torch.nn.functional.normalize(world - cam[:, None, :], dim=2)
    origins = cam[:, None, :].repeat(1, dirs.shape[1], 1)
    return origins, dirs.contiguous()          # (both contiguous: ops.raymarch_rays takes them as they are)


def pixel_rays(c: torch.Tensor, uv: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The rays of a label through given image points: c [B,25], uv [B,P,2] in `ray_grid`'s normalised image coordinates (u along a
    row, v down the rows, the whole image is [0,1]²; the centre of pixel (row i, column j) of a res x res image is
    u = j·(1/res) + 0.5/res, v = i·(1/res) + 0.5/res) → (origins, directions), each [B,P,3], unit directions.  `ray_grid`'s formula,
    so at its pixel centres the results are bit-equal to its rays.  Differentiable w.r.t. c and uv — a 2-D landmark becomes a 3-D
    point on the head with `TriPlaneGenerator.trace_rays` on these rays."""
    if uv.dim() != 3 or uv.shape[-1] != 2 or uv.shape[0] != c.shape[0]:
        raise ValueError(f"pixel_rays: uv must be [B, P, 2] for c of batch {c.shape[0]}, got {tuple(uv.shape)}")
    return _rays_through(c, uv[:, :, 0], uv[:, :, 1])


def ray_grid_ortho(cam2world: torch.Tensor, res: int, extent: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """A parallel-projection ray grid: cam2world [B,4,4] (or [B,16]) → (origins, directions), each [B, res*res, 3].  Origins are the
    res x res pixel centres of a square of side ``extent`` (world units) in the camera's z = 0 plane, centred on the camera
    position, in `ray_grid`'s row order (x along a row, y down the rows, in the camera's own axes); every direction is the camera's
    +z axis as cam2world gives it (unit length for a rigid pose).  With `render_rays(..., ray_limits="box")` the camera may stand at
    any distance.  Differentiable w.r.t. cam2world."""
    n = cam2world.shape[0]
    c2w = cam2world.reshape(n, 4, 4)
    ar = (torch.arange(res, dtype=c2w.dtype, device=c2w.device) * (1.0 / res) + (0.5 / res) - 0.5) * float(extent)
    yl, xl = torch.meshgrid(ar, ar, indexing="ij")                 # rows = y, columns = x: pixel (i, j) is ray i * res + j
    pts = torch.stack((xl.reshape(-1), yl.reshape(-1)), dim=-1)    # [R, 2] in the camera's z = 0 plane
    origins = c2w[:, None, :3, 3] + pts[None, :, 0:1] * c2w[:, None, :3, 0] + pts[None, :, 1:2] * c2w[:, None, :3, 1]
    dirs = c2w[:, None, :3, 2].expand(-1, res * res, -1)
    return origins.contiguous(), dirs.contiguous()


def ray_limits_box(origins: torch.Tensor, directions: torch.Tensor, box_side: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(t_near, t_far), each [..., ] for rays [..., 3]: the slab intersection with the cube [−box_side/2, box_side/2]³ in plain
    torch — the formula of `ops.ray_limits_box` (hfagp_ray_limits_box), for which this is the reference, and usable on the CPU.
    Per axis inv = 1 / d (±inf for a zero component), t0 = (−h − o)·inv, t1 = (h − o)·inv;  t_near = max over the axes of
    min(t0, t1), clamped below at 0 — NOT EG3D's value for an origin inside the box (math_utils.get_ray_limits_box), on purpose: the
    ray starts at its origin —;  t_far = min over the axes of max(t0, t1).  A ray misses iff t_far <= t_near; 0 · inf (origin
    exactly on a slab of an axis the ray is parallel to) is NaN and makes both limits NaN.  Not differentiable (computed under
    no_grad): the limits carry no gradient."""
    with torch.no_grad():
        h = 0.5 * float(box_side)
        inv = 1.0 / directions
        t0, t1 = (-h - origins) * inv, (h - origins) * inv
        near = torch.minimum(t0, t1).amax(-1).clamp(min=0.0)       # (minimum / maximum / amax / amin propagate NaN)
        far = torch.maximum(t0, t1).amin(-1)
        bad = torch.isnan(near) | torch.isnan(far)
        nan = torch.full_like(near, float("nan"))
        return torch.where(bad, nan, near), torch.where(bad, nan, far)


def ray_limits_valid(t_near: torch.Tensor, t_far: torch.Tensor) -> torch.Tensor:
    """The rays the ray marcher marches: both limits finite and t_far > t_near (bool, the shape of the limits)."""
    return torch.isfinite(t_near) & torch.isfinite(t_far) & (t_far > t_near)


def ray_limits_grid(origins: torch.Tensor, directions: torch.Tensor, dense: torch.Tensor, cube_length: float,
                    max_pairs: int = 1 << 22) -> Tuple[torch.Tensor, torch.Tensor]:
    """(t_near, t_far), each [B, R], of rays [B, R, 3] against an occupancy mask `dense` bool [B or 1, G, G, G] (indexed ix, iy, iz)
    over the cube of side `cube_length`: the entry of the first and the exit of the last occupied cell a ray passes through at
    t ≥ 0 — the reference of `ops.ray_limits_grid` (hfagp_ray_limits_grid) in plain torch, in the dtype of the rays (float32 as the
    kernel computes, float64 as its yardstick), usable on the CPU.  A BRUTE FORCE on purpose: per ray the slab interval against
    EVERY occupied cell, then a min / max over the cells — no traversal, no order, nothing shared with the kernel's DDA.  Chunked
    over the rays so that rays × cells stays below `max_pairs`.
    Cell (ix, iy, iz) spans [plane(i), plane(i+1)] per axis, plane(i) = −L/2 + i·(L/G).  Per axis with d ≠ 0: inv = 1/d,
    ta = (plane(i) − o)·inv, tb = (plane(i+1) − o)·inv, in = min(ta, tb), out = max(ta, tb) (`ray_limits_box`'s formula on the
    cell's planes); an axis with d = 0 lies in the half-open slab plane(i) ≤ o < plane(i+1) of one i (in = −inf, out = +inf), and
    o ≤ plane(0) or o ≥ plane(G) there empties the ray (the box's 0·inf).  near_c = max in, far_c = min out; a cell COUNTS iff
    far_c > max(near_c, 0) (a NaN never does); t_near = min over the counting cells of max(near_c, 0), t_far = max of far_c.  No
    counting cell, a zero direction or a limit that is not finite: (+inf, −inf), an empty ray.  Not differentiable."""
    if origins.dim() != 3 or origins.shape[-1] != 3 or origins.shape != directions.shape:
        raise ValueError(f"ray_limits_grid: origins / directions must be [B, R, 3], got {tuple(origins.shape)}, {tuple(directions.shape)}")
    if dense.dim() != 4 or dense.shape[0] not in (1, origins.shape[0]) or len(set(dense.shape[1:])) != 1:
        raise ValueError(f"ray_limits_grid: dense must be [B or 1, G, G, G] for {origins.shape[0]} frames, got {tuple(dense.shape)}")
    with torch.no_grad():
        b, r = origins.shape[:2]
        g = dense.shape[1]
        dt, dev = origins.dtype, origins.device
        inf = float("inf")
        half = torch.tensor(0.5 * float(cube_length), dtype=dt, device=dev)
        cell = torch.tensor(float(cube_length), dtype=dt, device=dev) / g
        plane = -half + torch.arange(g + 1, device=dev).to(dt) * cell          # [G+1], each operation rounded in dt
        t_near = torch.full((b, r), inf, dtype=dt, device=dev)
        t_far = torch.full((b, r), -inf, dtype=dt, device=dev)
        for f in range(b):
            cells = dense[f if dense.shape[0] > 1 else 0].nonzero()          # [C, 3]
            if cells.shape[0] == 0:
                continue
            lo, hi = plane[cells], plane[cells + 1]                           # [C, 3]
            chunk = max(1, int(max_pairs) // cells.shape[0])
            for r0 in range(0, r, chunk):
                o, d = origins[f, r0:r0 + chunk, None, :], directions[f, r0:r0 + chunk, None, :]     # [n, 1, 3]
                inv = 1.0 / d
                ta, tb = (lo - o) * inv, (hi - o) * inv                       # [n, C, 3]
                t_in, t_out = torch.minimum(ta, tb), torch.maximum(ta, tb)    # (NaN propagates)
                par = (d == 0).expand_as(ta)
                inside = (lo <= o) & (o < hi)
                t_in = torch.where(par, torch.where(inside, -inf, inf).to(dt), t_in)
                t_out = torch.where(par, torch.where(inside, inf, -inf).to(dt), t_out)
                near_c = t_in.amax(-1).clamp(min=0.0)                         # (amax / amin / clamp propagate NaN)
                far_c = t_out.amin(-1)
                counts = far_c > near_c                                       # (False for a NaN)
                t_near[f, r0:r0 + chunk] = torch.where(counts, near_c, torch.full_like(near_c, inf)).amin(1)
                t_far[f, r0:r0 + chunk] = torch.where(counts, far_c, torch.full_like(far_c, -inf)).amax(1)
        par = directions == 0
        empty = par.all(-1) | (par & ((origins <= plane[0]) | (origins >= plane[g]))).any(-1)
        empty |= ~(torch.isfinite(t_near) & torch.isfinite(t_far))
        return torch.where(empty, torch.full_like(t_near, inf), t_near), torch.where(empty, torch.full_like(t_far, -inf), t_far)
