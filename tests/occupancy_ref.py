"""What tests/test_occupancy_cpu.py and tests/test_gpu_occupancy.py share: the ray recipe, the seeded masks, the grazing test and the
tolerance of the occupancy-grid ray limits (cam_utils.ray_limits_grid is the reference itself and lives in the package)."""
import math

import torch

CUBE = 1.0                      # cube_length of every case here (box_warp of the presets)
GRAZING_REL = 1e-3              # a ray is grazing if an occupied cell's chord is below this share of L / G / |d|
GRAZING_CAP = 0.02              # ... and at most this share of a recipe's rays may be
# per G, the largest |float32 - float64| of t_near / t_far of cam_utils.ray_limits_grid off the grazing rays in
# test_occupancy_cpu.test_twin_float32_vs_float64 (t <= 3.5): measured there — 3.814e-7, 3.953e-7, 2.242e-6 — rounded up in the
# third digit and asserted against (profiles/occupancy/README.md).  G = 40 is larger because L / G is not exact in float32.
TWIN_F32_DEVIATION = {8: 3.9e-7, 16: 4.0e-7, 40: 2.3e-6}


def atol_gpu(g: int) -> float:
    """4 x the float32 reference's own deviation at this G: the margin covers a differently rounded reciprocal, not an accumulated DDA."""
    return 4 * TWIN_F32_DEVIATION[g]


def random_mask(g: int, seed: int, b: int = 1, share: float = 0.3) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(b, g, g, g, generator=gen) < share


def recipe_rays(r: int, seed: int, b: int = 1, dtype=torch.float64):
    """[B, R, 3] origins / directions: the first half unit rays from radius 2.7 towards points in [-0.6, 0.6]^3, the second half
    origins in [-0.7, 0.7]^3 with directions of length 0.5 ... 2."""
    gen = torch.Generator().manual_seed(seed)
    h = r // 2
    o1 = torch.nn.functional.normalize(torch.randn(b, h, 3, generator=gen, dtype=torch.float64), dim=-1) * 2.7
    tgt = (torch.rand(b, h, 3, generator=gen, dtype=torch.float64) - 0.5) * 1.2
    d1 = torch.nn.functional.normalize(tgt - o1, dim=-1)
    o2 = (torch.rand(b, r - h, 3, generator=gen, dtype=torch.float64) - 0.5) * 1.4
    d2 = torch.nn.functional.normalize(torch.randn(b, r - h, 3, generator=gen, dtype=torch.float64), dim=-1)
    d2 = d2 * (0.5 + 1.5 * torch.rand(b, r - h, 1, generator=gen, dtype=torch.float64))
    o, d = torch.cat((o1, o2), 1), torch.cat((d1, d2), 1)
    # rounded to float32 first, so that the float32 and the float64 evaluation see the SAME rays
    return o.float().to(dtype), d.float().to(dtype)


def grazing(o: torch.Tensor, d: torch.Tensor, dense: torch.Tensor, cube: float = CUBE, chunk: int = 256) -> torch.Tensor:
    """bool [B, R] in float64: the ray has an occupied cell whose signed chord far_c - max(near_c, 0) is closer to zero than
    GRAZING_REL * (L / G) / |d| — a hit or a miss of that cell is then a matter of rounding."""
    o, d = o.double(), d.double()
    b, r = o.shape[:2]
    g = dense.shape[1]
    plane = -0.5 * cube + torch.arange(g + 1, dtype=torch.float64) * (cube / g)
    out = torch.zeros(b, r, dtype=torch.bool)
    for f in range(b):
        cells = dense[f if dense.shape[0] > 1 else 0].nonzero()
        if not cells.shape[0]:
            continue
        lo, hi = plane[cells], plane[cells + 1]
        for r0 in range(0, r, chunk):
            oc, dc = o[f, r0:r0 + chunk, None], d[f, r0:r0 + chunk, None]
            par = (dc == 0).expand(-1, cells.shape[0], -1)
            dsafe = torch.where(dc == 0, torch.ones_like(dc), dc)
            ta, tb = (lo - oc) / dsafe, (hi - oc) / dsafe
            inside = (lo <= oc) & (oc <= hi)
            t_in = torch.where(par, torch.where(inside, -math.inf, math.inf), torch.minimum(ta, tb))
            t_out = torch.where(par, torch.where(inside, math.inf, -math.inf), torch.maximum(ta, tb))
            chord = t_out.amin(-1) - t_in.amax(-1).clamp(min=0.0)
            bar = GRAZING_REL * (cube / g) / dc.norm(dim=-1).clamp(min=1e-30)
            out[f, r0:r0 + chunk] = (chord.abs() < bar).any(1)
    return out


def special_rays(g: int, dense: torch.Tensor, cube: float = CUBE):
    """Rows that a DDA gets wrong first, for frame 0 of `dense`: zero components (axis-parallel rays through cell centres, from
    inside and outside), rays that miss the cube, a zero direction, an origin in the centre of an occupied cell.  float32 values
    as float64 tensors [1, n, 3]."""
    cell = cube / g
    centre = lambda i: -0.5 * cube + (i + 0.5) * cell          # noqa: E731
    occ = dense[0].nonzero()[0].tolist()
    c = [centre(i) for i in occ]
    rows = [
        ((-2.0, centre(1), centre(2)), (1.0, 0.0, 0.0)),      # parallel to x through cell centres, from outside
        ((centre(0), 2.0, centre(g - 1)), (0.0, -0.5, 0.0)),  # parallel to -y, not unit length
        ((centre(1), centre(1), centre(1)), (0.0, 0.0, 2.0)),  # parallel to z from inside
        ((centre(2), centre(0), -3.0), (0.0, 1e-3, 1.0)),     # one zero component
        ((0.9, 0.9, 0.9), (1.0, 0.0, 0.0)),                   # parallel and outside the cube: a miss
        ((2.0, 2.0, 2.0), (1.0, 1.0, 1.0)),                   # points away: a miss
        ((0.0, 3.0, 0.0), (1.0, 0.0, 0.2)),                   # passes beside the cube: a miss
        ((0.1, 0.1, 0.1), (0.0, 0.0, 0.0)),                   # zero direction
        (tuple(c), (0.3, -0.2, 0.9)),                         # origin in an occupied cell: t_near == 0
        (tuple(c), (-1.0, 0.0, 0.0)),                         # the same, axis-parallel
    ]
    o = torch.tensor([r[0] for r in rows], dtype=torch.float32)[None]
    d = torch.tensor([r[1] for r in rows], dtype=torch.float32)[None]
    return o.double(), d.double()
