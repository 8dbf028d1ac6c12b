"""Occupancy grids for ray lists: one bit per cell of a G³ grid over the tri-plane cube, from which `ops.ray_limits_grid`
(hfagp_ray_limits_grid) takes tight per-ray depth limits and a miss test — `render_rays(..., ray_limits=occ)`.  A grid comes from
`TriPlaneGenerator.occupancy_grid` (the density field, thresholded) or from any bool mask of the caller's (`from_dense`: a visual
hull, a scan's voxels)."""
from __future__ import annotations

from dataclasses import dataclass

import torch

G_MIN, G_MAX = 2, 256


@dataclass
class OccupancyGrid:
    """``bits`` int32 [B, G, G, W], W = ceil(G / 32): bit ``iz & 31`` of word ``iz >> 5`` at [b, ix, iy] is cell (ix, iy, iz);
    padding bits are 0.  ``resolution`` = G (2 … 256), ``cube_length`` = L: cell (ix, iy, iz) is the closed box
    [−L/2 + i·L/G, −L/2 + (i+1)·L/G] per axis, in the world frame `sample_mixed` takes."""
    bits: torch.Tensor
    resolution: int
    cube_length: float

    def __post_init__(self):
        g = int(self.resolution)
        if not G_MIN <= g <= G_MAX:
            raise ValueError(f"OccupancyGrid: resolution must be in [{G_MIN}, {G_MAX}], got {self.resolution}")
        length = float(self.cube_length)
        if not (length > 0 and length < float("inf")):
            raise ValueError(f"OccupancyGrid: cube_length must be positive and finite, got {self.cube_length}")
        w = (g + 31) // 32
        if self.bits.dtype != torch.int32 or self.bits.dim() != 4 or tuple(self.bits.shape[1:]) != (g, g, w):
            raise ValueError(f"OccupancyGrid: bits must be int32 [B, {g}, {g}, {w}], got {self.bits.dtype} {tuple(self.bits.shape)}")
        self.resolution, self.cube_length = g, length

    @property
    def batch(self) -> int:
        return self.bits.shape[0]

    def dense(self) -> torch.Tensor:
        """bool [B, G, G, G], indexed (ix, iy, iz)."""
        g = self.resolution
        shifts = torch.arange(32, device=self.bits.device, dtype=torch.int32)
        cells = (self.bits[..., None] >> shifts) & 1                   # [B,G,G,W,32]
        return cells.reshape(*self.bits.shape[:3], -1)[..., :g].bool()

    @classmethod
    def from_dense(cls, mask: torch.Tensor, cube_length: float) -> "OccupancyGrid":
        """A grid from any bool mask [B, G, G, G] (or [G, G, G]: one frame), indexed (ix, iy, iz).  Packs in torch, on the mask's
        device — CPU or GPU."""
        if mask.dim() == 3:
            mask = mask[None]
        if mask.dim() != 4 or mask.shape[1] != mask.shape[2] or mask.shape[2] != mask.shape[3]:
            raise ValueError(f"OccupancyGrid.from_dense: mask must be [B, G, G, G], got {tuple(mask.shape)}")
        g = mask.shape[1]
        if not G_MIN <= g <= G_MAX:
            raise ValueError(f"OccupancyGrid: resolution must be in [{G_MIN}, {G_MAX}], got {g}")
        w = (g + 31) // 32
        cells = torch.zeros(*mask.shape[:3], w * 32, device=mask.device, dtype=torch.int64)
        cells[..., :g] = mask != 0
        weights = torch.ones(32, device=mask.device, dtype=torch.int64) << torch.arange(32, device=mask.device, dtype=torch.int64)
        words = (cells.view(*mask.shape[:3], w, 32) * weights).sum(-1)                 # 0 … 2³² − 1
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)   # the same 32 bits as an int32
        return cls(words.contiguous(), g, cube_length)


def occupancy_reference(volume: torch.Tensor, resolution: int, oversample: int, level: float, dilate: int) -> torch.Tensor:
    """What `ops.occupancy_pack` computes, in plain torch (its reference; CPU or device): volume [B, n, n, n] with
    n = G·k + 1 → bool [B, G, G, G].  A cell is occupied iff one of the (k+1)³ lattice points of its closed extent has
    !(v < level) (a NaN counts), then the grid is dilated by `dilate` cells (Chebyshev, clipped at the cube)."""
    g, k = int(resolution), int(oversample)
    if volume.dim() != 4 or tuple(volume.shape[1:]) != (g * k + 1,) * 3:
        raise ValueError(f"occupancy_reference: volume must be [B, {g * k + 1}, ...] for G = {g}, k = {k}, got {tuple(volume.shape)}")
    pool = torch.nn.functional.max_pool3d
    hot = (~(volume < level)).float()[:, None]
    occ = pool(hot, kernel_size=k + 1, stride=k)
    for _ in range(int(dilate)):
        occ = pool(occ, kernel_size=3, stride=1, padding=1)
    return occ[:, 0] > 0
