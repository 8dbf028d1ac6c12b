"""Batched reenactment harness — counterpart of the per-frame loop in
/root/reference/code/run_recon_video_rgb.py:216-236 (driver → get_latent → get_image → save_image)
and of its `layout_grid` uint8 quantisation (:28-42).  PNG / mp4 encoding is out of scope
(SURVEY.md §2.1 row 7); frames come back as uint8 tensors, quantised on the GPU and copied to pinned
host memory asynchronously so the copy of batch i overlaps the render of batch i+1."""
from __future__ import annotations

from typing import Iterable, Iterator, Optional, Tuple

import numpy as np
import torch


def to_uint8(img: torch.Tensor) -> torch.Tensor:
    """[-1, 1] float image → uint8 with the reference's rounding: (img * 127.5 + 128).clamp(0, 255)."""
    return (img * 127.5 + 128).clamp(0, 255).to(torch.uint8)


def layout_grid(img: torch.Tensor, grid_w: Optional[int] = None, grid_h: int = 1, float_to_uint8: bool = True,
                chw_to_hwc: bool = True, to_numpy: bool = True):
    """Tile a batch [B,C,H,W] into one grid_h x grid_w image."""
    b, c, h, w = img.shape
    if grid_w is None:
        grid_w = b // grid_h
    assert b == grid_w * grid_h
    if float_to_uint8:
        img = to_uint8(img)
    img = img.reshape(grid_h, grid_w, c, h, w).permute(2, 0, 3, 1, 4).reshape(c, grid_h * h, grid_w * w)
    if chw_to_hwc:
        img = img.permute(1, 2, 0)
    return img.cpu().numpy() if to_numpy else img


@torch.no_grad()
def render_frames(gen, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], person_2: bool = False,
                  to_host: bool = True, neural_rendering_resolution: Optional[int] = None) -> Iterator[torch.Tensor]:
    """`gen` is a HeadNeRF_* module; `batches` yields (driver_input [B,...], label [B,25]) on gen's device.
    Yields uint8 frames [B,3,H,W].  The label flip side effect of `get_image` is preserved.
    A label [B,V,25] renders V cameras of every driven frame on one backbone pass (a stereo pair or a light-field frame of a
    reenacted clip; `cam_utils.orbit_labels` for a turntable) and yields [B,V,3,H,W]: the view axis after the frame axis.
    `neural_rendering_resolution=N`: march N x N rays per frame (`get_image(neural_rendering_resolution=)`; twice the configured
    value supersamples a clip: four rays per super-resolution input pixel).  The generator keeps N afterwards."""
    res_kw = {} if neural_rendering_resolution is None else {"neural_rendering_resolution": neural_rendering_resolution}
    gen.eval()
    copy_stream = torch.cuda.Stream() if to_host and torch.cuda.is_available() else None
    pending = None
    for driver_in, label in batches:
        weights = gen.get_weights(driver_in)
        if isinstance(weights, tuple):
            weights = weights[0]
        frames = to_uint8(gen.get_image(gen.get_latent(weights, person_2), label, **res_kw))
        if copy_stream is None:
            yield frames
            continue
        host = torch.empty(frames.shape, dtype=torch.uint8, pin_memory=True)
        copy_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(copy_stream):
            host.copy_(frames, non_blocking=True)
            frames.record_stream(copy_stream)
            done = torch.cuda.Event()
            done.record(copy_stream)
        if pending is not None:
            pending[1].synchronize()
            yield pending[0]
        pending = (host, done)
    if pending is not None:
        pending[1].synchronize()
        yield pending[0]


def normal_map(image_normal: torch.Tensor, c: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """'image_normal' [B,3,r,r] of `synthesis(normals=True)` (world space, not normalised) → uint8 [B,3,r,r] in the conventional
    colouring n·0.5 + 0.5 of the per-pixel UNIT normal (zero, i.e. mid-grey, where ‖N‖ is 0).
    `c` [B,25], the label the synthesis call received: the normals are rotated into that camera's space first (the transpose of
    the label's cam2world rotation block).  `mask` [B,1,r,r] ('image_mask'): the unit normal is premultiplied by it, so that
    empty rays fade to mid-grey.  Plain torch, on whatever device the inputs live."""
    n = image_normal.detach().float()
    if n.dim() != 4 or n.shape[1] != 3:
        raise ValueError(f"normal_map: expected image_normal [B, 3, r, r], got {tuple(image_normal.shape)}")
    norm = n.norm(dim=1, keepdim=True)
    n = torch.where(norm > 0, n / norm.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(n))
    if c is not None:
        rot = c.detach().float()[:, :16].reshape(-1, 4, 4)[:, :3, :3].to(n.device)        # cam2world: n_cam = rotᵀ n_world
        n = torch.einsum("bji,bjhw->bihw", rot, n)
    if mask is not None:
        n = n * mask.detach().float().to(n.device)
    return to_uint8(n)


# ----------------------------------------------------------------------------- shape export (EG3D gen_samples.py --shapes)
def shape_volume_eg3d(sigma_grid) -> np.ndarray:
    """EG3D's post-processing of a density grid [N, N, N] (TriPlaneGenerator.density_grid of one identity, indexed (ix, iy, iz)):
    flip along axis 0, then every voxel within pad = int(30 N / 256) of a face set to -1000.  Returns a float32 numpy array."""
    v = sigma_grid.detach().float().cpu().numpy() if isinstance(sigma_grid, torch.Tensor) else np.asarray(sigma_grid, np.float32)
    if v.ndim != 3 or len(set(v.shape)) != 1:
        raise ValueError(f"shape_volume_eg3d: expected an [N, N, N] grid, got {v.shape}")
    v = np.ascontiguousarray(np.flip(v, 0), dtype=np.float32)
    pad = int(30 * v.shape[0] / 256)
    if pad > 0:
        v[:pad] = -1000; v[-pad:] = -1000
        v[:, :pad] = -1000; v[:, -pad:] = -1000
        v[:, :, :pad] = -1000; v[:, :, -pad:] = -1000
    return v


def shape_mesh_eg3d(sigma_grid: torch.Tensor, level: float = 10.0):
    """EG3D's .ply geometry (gen_samples.py --shapes: convert_sdf_samples_to_ply of the transposed volume, level 10) on the GPU:
    the flip and -1000 border of `shape_volume_eg3d`, then transpose(2, 1, 0), then marching cubes with spacing 1 and origin 0
    (EG3D's vertex units: lattice indices of the transposed volume).  `sigma_grid` [N, N, N] is one identity of
    TriPlaneGenerator.density_grid, on the GPU.  Returns (verts [V, 3] float32, faces [F, 3] int32) on its device."""
    from . import ops
    if not isinstance(sigma_grid, torch.Tensor) or not sigma_grid.is_cuda:
        raise RuntimeError("shape_mesh_eg3d: expected a CUDA/ROCm [N, N, N] tensor (the HIP path has no CPU fallback)")
    if sigma_grid.dim() != 3 or len(set(sigma_grid.shape)) != 1:
        raise ValueError(f"shape_mesh_eg3d: expected an [N, N, N] grid, got {tuple(sigma_grid.shape)}")
    with torch.no_grad():
        v = _border_eg3d(sigma_grid.detach().float().flip(0))
        return ops.marching_cubes(v.permute(2, 1, 0).contiguous(), level)


def _border_eg3d(v: torch.Tensor) -> torch.Tensor:
    """EG3D's border trim of a shape volume (a fresh tensor): voxels within int(30 N / 256) of a face set to -1000"""
    v = v.clone()
    pad = int(30 * v.shape[0] / 256)
    if pad > 0:
        v[:pad] = -1000; v[-pad:] = -1000
        v[:, :pad] = -1000; v[:, -pad:] = -1000
        v[:, :, :pad] = -1000; v[:, :, -pad:] = -1000
    return v


def save_ply(path, verts, faces, colors=None, normals=None) -> None:
    """Write a triangle mesh as binary little-endian PLY in the layout plyfile writes for EG3D's shape export: `element vertex`
    with float x / y / z (then float nx / ny / nz when `normals` [V, 3] is given, then uchar red / green / blue when `colors`
    [V, 3] uint8 is given: the order plyfile and MeshLab use), `element face` with `property list uchar int vertex_indices`.
    verts [V, 3], faces [F, 3]: numpy arrays or tensors.  Without `normals` the file is what it was before the keyword existed."""
    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    v, f = host(verts), host(faces)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"save_ply: expected verts [V, 3] and faces [F, 3], got {v.shape} and {f.shape}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    if normals is not None:
        nrm = host(normals)
        if nrm.shape != v.shape or nrm.dtype.kind != "f":
            raise ValueError(f"save_ply: normals must be floating point [V, 3], got {nrm.dtype} {nrm.shape}")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        c = host(colors)
        if c.shape != v.shape or c.dtype != np.uint8:
            raise ValueError(f"save_ply: colors must be uint8 [V, 3], got {c.dtype} {c.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    vert = np.empty(v.shape[0], dtype=fields)
    for i, name in enumerate("xyz"):
        vert[name] = v[:, i]
    if normals is not None:
        for i, name in enumerate(("nx", "ny", "nz")):
            vert[name] = nrm[:, i]
    if colors is not None:
        for i, name in enumerate(("red", "green", "blue")):
            vert[name] = c[:, i]
    face = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    face["n"] = 3
    face["idx"] = f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", *props,
              f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vert.tobytes())
        out.write(face.tobytes())


def save_mrc(path, volume, voxel_size: float = 1.0) -> None:
    """Write a float32 volume [NZ, NY, NX] (C order: NX = last axis) as an MRC2014 map (MODE 2), the format EG3D's shape export
    writes through the `mrcfile` package: 1024-byte header, then the data.  Cell = N * voxel_size per axis, angles 90."""
    v = np.ascontiguousarray(np.asarray(volume, dtype=np.float32))
    if v.ndim != 3:
        raise ValueError(f"save_mrc: expected a 3-D volume, got {v.shape}")
    nz, ny, nx = v.shape
    words = np.zeros(256, dtype="<i4")
    floats = words.view("<f4")
    words[0:3] = (nx, ny, nz)                 # NX NY NZ
    words[3] = 2                              # MODE 2: float32
    words[7:10] = (nx, ny, nz)                # MX MY MZ
    floats[10:13] = (nx * voxel_size, ny * voxel_size, nz * voxel_size)    # CELLA
    floats[13:16] = 90.0                      # CELLB
    words[16:19] = (1, 2, 3)                  # MAPC MAPR MAPS
    vd = v.astype(np.float64)
    floats[19], floats[20], floats[21] = (v.min(), v.max(), vd.mean()) if v.size else (0.0, 0.0, 0.0)    # DMIN DMAX DMEAN
    words[22] = 1                             # ISPG
    words[27] = 20140                         # NVERSION
    header = bytearray(words.tobytes())
    header[208:212] = b"MAP "                 # MAP (word 53)
    header[212:216] = bytes((0x44, 0x44, 0, 0))   # MACHST: little-endian
    floats_rms = np.float32(np.sqrt(((vd - vd.mean()) ** 2).mean())) if v.size else np.float32(0)
    header[216:220] = np.array([floats_rms], dtype="<f4").tobytes()           # RMS (word 55)
    with open(path, "wb") as f:
        f.write(bytes(header))
        f.write(v.astype("<f4", copy=False).tobytes())
