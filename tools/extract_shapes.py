#!/usr/bin/env python
"""Shape export in the spirit of EG3D's `gen_samples.py --shapes`: the density volume of a generated or fitted head as an
MRC2014 map, one `seedNNNN.mrc` per seed (or `<ws file stem>_<b>.mrc` per identity of a saved ws).

    python tools/extract_shapes.py --preset ffhq512_128 --weights ffhq512-128.safetensors --seeds 0-3 --outdir out/
    python tools/extract_shapes.py --preset tiny14 --ws fitted_ws.npy --resolution 256 --outdir out/

Seeds go through `mapping(z, c)` with z = RandomState(seed).randn(z_dim) and the frontal conditioning label EG3D uses
(camera on the +z axis at radius 2.7 around the pivot (0, 0, 0.2), FFHQ intrinsics).  A `.npy` of ws [B, num_ws, w_dim]
(e.g. `HeadNeRF_*.get_latent(...)` saved with numpy) skips the mapping.  The volume is `TriPlaneGenerator.density_grid`
(one backbone pass, one launch per x slab) post-processed like EG3D (`render.shape_volume_eg3d`: flip along axis 0, borders
set to -1000) and written with the lattice spacing box_warp / (resolution - 1) as voxel size.

`--format ply` (or `both`) writes the surface as `<name>.ply` instead (or as well), in EG3D's vertex units: marching cubes
at `--level` (EG3D: 10) on the GPU over the same volume transposed (`render.shape_mesh_eg3d`), as `gen_samples.py --shapes
--shape-format .ply` writes it.  `--colors` adds per-vertex RGB: the first three decoder features at each vertex, mapped back
to world units.  `--normals` adds per-vertex unit normals (`property float nx ny nz`): the analytic −∇σ/‖∇σ‖ of the density field at
each vertex (`sample_mixed(normals=True)`), rotated into the same EG3D lattice frame as the vertices, pointing from dense to empty.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_seeds(text: str):
    """'0,3,5-7' -> [0, 3, 5, 6, 7]"""
    out = []
    for part in text.split(","):
        part = part.strip()
        if not part:
            continue
        if "-" in part:
            lo, hi = part.split("-", 1)
            out.extend(range(int(lo), int(hi) + 1))
        else:
            out.append(int(part))
    return out


def build_parser() -> argparse.ArgumentParser:
    from hfa_gp_amd.config import PRESETS
    p = argparse.ArgumentParser(description="Export generator head shapes as .mrc density volumes and / or .ply meshes (EG3D gen_samples --shapes).")
    p.add_argument("--preset", default="ffhq512_128", choices=sorted(PRESETS), help="generator topology")
    p.add_argument("--weights", default=None, help="safetensors file with EG3D key names (default: seeded random init)")
    p.add_argument("--generator-seed", type=int, default=0, help="init seed when no --weights are given")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--seeds", type=parse_seeds, help="latent seeds, e.g. '0-3' or '1,5,9'")
    src.add_argument("--ws", help=".npy file of ws [B, num_ws, w_dim]")
    p.add_argument("--trunc", type=float, default=1.0, help="truncation psi of the mapping (seeds only)")
    p.add_argument("--resolution", type=int, default=512, help="lattice points per axis")
    p.add_argument("--max-points", type=int, default=None, help="points per kernel launch (x slabs); default: one launch")
    p.add_argument("--format", default="mrc", choices=("mrc", "ply", "both"), help="density volume, surface mesh, or both")
    p.add_argument("--level", type=float, default=10.0, help="iso level of the .ply surface (EG3D: 10)")
    p.add_argument("--colors", action="store_true", help="per-vertex colours in the .ply")
    p.add_argument("--normals", action="store_true",
                   help="per-vertex unit normals (nx ny nz) in the .ply, for --format ply|both: the analytic density-field normal, in the "
                        "frame of the .ply's vertices (EG3D's lattice frame: world (x, y, z) -> (z, y, -x)), from dense to empty")
    p.add_argument("--outdir", required=True, help="output directory")
    return p


def frontal_label(device):
    import torch
    from hfa_gp_amd.cam_utils import create_cam2world_matrix, make_label
    pivot = torch.tensor([0.0, 0.0, 0.2], device=device)
    origin = pivot + torch.tensor([0.0, 0.0, 2.7], device=device)
    return make_label(create_cam2world_matrix((pivot - origin)[None], origin[None], device=device))


def eg3d_to_world(verts, n: int, cube: float):
    """EG3D .ply vertex (a, b, c) (indices of the flipped, transposed lattice) -> world point
    ((N-1-c) voxel - cube/2, b voxel - cube/2, a voxel - cube/2)"""
    import torch
    voxel = cube / (n - 1)
    a, b, c = verts.unbind(-1)
    return torch.stack([(n - 1 - c) * voxel, b * voxel, a * voxel], -1) - cube / 2


def world_to_eg3d_dir(d):
    """A world-space direction (x, y, z) in the frame of the EG3D .ply vertices (a, b, c): the axis permutation and flip of
    `eg3d_to_world` inverted, without its scale and offset: (a, b, c) = (z, y, -x)"""
    import torch
    x, y, z = d.unbind(-1)
    return torch.stack([z, y, -x], -1)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import load_G_official
    from hfa_gp_amd.render import save_mrc, save_ply, shape_mesh_eg3d, shape_volume_eg3d, to_uint8

    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = PRESETS[args.preset]()
    gen = load_G_official(cfg=cfg, seed=args.generator_seed, weights=args.weights, device=dev)
    os.makedirs(args.outdir, exist_ok=True)
    voxel = cfg.box_warp / (args.resolution - 1)
    with torch.no_grad():
        if args.seeds is not None:
            jobs = []
            for seed in args.seeds:
                z = torch.from_numpy(np.random.RandomState(seed).randn(1, cfg.z_dim)).float().to(dev)
                jobs.append((f"seed{seed:04d}", gen.mapping(z, frontal_label(dev), truncation_psi=args.trunc)))
        else:
            ws = torch.from_numpy(np.load(args.ws)).float().to(dev)
            stem = os.path.splitext(os.path.basename(args.ws))[0]
            jobs = [(f"{stem}_{b}", ws[b:b + 1]) for b in range(ws.shape[0])]
        for name, ws in jobs:
            grid = gen.density_grid(ws, resolution=args.resolution, max_points=args.max_points)[0]
            if args.format in ("mrc", "both"):
                path = os.path.join(args.outdir, name + ".mrc")
                save_mrc(path, shape_volume_eg3d(grid), voxel_size=voxel)
                print(path)
            if args.format in ("ply", "both"):
                verts, faces = shape_mesh_eg3d(grid, level=args.level)
                colors = normals = None
                if args.colors or args.normals:
                    world = eg3d_to_world(verts, args.resolution, cfg.box_warp)
                    q = gen.sample_mixed(world[None], None, ws, normals=args.normals)
                    if args.colors:
                        colors = to_uint8(q["rgb"][0, :, :3])
                    if args.normals:
                        normals = world_to_eg3d_dir(q["normal"][0])
                path = os.path.join(args.outdir, name + ".ply")
                save_ply(path, verts, faces, colors, normals)
                print(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
