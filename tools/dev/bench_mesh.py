"""Marching-cubes extraction (marching_cubes.hip) on one GPU, in one process (run on the GPU box), at N = 256 and 512:

  * `field`: a synthetic sphere + torus distance field (level 0);
  * `head`: an ffhq512_128 density grid (seeded random init, EG3D's border trim), level = median of the untrimmed interior
    (random weights put no surface at EG3D's level 10).

Per workload: the count phase (count + scan kernels) and the emit phase (HIP events around each; emit includes its read-back of
the two counts), `ops.marching_cubes` end to end (device-synchronised wall clock: count, count read-back, allocation, emit),
the vertex and face counts, and GB/s of the N^3 x 4-byte volume read per phase.

    python tools/dev/bench_mesh.py [reps] [out.json]
"""
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import _lib as L  # noqa: E402
from hfa_gp_amd import ops  # noqa: E402
from hfa_gp_amd.config import ffhq512_128  # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator  # noqa: E402
from hfa_gp_amd.render import _border_eg3d  # noqa: E402
from hfa_gp_amd.synthetic import perturb_state  # noqa: E402


def field(n, dev):
    g = torch.arange(n, device=dev, dtype=torch.float32) * (64.0 / (n - 1)) - 32.0
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    sphere = 12.0 - ((x - 12) ** 2 + y ** 2 + z ** 2).sqrt()
    torus = 5.0 - (((x + 10) ** 2 + y ** 2).sqrt() - 14.0).square().add(z ** 2).sqrt()
    return torch.maximum(sphere, torus).contiguous()


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        ts.append(fn())
    ts.sort()
    return ts[len(ts) // 2]


def phases(vol, level, reps):
    h = L.lib()
    n0, n1, n2 = vol.shape
    ws = torch.empty(h.hfagp_marching_cubes_workspace_bytes(n0, n1, n2) // 8, device=vol.device, dtype=torch.int64)
    counts = torch.zeros(2, device=vol.device, dtype=torch.int64)
    a = L.MarchingCubesArgs()
    a.volume, a.workspace, a.counts, a.workspace_bytes = vol.data_ptr(), ws.data_ptr(), counts.data_ptr(), ws.numel() * 8
    a.n0, a.n1, a.n2, a.level = n0, n1, n2, level
    a.spacing[:] = [1.0, 1.0, 1.0]
    L.check(h.hfagp_marching_cubes_count(C.byref(a), ops._stream()), "count")
    nv, nf = (int(x) for x in counts.cpu())
    verts = torch.empty(nv, 3, device=vol.device)
    faces = torch.empty(nf, 3, device=vol.device, dtype=torch.int32)
    a.verts, a.faces, a.vert_capacity, a.face_capacity = verts.data_ptr(), faces.data_ptr(), nv, nf

    def ev(call):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.check(call(C.byref(a), ops._stream()), "mc")
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        return run

    def e2e():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.marching_cubes(vol, level)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    count_ms = median_ms(ev(h.hfagp_marching_cubes_count), reps)
    emit_ms = median_ms(ev(h.hfagp_marching_cubes_emit), reps)
    total_ms = median_ms(e2e, reps)
    gb = vol.numel() * 4 / 1e9
    return {"level": level, "vertices": nv, "faces": nf, "count_ms": count_ms, "emit_ms": emit_ms, "end_to_end_ms": total_ms,
            "volume_GB": gb, "count_GBps": gb / count_ms * 1e3, "emit_GBps": gb / emit_ms * 1e3,
            "output_MB": (nv * 12 + nf * 12) / 1e6}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    dev = torch.device("cuda:0")
    cfg = ffhq512_128()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    ws = torch.randn(1, cfg.num_ws, cfg.w_dim, generator=torch.Generator().manual_seed(5)).to(dev)
    res = {}
    with torch.no_grad():
        for n in (256, 512):
            res[f"field_{n}"] = phases(field(n, dev), 0.0, reps)
            grid = gen.density_grid(ws, resolution=n)[0]
            p = int(30 * n / 256)
            level = float(grid[p:n - p, p:n - p, p:n - p].median())
            res[f"head_{n}"] = phases(_border_eg3d(grid), level, reps)
            del grid
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
