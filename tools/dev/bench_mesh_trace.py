"""Developer micro-benchmark of mesh tracing (run on the GPU box).
usage: bench_mesh_trace.py [--calls 30] [--warmup 3] [--brute 10000,70000,1000000] [--heads 128,256] [--grids 32,64,128]

ffhq512_128, random weights, the list `cam_utils.ray_grid(c, 128)` in row order from radius 2.7 (16 384 rays, one frame).
Device events around each call, the arms of a group alternating inside one process, median / minimum in ms.
  * brute force (`ops.trace_mesh` without a grid) on latitude-longitude spheres of radius 0.3 with about the asked face counts,
    next to the pair tests per second they stand for;
  * the grid on `extract_mesh` heads at the asked lattice resolutions (level = the 0.9 quantile of a 64-cubed density lattice:
    random weights carry no head, so the face count and the share of hits are printed), at the asked G and at
    `build_grid`'s default, with the pairs per face, the build time (host clock around a synchronised build) and the brute-force
    time on the same mesh; every grid result is compared with the brute-force one, and every ray on which the two differ is
    classified in float64 (`classify`): is brute force's winner a candidate of the float64 definition at all (no: a PHANTOM of
    float32 rounding), and is the grid's winner the float64 winner;
  * the median |t_mesh − t_iso| against `trace_rays` at the same level over the rays both hit, in voxels of the lattice, and
    `trace_rays`' and `render_rays`' times on the same list (`render_rays` also runs on a tree from before this feature)."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd.cam_utils import ray_grid  # noqa: E402
from hfa_gp_amd.config import ffhq512_128  # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator  # noqa: E402
from hfa_gp_amd.synthetic import make_inputs  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(arms, calls, warmup):
    times = {k: [] for k in arms}
    for i in range(warmup + calls):
        for name, fn in arms.items():
            t = timed(fn)
            if i >= warmup:
                times[name].append(t)
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}


def show(what, res):
    print(f"{what}: " + "; ".join(f"{n} {m:.4f} / {lo:.4f}" for n, (m, lo) in res.items()), flush=True)


def uv_sphere(n_faces, radius, dev):
    """a closed latitude-longitude sphere of 4 n² − 4 n faces ≈ n_faces, wound counter-clockwise seen from outside"""
    n = max(3, int(round(math.sqrt(n_faces / 4.0))))
    lat = torch.linspace(0, math.pi, n + 1, device=dev)[1:-1]
    lon = torch.arange(2 * n, device=dev) * (math.pi / n)
    ring = torch.stack((torch.sin(lat)[:, None] * torch.cos(lon)[None], torch.cos(lat)[:, None].expand(-1, 2 * n),
                        torch.sin(lat)[:, None] * torch.sin(lon)[None]), -1).reshape(-1, 3)
    verts = torch.cat((ring, torch.tensor([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], device=dev))) * radius
    i = torch.arange(n - 2, device=dev)[:, None] * (2 * n)
    j = torch.arange(2 * n, device=dev)[None]
    jn = (j + 1) % (2 * n)
    a, b, c, d = i + j, i + jn, i + 2 * n + j, i + 2 * n + jn
    quads = torch.cat((torch.stack((a, b, c), -1).reshape(-1, 3), torch.stack((b, d, c), -1).reshape(-1, 3)))
    top, bot, last = ring.shape[0], ring.shape[0] + 1, (n - 2) * 2 * n
    caps = torch.cat((torch.stack((torch.full_like(j[0], top), jn[0], j[0]), -1),
                      torch.stack((torch.full_like(j[0], bot), last + j[0], last + jn[0]), -1)))
    return verts.float(), torch.cat((quads, caps)).to(torch.int32)


def classify(M, m, o, d, brute, out):
    """The rays on which a grid run and the brute-force run differ, judged by the float64 definition on the same float32 inputs:
    (differing rays, of them: brute force's winner is NOT a float64 candidate, the grid's result IS the float64 result (same
    face, or both a miss), brute force's result is the float64 result)."""
    bad = torch.zeros_like(out["face"][0], dtype=torch.bool)
    for k in out:
        bad |= (out[k] != brute[k]).reshape(1, bad.shape[0], -1).any(-1)[0]
    n = int(bad.sum())
    if n == 0:
        return 0, 0, 0, 0
    ob, db = o[:, bad].double().contiguous(), d[:, bad].double().contiguous()
    v64 = m.vertices.double()
    ref = M.trace_mesh_reference(v64, m.faces, ob, db)
    fb, fg = brute["face"][:, bad].long(), out["face"][:, bad].long()
    ids = m.faces.long()[fb.clamp(min=0)]
    a, b, c = (torch.gather(v64.expand(1, -1, -1), 1, ids[..., k:k + 1].expand(-1, -1, 3)) for k in range(3))
    U, V, W, det, _, dn, t = M._face_terms(ob, db, a, b, c)
    cand = M._candidate(U, V, W, det, dn, t, 0.0, float("inf")) & (fb >= 0)
    return n, int((~cand).sum()), int((fg == ref["face"].long()).sum()), int((fb == ref["face"].long()).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--brute", default="10000,70000,1000000")
    ap.add_argument("--heads", default="128,256")
    ap.add_argument("--grids", default="32,64,128")
    ap.add_argument("--yardsticks", action="store_true", help="only render_rays (runs on a tree from before this feature)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_trace.py needs the GPU")
    dev = torch.device("cuda:0")
    cfg = ffhq512_128()
    gen = TriPlaneGenerator(cfg, seed=0).requires_grad_(False).to(dev)
    res = cfg.neural_rendering_resolution
    ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, 1))
    us, ui = us.reshape(1, res * res, -1).contiguous(), ui.contiguous()
    o, d = (t.contiguous() for t in ray_grid(c, res))
    n_rays = o.shape[1]
    tn, tf = torch.zeros(1, n_rays, device=dev), torch.full((1, n_rays), float("inf"), device=dev)
    with torch.no_grad():
        if a.yardsticks:
            show("yardstick", run({"render_rays": lambda: gen.render_rays(ws, o, d, us, ui)}, a.calls, a.warmup))
            return
        from hfa_gp_amd import mesh as M                        # (below the yardstick: a tree from before this feature has none)
        from hfa_gp_amd import ops
        for nf in (int(t) for t in a.brute.split(",") if t):
            v, f = uv_sphere(nf, 0.3, dev)
            m = M.TriangleMesh(v, f)
            out = ops.trace_mesh(m.tri, o, d, tn, tf)
            calls = max(3, min(a.calls, int(2e10 / (n_rays * m.num_faces))))
            r = run({"brute": lambda: ops.trace_mesh(m.tri, o, d, tn, tf)}, calls, 1)
            pairs = n_rays * m.num_faces
            print(f"brute force, {m.num_faces} faces x {n_rays} rays ({100 * out['hit'].float().mean().item():.1f} % hit): "
                  f"{r['brute'][0]:.4f} / {r['brute'][1]:.4f} ms over {calls} calls = {pairs / r['brute'][0] * 1e-6:.1f} G pair tests / s",
                  flush=True)
        level = float(torch.quantile(gen.density_grid(ws, 64).flatten(), 0.9))
        for n in (int(t) for t in a.heads.split(",") if t):
            m = M.TriangleMesh.from_dict(gen.extract_mesh(ws, resolution=n, level=level)[0])
            brute = ops.trace_mesh(m.tri, o, d, tn, tf)
            hit = brute["hit"].bool()
            print(f"head at {n}^3, level {level:.3f}: {m.num_faces} faces, {100 * hit.float().mean().item():.1f} % of the rays hit",
                  flush=True)
            arms = {}
            if n_rays * m.num_faces <= 4e9:
                arms["brute"] = lambda: ops.trace_mesh(m.tri, o, d, tn, tf)
            for g in [None] + [int(t) for t in a.grids.split(",") if t]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                grid = m.build_grid(g)
                torch.cuda.synchronize()
                build = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                m.build_grid(g)
                torch.cuda.synchronize()
                build2 = (time.perf_counter() - t0) * 1e3
                out = ops.trace_mesh(m.tri, o, d, tn, tf, grid=grid)
                n_bad, phantom, grid_ok, brute_ok = classify(M, m, o, d, brute, out)
                name = f"G = {grid[3]}" + (" (default)" if g is None else "")
                print(f"  {name}: {grid[1].shape[0] / m.num_faces:.2f} pairs per face, build {build:.1f} ms first / {build2:.1f} ms "
                      f"again; {n_bad} of {n_rays} rays differ from brute force: on {phantom} brute force's face is no float64 "
                      f"candidate, on {grid_ok} the grid's answer is the float64 one, on {brute_ok} brute force's is", flush=True)
                arms[name] = (lambda gr: lambda: ops.trace_mesh(m.tri, o, d, tn, tf, grid=gr))(grid)
            show(f"head at {n}^3", run(arms, a.calls, a.warmup))
            tr = gen.trace_rays(ws, o, d, level=level, ray_limits="box", normals=False)
            both = hit & tr["hit"].bool()
            voxel = cfg.box_warp / (n - 1)
            dt = (brute["t"] - tr["t"]).abs()[both] / voxel
            print(f"  against trace_rays (steps 128, refine 8, box limits) at the same level: {int(both.sum())} rays hit both, "
                  f"{int((hit ^ tr['hit'].bool()).sum())} only one; |t_mesh - t_iso| median {dt.median().item():.4f}, "
                  f"90 % {dt.quantile(0.9).item():.4f}, max {dt.max().item():.3f} voxels", flush=True)
        show("same list", run({"trace_rays": lambda: gen.trace_rays(ws, o, d, level=level, ray_limits="box", normals=False),
                               "render_rays": lambda: gen.render_rays(ws, o, d, us, ui)}, a.calls, a.warmup))


if __name__ == "__main__":
    main()
