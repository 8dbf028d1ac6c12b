"""Developer micro-benchmark of the occupancy-grid ray limits (run on the GPU box).
usage: bench_occupancy.py [--frames 1,8] [--calls 30] [--bwd-calls 8] [--warmup 5]

ffhq512_128 (48 + 48 samples), random weights, the list `cam_utils.ray_grid(c, 128)` in row order from radius 2.7 (16 384 rays per
frame), G = 64 with a SYNTHETIC ball mask of radius 0.3 — random weights carry no head, so the mask says nothing about a real one.
Device events around each call, the arms of a group alternating inside one process, median / minimum in ms (the protocol of
profiles/ray_limits/README.md).  Groups per frame count: the two limit kernels and the pack kernel alone; `render_rays` forward
under no_grad and forward + backward (d ws, the backbone's passes included) with ray_limits="box" — the parent's code path, which
this feature does not touch —, ray_limits=occ, and ray_limits=occ with compact=True."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops  # noqa: E402
from hfa_gp_amd.cam_utils import ray_grid  # noqa: E402
from hfa_gp_amd.config import ffhq512_128  # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator  # noqa: E402
from hfa_gp_amd.occupancy import OccupancyGrid  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--bwd-calls", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy.py needs the GPU")
    dev = torch.device("cuda:0")
    cfg = ffhq512_128()
    gen = TriPlaneGenerator(cfg, seed=0).requires_grad_(False).to(dev)
    res, g, k = cfg.neural_rendering_resolution, 64, 2
    x = (torch.arange(g) + 0.5) / g * cfg.box_warp - 0.5 * cfg.box_warp
    ball = torch.stack(torch.meshgrid(x, x, x, indexing="ij"), -1).norm(dim=-1) < 0.3
    for b in (int(t) for t in a.frames.split(",")):
        ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, b))
        us, ui = us.reshape(b, res * res, -1).contiguous(), ui.contiguous()
        o, d = (t.contiguous() for t in ray_grid(c, res))
        occ = OccupancyGrid.from_dense(ball[None].expand(b, -1, -1, -1).to(dev), cfg.box_warp)
        vol = torch.randn(b, g * k + 1, g * k + 1, g * k + 1, device=dev)
        tn, tf = ops.ray_limits_grid(o, d, occ)
        bn, bf = ops.ray_limits_box(o, d, cfg.box_warp)
        hit, box = torch.isfinite(tn), bf > bn
        print(f"B = {b}: {100 * hit.float().mean().item():.1f} % of the rays meet the mask ({100 * box.float().mean().item():.1f} % the cube); "
              f"mean chord {((tf - tn)[hit]).mean().item():.3f} against {((bf - bn)[box]).mean().item():.3f} of the cube", flush=True)
        groups = [("kernels", {"ray_limits_box": lambda: ops.ray_limits_box(o, d, cfg.box_warp),
                               "ray_limits_grid": lambda: ops.ray_limits_grid(o, d, occ),
                               "occupancy_pack": lambda: ops.occupancy_pack(vol, g, k, 0.0, 1)}, a.calls)]
        variants = {"box": dict(ray_limits="box"), "occ": dict(ray_limits=occ), "occ compact": dict(ray_limits=occ, compact=True)}

        def forward(kw):
            with torch.no_grad():
                gen.render_rays(ws, o, d, us, ui, **kw)

        def both(kw):
            w = ws.clone().requires_grad_(True)
            out = gen.render_rays(w, o, d, us, ui, **kw)
            (out["feature"].square().mean() + out["depth"].mean() + out["mask"].mean()).backward()

        groups.append(("render_rays forward", {n: (lambda kw=kw: forward(kw)) for n, kw in variants.items()}, a.calls))
        groups.append(("render_rays forward + backward", {n: (lambda kw=kw: both(kw)) for n, kw in variants.items()}, a.bwd_calls))
        for what, arms, calls in groups:
            out = run(arms, calls, a.warmup)
            print(f"B = {b} {what}: " + "; ".join(f"{n} {m:.4f} / {lo:.4f}" for n, (m, lo) in out.items()), flush=True)


if __name__ == "__main__":
    main()
