"""Developer micro-benchmark of surface tracing (run on the GPU box).
usage: bench_trace_rays.py [--frames 1,8] [--calls 50] [--warmup 5] [--steps 128] [--refine 8] [--yardsticks]

ffhq512_128, random weights, the list `cam_utils.ray_grid(c, 128)` in row order from radius 2.7 (16 384 rays per frame) on the
config's interval; level = the 0.9 quantile of a 64-cubed density lattice of frame 0 — random weights carry no head, so the share of
hits and the mean cell are printed next to every time and say how much of the march the figures stand for.
Device events around each call, the arms of a group alternating inside one process, median / minimum in ms.  Groups per frame
count: the kernel alone (`ops.trace_rays` on ready planes) with and without normals next to `ops.raymarch_rays` on the same list —
the yardstick —; then the whole calls under no_grad, backbone pass included: `trace_rays`, `render_rays`, `sample_mixed` at the
same number of points.  --yardsticks: only the last two, which also run on a tree from before this feature (A/B against the parent:
start the two trees in turn)."""
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
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--refine", type=int, default=8)
    ap.add_argument("--yardsticks", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trace_rays.py needs the GPU")
    dev = torch.device("cuda:0")
    cfg = ffhq512_128()
    gen = TriPlaneGenerator(cfg, seed=0).requires_grad_(False).to(dev)
    res = cfg.neural_rendering_resolution
    for b in (int(t) for t in a.frames.split(",")):
        ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, b))
        us, ui = us.reshape(b, res * res, -1).contiguous(), ui.contiguous()
        o, d = (t.contiguous() for t in ray_grid(c, res))
        groups = []
        with torch.no_grad():
            pts = (o + 0.5 * (cfg.ray_start + cfg.ray_end) * d).contiguous()
            calls = {"render_rays": lambda: gen.render_rays(ws, o, d, us, ui), "sample_mixed": lambda: gen.sample_mixed(pts, None, ws)}
            if not a.yardsticks:
                level = float(torch.quantile(gen.density_grid(ws[:1], 64).flatten(), 0.9))
                planes, pam = gen._query_planes(ws)
                tn = torch.full((b, res * res), float(cfg.ray_start), device=dev)
                tf = torch.full((b, res * res), float(cfg.ray_end), device=dev)
                plain = tuple(k for k in ops._TRACE_OUT if k not in ("sigma_grad", "normal"))
                out = ops.trace_rays(planes, o, d, tn, tf, level, a.steps, a.refine, pam, **gen._query_kwargs())
                hit, cell = out["hit"].bool(), out["cell"]
                print(f"B = {b}: level {level:.3f}, {100 * hit.float().mean().item():.1f} % of the rays hit, mean cell of a hit "
                      f"{cell[hit].float().mean().item():.1f} of {a.steps}, {100 * (cell == 0).float().mean().item():.1f} % start inside",
                      flush=True)
                groups.append(("kernels", {
                    "trace_rays normals": lambda: ops.trace_rays(planes, o, d, tn, tf, level, a.steps, a.refine, pam, **gen._query_kwargs()),
                    "trace_rays plain": lambda: ops.trace_rays(planes, o, d, tn, tf, level, a.steps, a.refine, pam, plain,
                                                               **gen._query_kwargs()),
                    "trace_rays all miss": lambda: ops.trace_rays(planes, o, d, tn, tf, 1e30, a.steps, a.refine, pam, plain,
                                                                  **gen._query_kwargs()),
                    "raymarch_rays": lambda: ops.raymarch_rays(planes, o, d, us, ui, planes_absmax=pam, **gen._rays_kwargs())}))
                calls = {"trace_rays": lambda: gen.trace_rays(ws, o, d, level, a.steps, a.refine),
                         "trace_rays normals=False": lambda: gen.trace_rays(ws, o, d, level, a.steps, a.refine, normals=False), **calls}
            groups.append(("calls", calls))
            for what, arms in groups:
                res_ = run(arms, a.calls, a.warmup)
                print(f"B = {b} {what}: " + "; ".join(f"{n} {m:.4f} / {lo:.4f}" for n, (m, lo) in res_.items()), flush=True)


if __name__ == "__main__":
    main()
