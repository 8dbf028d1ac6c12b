"""Developer micro-benchmark of the per-sample outputs of ray lists (run on the GPU box).
usage: bench_ray_samples.py [--frames 1,8] [--calls 30] [--bwd-calls 12] [--warmup 5]

ffhq512_128 (48 + 48 samples, the 16-bit decoder), random 256 x 256 planes, the list `cam_utils.ray_grid(c, 128)` in row order
(16 384 rays per frame): the protocol of profiles/ray_limits/README.md — the ops alone, device events around each call, the arms of
a group alternating inside one process, median / minimum in ms.  Groups per frame count: the forward (grid, list, list with
`state=`, and — where the tree has them — the two list forms with `samples=True`), the backward from the forward's state and the
backward recomputing pass 1 (grid, list, list with `g_weights=`), the rays' pass.  The script also runs from a tree that has no
`samples=` (it then times the arms that tree has), for a before / after of the calls without the keyword."""
import argparse
import inspect
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
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--bwd-calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_samples.py needs the GPU")
    has = "samples" in inspect.signature(ops.raymarch_rays).parameters
    print(f"tree {'with' if has else 'without'} samples=", flush=True)
    dev = torch.device("cuda:0")
    cfg = ffhq512_128()
    gen = TriPlaneGenerator(cfg, seed=0).requires_grad_(False).to(dev)
    res = cfg.neural_rendering_resolution
    r, s = res * res, cfg.depth_resolution + cfg.depth_resolution_importance
    for b in (int(x) for x in a.frames.split(",")):
        _, c, us, ui = (t.to(dev) for t in make_inputs(cfg, b))
        g = torch.Generator().manual_seed(1)
        planes = torch.randn(b, 3, 256, 256, 32, generator=g).to(dev)
        us, ui = us.reshape(b, r, -1).contiguous(), ui.contiguous()
        g_feat = torch.randn(b, r, 32, generator=g).to(dev)
        g_w = torch.randn(b, r, s - 1, generator=g).to(dev)
        pam = ops._decoder_bound(planes, cfg.decoder_precision, None)
        grid_kw = dict(gen._render_args(c), u_strat=us, u_imp=ui, planes_absmax=pam)
        o, d = (t.contiguous() for t in ray_grid(c, res))
        list_kw = dict(gen._rays_kwargs(), planes_absmax=pam)
        st_grid = ops.raymarch_state(b, res, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
        st_list = ops.raymarch_rays_state(b, r, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
        fwd = {"grid": lambda: ops.raymarch(planes, **grid_kw),
               "grid state": lambda: ops.raymarch(planes, state=st_grid, **grid_kw),
               "list": lambda: ops.raymarch_rays(planes, o, d, us, ui, **list_kw),
               "list state": lambda: ops.raymarch_rays(planes, o, d, us, ui, state=st_list, **list_kw)}
        if has:
            fwd["list samples"] = lambda: ops.raymarch_rays(planes, o, d, us, ui, samples=True, **list_kw)
            fwd["list state samples"] = lambda: ops.raymarch_rays(planes, o, d, us, ui, state=st_list, samples=True, **list_kw)
            out = fwd["list state samples"]()
            ref = fwd["list state"]()
            print(f"B = {b}: samples=True keeps the other outputs' bits: {all(torch.equal(x, y) for x, y in zip(ref, out))}; "
                  f"max |sum w - wsum| {float((out[4].sum(-1) - out[2]).abs().max()):.3e}", flush=True)
        # (the gradients go into buffers made once: no allocation or memset of them inside the timed calls)
        outb = (torch.zeros_like(planes), torch.empty(b, r, s, 4, device=dev))
        groups = [("forward", fwd, a.calls)]
        for name, st_g, st_l in (("backward, state", st_grid, st_list), ("backward, recompute", None, None)):
            arms = {"grid": lambda sg=st_g: ops.raymarch_bwd(g_feat, planes, state=sg, _out=outb, **grid_kw),
                    "list": lambda sl=st_l: ops.raymarch_rays_bwd(g_feat, planes, o, d, us, ui, state=sl, _out=outb, **list_kw)}
            if has:
                arms["list g_weights"] = lambda sl=st_l: ops.raymarch_rays_bwd(g_feat, planes, o, d, us, ui, state=sl, _out=outb,
                                                                              g_weights=g_w, **list_kw)
            groups.append((name, arms, a.bwd_calls))
        groups.append(("rays' pass", {"list": lambda: ops.raymarch_rays_bwd_rays(g_feat, planes, outb[1], o, d, us, ui, **list_kw)},
                       a.bwd_calls))
        for what, arms, calls in groups:
            res_ = run(arms, calls, a.warmup)
            print(f"B = {b} {what}: " + "; ".join(f"{k} {m:.4f} / {lo:.4f}" for k, (m, lo) in res_.items()), flush=True)


if __name__ == "__main__":
    main()
