"""Developer micro-benchmark of the normals ops on ray lists against the grid ops on the same rays (run on the GPU box).
usage: bench_rays_normals.py [--frames 1,8] [--calls 30] [--warmup 5] [--grid-only]

ffhq512_128 (48 + 48 samples, the 16-bit decoder), random 256 x 256 planes, the list `cam_utils.ray_grid(c, 128)` in row order
(16 384 rays per frame).  Per frame count and per op — normals, normals_bwd (with the decoder gradients), normals_bwd_camera without
its reduction / normals_bwd_rays — three arms alternate inside one process, each call between device events: the grid op, the list
op, the list op with limits equal to the config's constant range.  Prints median / minimum in ms per arm and the ratios of the
medians; with --grid-only the grid arm alone (this script also runs from a tree that has no list ops, for a before / after of the
grid kernels).  The forward outputs of the arms are compared first: max |list - grid| and max |limits - list| of the normal."""
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
    """arms: {name: callable}; the arms alternate call by call -> {name: (median, minimum)} in ms."""
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rays_normals.py needs the GPU")
    dev = torch.device("cuda:0")
    cfg = ffhq512_128()
    gen = TriPlaneGenerator(cfg, seed=0).requires_grad_(False).to(dev)
    res = cfg.neural_rendering_resolution
    for b in (int(x) for x in a.frames.split(",")):
        _, c, us, ui = (t.to(dev) for t in make_inputs(cfg, b))
        g = torch.Generator().manual_seed(1)
        planes = torch.randn(b, 3, 256, 256, 32, generator=g).to(dev)
        us, ui = us.reshape(b, res * res, -1).contiguous(), ui.contiguous()
        g_n = torch.randn(b, res * res, 3, generator=g).to(dev)
        pam = ops._decoder_bound(planes, cfg.decoder_precision, None)
        # (the gradients accumulate into buffers made once: no allocation or memset inside the timed calls)
        acc = dict(d_planes=torch.zeros_like(planes), decoder_grads=True, dec_out=tuple(torch.zeros_like(t) for t in gen.decoder_params()))
        grid_kw = dict(gen._render_args(c), u_strat=us, u_imp=ui, planes_absmax=pam)
        st_grid = ops.raymarch_state(b, res, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
        ops.raymarch(planes, state=st_grid, **grid_kw)
        n_grid = ops.raymarch_normals(planes, st_grid, **grid_kw)
        fwd = {"grid": lambda: ops.raymarch_normals(planes, st_grid, **grid_kw)}
        bwd = {"grid": lambda: ops.raymarch_normals_bwd(g_n, planes, st_grid, **acc, **grid_kw)}
        ray = {"grid": lambda: ops.raymarch_normals_bwd_camera(g_n, planes, st_grid, reduce=False, **grid_kw)}
        if not a.grid_only:
            o, d = ray_grid(c, res)
            kw = dict(gen._rays_kwargs(), ray_origins=o.contiguous(), ray_directions=d.contiguous(), u_strat=us, u_imp=ui,
                      planes_absmax=pam)
            march = {k: v for k, v in kw.items() if k not in ("ray_origins", "ray_directions", "u_strat", "u_imp")}
            lim = dict(t_near=torch.full((b, res * res), float(cfg.ray_start), device=dev),
                       t_far=torch.full((b, res * res), float(cfg.ray_end), device=dev))
            st = {}
            for name, extra in (("list", {}), ("limits", lim)):
                st[name] = ops.raymarch_rays_state(b, res * res, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
                ops.raymarch_rays(planes, kw["ray_origins"], kw["ray_directions"], us, ui, state=st[name], **extra, **march)
                fwd[name] = lambda n=name, e=extra: ops.raymarch_rays_normals(planes, st[n], **e, **kw)
                bwd[name] = lambda n=name, e=extra: ops.raymarch_rays_normals_bwd(g_n, planes, st[n], **acc, **e, **kw)
                ray[name] = lambda n=name, e=extra: ops.raymarch_rays_normals_bwd_rays(g_n, planes, st[n], **e, **kw)
            n_list, n_lim = fwd["list"](), fwd["limits"]()
            print(f"B = {b}: max |N| {float(n_grid.abs().max()):.3e}; max |list - grid| {float((n_list - n_grid).abs().max()):.3e} "
                  f"(bit-equal {torch.equal(n_list, n_grid)}); max |limits - list| {float((n_lim - n_list).abs().max()):.3e}", flush=True)
        for what, arms in (("normals", fwd), ("normals_bwd", bwd), ("normals_bwd_rays / _camera", ray)):
            r = run(arms, a.calls, a.warmup)
            line = f"B = {b} {what}: " + "; ".join(f"{k} {m:.4f} / {lo:.4f}" for k, (m, lo) in r.items())
            if not a.grid_only:
                line += f"; list / grid {r['list'][0] / r['grid'][0]:.3f}, limits / list {r['limits'][0] / r['list'][0]:.3f}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
