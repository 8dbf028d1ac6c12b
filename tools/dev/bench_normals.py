"""Developer timing of the per-ray surface normals (GPU box), ffhq512_128, B frames.
usage: bench_normals.py kernels [B] [iters] [runs]  ops.raymarch (forward ray marcher, leaving its state) and ops.raymarch_normals on
                                                    the same inputs in the same process, HIP events around `iters` calls of each,
                                                    arms alternating, `runs` runs; prints every run's ms per call and the ratio of
                                                    the medians
       bench_normals.py render [B] [steps] [runs]   the render step bench.py times (synthesis under no_grad, no `normals`): median
                                                    ms per step of each run.  Uses nothing this feature added, so the same file
                                                    runs on the parent commit for the A/B
       bench_normals.py synthesis [B] [steps] [runs]  synthesis under no_grad without and with normals=True, arms alternating"""
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops                                  # noqa: E402
from hfa_gp_amd.config import ffhq512_128                   # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator          # noqa: E402
from hfa_gp_amd.synthetic import make_inputs, perturb_state  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1
dev = torch.device("cuda:0")
cfg = ffhq512_128()
gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
ws, c, us, ui = [t.to(dev) for t in make_inputs(cfg, B)]


def median(v):
    return sorted(v)[len(v) // 2]


def timed(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def steps_per_run(arms, steps, runs):
    for _ in range(3):
        for _, call in arms:
            call()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    res = {name: [] for name, _ in arms}
    for _ in range(runs):
        for name, call in arms:
            per = []
            for _ in range(steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                per.append((e0, e1))
            torch.cuda.synchronize()
            res[name].append(median([a.elapsed_time(b) for a, b in per]))
    return res


with torch.no_grad():
    if mode == "kernels":
        iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
        runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
        res = cfg.neural_rendering_resolution
        planes = gen.backbone_planes(ws)
        u_s, u_i = gen._uniforms(B, dev, us, ui)
        kw = gen._render_args(c)
        pam = getattr(gen, "_planes_absmax", None)
        st = ops.raymarch_state(B, res, cfg.depth_resolution, cfg.depth_resolution_importance, dev)

        def forward():
            return ops.raymarch(planes, u_strat=u_s, u_imp=u_i, planes_absmax=pam, state=st, **kw)

        def normals():
            return ops.raymarch_normals(planes, st, u_strat=u_s, u_imp=u_i, planes_absmax=pam, **kw)

        for _ in range(3):
            wsum = forward()[2]
            out = normals()
        torch.cuda.synchronize()
        ms = {"raymarch": [], "raymarch_normals": []}
        for _ in range(runs):
            ms["raymarch"].append(timed(forward, iters))
            ms["raymarch_normals"].append(timed(normals, iters))
        nrm = out.norm(dim=-1)
        f, n = median(ms["raymarch"]), median(ms["raymarch_normals"])
        print(f"B={B} ({B * res * res} rays x {cfg.depth_resolution + cfg.depth_resolution_importance} samples, {st.numel() * 4 / 2**30:.2f} GiB of "
              f"state), ms per call of each run: raymarch (with state) " + ", ".join(f"{x:.3f}" for x in ms["raymarch"]) +
              "; raymarch_normals " + ", ".join(f"{x:.3f}" for x in ms["raymarch_normals"]) +
              f"; medians {f:.3f} / {n:.3f} ms, normals / forward = {n / f:.2f}; repeatable bits: {torch.equal(out, normals())}; "
              f"max |N| {nrm.max().item():.3f}, max (|N| - wsum) {(nrm - wsum).max().item():.2e}")
    else:
        steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
        runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
        arms = [("render step", lambda: gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)["image"])]
        if mode == "synthesis":
            arms.append(("render step with normals=True", lambda: gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui,
                                                                                normals=True)["image_normal"]))
        for name, v in steps_per_run(arms, steps, runs).items():
            print(f"B={B} {name} (synthesis, no_grad): median ms per step of each run: " + ", ".join(f"{x:.3f}" for x in v))
