"""Developer timing of synthesis(neural_rendering_resolution=N) (GPU box), ffhq512_128.
usage: bench_resample.py kernels [iters] [runs]     ops.resize_aa and ops.resize_aa_bwd (with g_nchw3) alone at the preset's sizes,
                                                    [B,256,256,32] -> 128^2 and [B,64,64,32] -> 128^2 for B = 1 and 8: HIP events
                                                    around `iters` calls after warm-up, median of `runs` runs, and the rate of the
                                                    algorithmic bytes B (N^2 + 128^2) 128 against the 6.29 TB/s measured-copy ceiling
       bench_resample.py synthesis [steps] [runs]   synthesis under no_grad at N = 64, 128, 256 for 1 and 8 frames: median ms per
                                                    step of each run, arms alternating
       bench_resample.py fit [steps] [runs]         the 2-frame latent fitting step (ws requires grad, generator frozen, mse on the
                                                    image, forward + backward) at N = 64 and N = 128, arms alternating"""
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops                                  # noqa: E402
from hfa_gp_amd.config import ffhq512_128                   # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator          # noqa: E402
from hfa_gp_amd.synthetic import make_inputs, perturb_state  # noqa: E402

COPY_CEILING = 6.29e12      # bytes / s, SURVEY.md section 8d
mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
n1 = int(sys.argv[2]) if len(sys.argv) > 2 else 20
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
cfg = ffhq512_128()
R0 = cfg.neural_rendering_resolution


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


def steps_per_run(arms, steps):
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
    gc.enable()
    return res


def inputs(b, n):
    ws, c, us, ui = make_inputs(cfg, b)
    g = torch.Generator().manual_seed(n)
    us = torch.rand(b, n * n, cfg.depth_resolution, 1, generator=g)
    ui = torch.rand(b * n * n, cfg.depth_resolution_importance, generator=g)
    return [t.to(dev) for t in (ws, c, us, ui)]


if mode == "kernels":
    g = torch.Generator().manual_seed(0)
    for b in (1, 8):
        for n in (256, 64):
            x = torch.randn(b, n, n, 32, generator=g).to(dev)
            gy = torch.randn(b, R0, R0, 32, generator=g).to(dev)
            g3 = torch.randn(b, 3, n, n, generator=g).to(dev)
            arms = {"resize_aa": lambda: ops.resize_aa(x, (R0, R0)), "resize_aa_bwd": lambda: ops.resize_aa_bwd(gy, (n, n), g_nchw3=g3)}
            nbytes = b * (n * n + R0 * R0) * 128
            for name, call in arms.items():
                for _ in range(5):
                    call()
                torch.cuda.synchronize()
                ms = [timed(call, n1) for _ in range(runs)]
                m = median(ms)
                print(f"B={b} {n}^2 <-> {R0}^2 {name}: ms per call of each run " + ", ".join(f"{v:.4f}" for v in ms) +
                      f"; median {m * 1e3:.1f} us, {nbytes / 2**20:.1f} MiB algorithmic = {nbytes / (m * 1e-3) / 1e12:.2f} TB/s "
                      f"({100 * nbytes / (m * 1e-3) / COPY_CEILING:.0f} % of the copy ceiling; at the ceiling {nbytes / COPY_CEILING * 1e6:.1f} us)")
elif mode == "synthesis":
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    with torch.no_grad():
        for b in (1, 8):
            arms = []
            for n in (64, 128, 256):
                ws, c, us, ui = inputs(b, n)
                arms.append((f"N={n}", lambda ws=ws, c=c, us=us, ui=ui, n=n: gen.synthesis(
                    ws, c, noise_mode="const", u_strat=us, u_imp=ui, neural_rendering_resolution=n)["image"]))
            for name, v in steps_per_run(arms, n1).items():
                print(f"B={b} synthesis (no_grad) {name}: median ms per step of each run: " + ", ".join(f"{x:.3f}" for x in v))
else:
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    target = torch.randn(2, 3, cfg.img_resolution, cfg.img_resolution, generator=torch.Generator().manual_seed(1)).clamp(-1, 1).to(dev)
    arms = []
    for n in (64, 128):
        ws, c, us, ui = inputs(2, n)
        ws.requires_grad_(True)

        def step(ws=ws, c=c, us=us, ui=ui, n=n):
            ws.grad = None
            img = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, neural_rendering_resolution=n)["image"]
            torch.nn.functional.mse_loss(img, target).backward()

        arms.append((f"N={n}", step))
    for name, v in steps_per_run(arms, n1).items():
        print(f"B=2 fitting step (d ws, generator frozen, forward + backward) {name}: median ms per step of each run: " +
              ", ".join(f"{x:.3f}" for x in v))
    print(f"peak memory {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")
