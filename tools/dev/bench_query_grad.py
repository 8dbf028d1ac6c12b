"""Developer timing of the point-query backward (GPU box).
usage: bench_query_grad.py kernels [B] [iters]   ops.planes_query (forward) beside ops.planes_query_bwd, every instance
                                                 ({f16x3, fp32} x {planes only, + decoder gradients, + point gradient}), at
                                                 M = 2000 (EG3D's density-regularisation size) and M = 2^20, on ffhq512_128's
                                                 256^2 planes; HIP events around the calls
       bench_query_grad.py step [B] [steps] [runs]
                                                 forward + backward of one fitting-style step on the generator (ffhq512_128, ws a
                                                 leaf, image MSE), generator frozen and tuned, three forms, arms alternating:
                                                   image      synthesis alone
                                                   joined     synthesis(query=) with 2 x 1000 points + EG3D's density L1
                                                   separate   synthesis + stand-alone sample_mixed(differentiable=True), one backward
                                                 separate - joined is the backbone pass the joined form saves.
The image arm runs the code path bench.py times; for the A/B against the parent commit run tools/dev/bench_camera_grad.py step
... plain (which exists on both sides) from each tree."""
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops                                  # noqa: E402
from hfa_gp_amd.config import ffhq512_128                   # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator          # noqa: E402
from hfa_gp_amd.synthetic import make_inputs, perturb_state    # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 2
dev = torch.device("cuda:0")


def timed(call, iters):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


if mode == "kernels":
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    cfg = ffhq512_128()
    gen = TriPlaneGenerator(cfg, seed=0).to(dev)
    ws = make_inputs(cfg, B)[0].to(dev)
    with torch.no_grad():
        planes = gen.backbone_planes(ws)
        pam = getattr(gen, "_planes_absmax", None)
        d_planes = torch.zeros_like(planes)
        for m in (2000, 1 << 20):
            g = torch.Generator().manual_seed(m)
            coords = ((torch.rand(B, m, 3, generator=g) * 2 - 1) * (cfg.box_warp / 2)).to(dev)
            gs, gr = torch.randn(B, m, 1, generator=g).to(dev), torch.randn(B, m, 32, generator=g).to(dev)
            for prec in ("f16x3", "fp32"):
                kw = dict(gen._query_kwargs(), decoder_precision=prec, planes_absmax=pam if prec == "f16x3" else None)
                fwd = timed(lambda: ops.planes_query(planes, coords, **kw), iters)
                line = [f"forward {fwd * 1e3:9.1f} us"]
                for name, extra in (("planes", {}), ("planes+dec", dict(decoder_grads=True)), ("planes+coords", dict(coords_grad=True)),
                                    ("planes+dec+coords", dict(decoder_grads=True, coords_grad=True)),
                                    ("coords only", dict(d_planes=False, coords_grad=True))):
                    if "d_planes" not in extra:
                        extra = dict(extra, d_planes=d_planes)
                    ms = timed(lambda: ops.planes_query_bwd(planes, coords, gs, gr, **kw, **extra), iters)
                    line.append(f"{name} {ms * 1e3:9.1f} us")
                # 12 line atomics of 128 B per point when d_planes is wanted
                print(f"B={B} M={m:8d} {prec:5s}: " + "  ".join(line) + f"   ({B * m * 12 / 1e6:.2f} M line atomics)")
else:
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    cfg = ffhq512_128()
    ws0, c, us, ui = [t.to(dev) for t in make_inputs(cfg, B)]
    g = torch.Generator().manual_seed(40)
    target = (0.5 * torch.randn(B, 3, cfg.img_resolution, cfg.img_resolution, generator=g)).clamp(-1, 1).to(dev)
    pts = (torch.rand(B, 1000, 3, generator=g) * 2 - 1) * (cfg.box_warp / 2)
    coords = torch.cat([pts, pts + torch.randn(B, 1000, 3, generator=g) * (0.004 * cfg.box_warp)], 1).to(dev)

    def l1(sigma):
        return torch.nn.functional.l1_loss(sigma[:, :1000], sigma[:, 1000:])

    for tuned in (False, True):
        gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
        if tuned:
            for n, p in gen.named_parameters():
                if not n.startswith("backbone.mapping."):
                    p.requires_grad_(True)
        ws = ws0.clone().requires_grad_(True)

        def zero():
            ws.grad = None
            for p in gen.parameters():
                p.grad = None

        def image():
            zero()
            out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)
            torch.nn.functional.mse_loss(out["image"], target).backward()

        def joined():
            zero()
            out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, query=coords)
            (torch.nn.functional.mse_loss(out["image"], target) + 0.25 * l1(out["query_sigma"])).backward()

        def separate():
            zero()
            out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)
            sigma = gen.sample_mixed(coords, None, ws, differentiable=True)["sigma"]
            (torch.nn.functional.mse_loss(out["image"], target) + 0.25 * l1(sigma)).backward()

        todo = (("image", image), ("joined", joined), ("separate", separate))
        for _ in range(3):
            for _, call in todo:
                call()
        torch.cuda.synchronize()
        gc.collect()
        gc.disable()
        res = {name: [] for name, _ in todo}
        for _ in range(runs):
            for name, call in todo:
                per = []
                for _ in range(steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    per.append((e0, e1))
                torch.cuda.synchronize()
                ms = sorted(a.elapsed_time(b) for a, b in per)
                res[name].append(ms[len(ms) // 2])
        gc.enable()
        for name, v in res.items():
            print(f"B={B} generator {'tuned' if tuned else 'frozen'}, {name:8s}: median ms per forward + backward of each run: "
                  + ", ".join(f"{x:.3f}" for x in v))
        del gen
