"""Developer timing of multi-view synthesis (GPU box), ffhq512_128, random weights: `synthesis(ws [B], c [B,V,25])` against the
flattened call `synthesis(ws.repeat_interleave(V, 0), c.flatten(0, 1))` — the single-view code path — in one process, the two arms
alternating, device events around every call, median / minimum ms over `runs` x `steps` calls after warm-up.
usage: bench_multi_view.py forward [steps] [runs]   under no_grad for (B,V) = (1,2), (1,8), (4,2), next to the FLOP-split ceiling
                                                    1 / (1 - 0.322 (V-1)/V) of the forward gain
       bench_multi_view.py step [steps] [runs]      forward + backward (mse on the image, ws requires grad), generator frozen and
                                                    tuned, for (B,V) = (1,2), (1,4)
       bench_multi_view.py kernel [iters] [runs]    ops.planes_sum_to_nhwc against pm.sum(1) + ops.planes_to_nhwc for (B,V) = (1,8),
                                                    (4,2) at 256^2 x 32: us per call and GB/s of the algorithmic bytes (V + 1) |planes|
A path that finds no GPU fails."""
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops                                  # noqa: E402
from hfa_gp_amd.config import ffhq512_128                   # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator          # noqa: E402
from hfa_gp_amd.synthetic import make_inputs, perturb_state  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "forward"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
if not torch.cuda.is_available():
    raise SystemExit("bench_multi_view.py needs the GPU")
dev = torch.device("cuda:0")
cfg = ffhq512_128()


def alternate(arms):
    """{name: (median ms, min ms)} of the arms' calls: warm-up, then `runs` rounds of `steps` calls per arm, arms in turn."""
    for _ in range(3):
        for _, call in arms:
            call()
    torch.cuda.synchronize()
    gc.collect()
    res = {name: [] for name, _ in arms}
    for _ in range(runs):
        for name, call in arms:
            evs = []
            for _ in range(steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            res[name] += [a.elapsed_time(b) for a, b in evs]
    return {name: (sorted(v)[len(v) // 2], min(v)) for name, v in res.items()}


def inputs(b, v):
    ws = make_inputs(cfg, b)[0].to(dev)
    _, c, us, ui = (t.to(dev) for t in make_inputs(cfg, b * v, 11))
    return ws, c.reshape(b, v, 25), us, ui


def generator(tuned):
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    if tuned:
        for n, p in gen.named_parameters():
            if not n.startswith("backbone.mapping."):
                p.requires_grad_(True)
    return gen


if mode == "forward":
    gen = generator(False)
    for b, v in ((1, 2), (1, 8), (4, 2)):
        ws, c, us, ui = inputs(b, v)
        ws_rep, c_flat = ws.repeat_interleave(v, 0), c.flatten(0, 1)
        with torch.no_grad():
            t = alternate([("multi", lambda: gen.synthesis(ws, c, u_strat=us, u_imp=ui)),
                           ("flat", lambda: gen.synthesis(ws_rep, c_flat, u_strat=us, u_imp=ui))])
        ceil = 1.0 / (1.0 - 0.322 * (v - 1) / v)
        print(f"forward B={b} V={v}: multi {t['multi'][0]:.3f} / {t['multi'][1]:.3f} ms, flat {t['flat'][0]:.3f} / {t['flat'][1]:.3f} ms, "
              f"ratio {t['flat'][0] / t['multi'][0]:.3f} x (ceiling {ceil:.2f} x)", flush=True)
elif mode == "step":
    for tuned in (False, True):
        gen = generator(tuned)
        for b, v in ((1, 2), (1, 4)):
            ws, c, us, ui = inputs(b, v)
            target = torch.rand(b, v, 3, cfg.img_resolution, cfg.img_resolution, device=dev) * 2 - 1

            def step(flat):
                w = ws.clone().requires_grad_(True)
                if flat:
                    img = gen.synthesis(w.repeat_interleave(v, 0), c.flatten(0, 1), u_strat=us, u_imp=ui)["image"].unflatten(0, (b, v))
                else:
                    img = gen.synthesis(w, c, u_strat=us, u_imp=ui)["image"]
                (img - target).square().mean().backward()
                for p in gen.parameters():
                    p.grad = None

            t = alternate([("multi", lambda: step(False)), ("flat", lambda: step(True))])
            print(f"step {'tuned' if tuned else 'frozen'} B={b} V={v}: multi {t['multi'][0]:.3f} / {t['multi'][1]:.3f} ms, "
                  f"flat {t['flat'][0]:.3f} / {t['flat'][1]:.3f} ms, ratio {t['flat'][0] / t['multi'][0]:.3f} x", flush=True)
        del gen
        gc.collect()
        torch.cuda.empty_cache()
elif mode == "kernel":
    r = cfg.plane_resolution
    for b, v in ((1, 8), (4, 2)):
        pm = torch.randn(b, v, 3, r, r, 32, device=dev)
        assert torch.equal(ops.planes_sum_to_nhwc(pm[:, :1].contiguous()), ops.planes_to_nhwc(pm[:, 0].contiguous()))
        k = 20          # launches per timed window: one launch is shorter than the events' resolution is good for
        t = alternate([("fused", lambda: [ops.planes_sum_to_nhwc(pm) for _ in range(k)]),
                       ("sum+layout", lambda: [ops.planes_to_nhwc(pm.sum(1)) for _ in range(k)])])
        nbytes = (v + 1) * b * 3 * r * r * 32 * 4
        for name in ("fused", "sum+layout"):
            med, low = t[name][0] / k, t[name][1] / k
            print(f"kernel B={b} V={v} {name}: {med * 1e3:.1f} / {low * 1e3:.1f} us, "
                  f"{nbytes / (med * 1e-3) / 1e9:.0f} GB/s of the (V + 1) |planes| = {nbytes / 1e6:.1f} MB", flush=True)
else:
    raise SystemExit(__doc__)
