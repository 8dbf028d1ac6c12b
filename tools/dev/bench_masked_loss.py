"""Developer timing of the masked-fit loss side on the GPU box (profiles/masked_loss/README.md):
  kernels  ops.pool_wmse against ops.pool_mse, forward and backward, at [2,3,512,512] -> 256^2 and [8,3,512,512] -> 256^2,
           the two sides alternating inside one process;
  step     the 2-frame ffhq512_128 fitting step of tools/dev/bench_train.py, generator frozen and tuned: without keywords,
           with mask=, with mask= + matte=.
Device events around every call, >= 20 warm-up and >= 200 timed iterations, median and p10 / p90.
  python tools/dev/bench_masked_loss.py [kernels|step|all] [--root TREE] [--iters 200] [--warmup 20] [--plain-only] [--json FILE]
--root TREE: time the package of another checkout (the parent commit: --plain-only, it has no keywords) in the same session."""
import argparse
import json
import os
import sys

import torch


def stats(ms):
    ms = sorted(ms)
    pick = lambda q: ms[min(len(ms) - 1, int(q * len(ms)))]
    return {"median_us": 1e3 * pick(0.5), "p10_us": 1e3 * pick(0.1), "p90_us": 1e3 * pick(0.9), "n": len(ms)}


def timed(fns, warmup, iters):
    """`fns`: name -> callable; the callables ALTERNATE, each call between its own pair of events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in evs.items()}


def bench_kernels(dev, warmup, iters):
    from hfa_gp_amd import ops
    out = {}
    for b in (2, 8):
        g = torch.Generator().manual_seed(b)
        img = torch.randn(b, 3, 512, 512, generator=g).to(dev).requires_grad_(True)
        real = (0.5 * torch.randn(b, 3, 256, 256, generator=g)).clamp(-1, 1).to(dev)
        weight = torch.rand(b, 1, 256, 256, generator=g).to(dev)
        one = torch.ones((), device=dev)
        lu, _ = ops.pool_mse(img, real)
        lw, _ = ops.pool_wmse(img, real, weight)
        with torch.no_grad():
            res = timed({"pool_mse fwd": lambda: ops.pool_mse(img, real), "pool_wmse fwd": lambda: ops.pool_wmse(img, real, weight)},
                        warmup, iters)
        res.update(timed({"pool_mse bwd": lambda: torch.autograd.grad(lu, img, one, retain_graph=True),
                          "pool_wmse bwd": lambda: torch.autograd.grad(lw, img, one, retain_graph=True)}, warmup, iters))
        for side in ("fwd", "bwd"):
            res[f"ratio {side}"] = res[f"pool_wmse {side}"]["median_us"] / res[f"pool_mse {side}"]["median_us"]
        out[f"[{b},3,512,512]->256"] = res
    return out


class Args:
    out_pose = False; person_2 = False; params_len = 76; size = 256; batch_size = 2; lr = 3e-4
    latent_dim_style = 512; latent_dim_shape = 50; generator_preset = "ffhq512_128"; generator_seed = 0


def bench_step(dev, warmup, iters, plain_only):
    from hfa_gp_amd.synthetic import look_at_label
    from hfa_gp_amd.trainer import Trainer
    out = {}
    b = 2
    g = torch.Generator().manual_seed(1)
    real = (0.5 * torch.randn(b, 3, 256, 256, generator=g)).clamp(-1, 1).to(dev)
    params = torch.randn(b, 76, generator=g).to(dev)
    label0 = look_at_label(1.57 + 0.3 * torch.randn(b, generator=g), 1.57 + 0.15 * torch.randn(b, generator=g), flipped=False).to(dev)
    y, x = torch.meshgrid(torch.linspace(-1, 1, 256), torch.linspace(-1, 1, 256), indexing="ij")
    matte = ((x * x + y * y) < 0.6).float()[None, None].repeat(b, 1, 1, 1).to(dev)
    mask = (matte * (0.5 + torch.rand(b, 1, 256, 256, generator=g).to(dev))).contiguous()
    for regime in ("frozen", "tuned"):
        torch.manual_seed(0)
        tr = Trainer(Args(), dev, mode="3dmm", lpips="none")
        if regime == "tuned":
            tr.tune_generator()
        fns = {"no keywords": lambda: tr.gen_update(real, label0.clone(), params)}
        if not plain_only:
            fns["mask"] = lambda: tr.gen_update(real, label0.clone(), params, mask=mask)
            fns["mask + matte"] = lambda: tr.gen_update(real, label0.clone(), params, mask=mask, matte=matte)
        out[regime] = timed(fns, warmup, iters)
        del tr
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["kernels", "step", "all"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.iters < 200 or a.warmup < 20:
        print("note: fewer than 200 timed / 20 warm-up iterations: not a number for the record", file=sys.stderr)
    sys.path.insert(0, os.path.abspath(a.root))
    if not torch.cuda.is_available():
        raise SystemExit("bench_masked_loss: needs the GPU (a timing without it says nothing)")
    dev = torch.device("cuda:0")
    res = {"root": os.path.abspath(a.root), "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup}
    if a.what in ("kernels", "all") and not a.plain_only:
        res["kernels"] = bench_kernels(dev, a.warmup, a.iters)
    if a.what in ("step", "all"):
        res["step"] = bench_step(dev, a.warmup, a.iters, a.plain_only)
    for sect in ("kernels", "step"):
        for shape, rows in res.get(sect, {}).items():
            for name, v in rows.items():
                if isinstance(v, dict):
                    print(f"{sect:8s} {shape:22s} {name:16s} median {v['median_us']:10.1f} us  p10 {v['p10_us']:10.1f}  p90 {v['p90_us']:10.1f}")
                else:
                    print(f"{sect:8s} {shape:22s} {name:16s} {v:.3f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)) or ".", exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
