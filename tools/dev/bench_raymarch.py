"""Developer micro-benchmark of the ray-march kernel alone (run on the GPU box).
usage: bench_raymarch.py [B] [iters] [pairs]
pairs > 0: A/B of the tap forms in ONE process — all three planes' taps on every quad lane (HFAGP_DEV_RAY_TAPS_LEGACY=1) against
one plane per lane exchanged by DPP (default), arms alternating, `pairs` rounds of `iters` launches each -> median [min, max] per
arm, and whether the two arms' outputs are the same bits."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd.synthetic import make_inputs  # noqa: E402
from hfa_gp_amd.config import ffhq512_128  # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator  # noqa: E402


SWITCH = "HFAGP_DEV_RAY_TAPS_LEGACY"


def ab(gen, args, B, iters, pairs):
    times, outs = {"legacy": [], "new": []}, {}
    for _ in range(pairs):
        for arm in ("legacy", "new"):
            if arm == "legacy":
                os.environ[SWITCH] = "1"
            else:
                os.environ.pop(SWITCH, None)
            for _ in range(2):
                outs[arm] = gen.render(*args)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                gen.render(*args)
            e1.record()
            torch.cuda.synchronize()
            times[arm].append(e0.elapsed_time(e1) / iters * 1e3)
    os.environ.pop(SWITCH, None)
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs["new"], outs["legacy"]))
    med = {a: statistics.median(t) for a, t in times.items()}
    print(f"raymarch B={B} ({pairs} pairs x {iters} launches): legacy {med['legacy']:.1f} us [{min(times['legacy']):.1f}, "
          f"{max(times['legacy']):.1f}]  new {med['new']:.1f} us [{min(times['new']):.1f}, {max(times['new']):.1f}]  "
          f"new/legacy {med['new'] / med['legacy']:.4f}  new max {'<' if max(times['new']) < min(times['legacy']) else '>='} legacy min  "
          f"outputs {'bit-identical' if same else 'DIFFER'}", flush=True)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    dev = torch.device("cuda:0")
    cfg = ffhq512_128()
    gen = TriPlaneGenerator(cfg, seed=0).to(dev)
    ws, c, us, ui = [t.to(dev) for t in make_inputs(cfg, B)]
    with torch.no_grad():
        planes = gen.backbone_planes(ws)
        if pairs > 0:
            ab(gen, (planes, c, us, ui), B, iters, pairs)
            return
        for _ in range(2):
            gen.render(planes, c, us, ui)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            out = gen.render(planes, c, us, ui)
        e1.record()
        torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    gb = B * 2.424438784   # GB per launch
    print(f"raymarch B={B}: {ms:.3f} ms/launch = {ms / B * 1e3:.1f} us/frame, {gb / ms * 1e3:.0f} GB/s algorithmic "
          f"({gb / ms * 1e3 / 8000:.3f} of 8 TB/s); checksum {out[0].double().sum().item():.6f}")


if __name__ == "__main__":
    main()
