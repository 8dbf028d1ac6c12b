"""Developer A/B of the forward 3x3 conv at F16X3, two arms alternating in ONE process on the same seeded random data, per
flagship layer.  The arm "legacy" sets a developer switch, the arm "new" leaves it unset:
  loop      (default) HFAGP_DEV_CONV9_LEGACY=1: the 16-channel loop against the 32-channel 16x16x32 loop;
  epilogue  HFAGP_DEV_CONV_EPILOGUE_LEGACY=1: the per-element epilogue against the batched one, on the 32-channel loop;
  epilogue16  the same switch with HFAGP_DEV_CONV9_LEGACY=1 held in both arms: the 16-channel loop's two epilogues.
usage: conv9_ab.py [B] [pairs] [iters] [loop|epilogue|epilogue16]
-> one line per layer: median / min / max us of each arm and the ratio; for the epilogue arms also the drop against the fixed
   share of the layer by the per-block model of DESIGN.md section 4.2 (17.4 us x blocks / 512)"""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops  # noqa: E402

SHAPES = [(512, 128, 128), (256, 256, 256), (256, 128, 128), (128, 256, 256), (64, 512, 512), (32, 512, 512), (16, 512, 512),
          (8, 512, 512)]
SWITCH = {"loop": "HFAGP_DEV_CONV9_LEGACY", "epilogue": "HFAGP_DEV_CONV_EPILOGUE_LEGACY", "epilogue16": "HFAGP_DEV_CONV_EPILOGUE_LEGACY"}
FIXED_US_PER_BLOCK = 17.4     # a of t_block = a + b chunks, one block slot out of 2 x 256


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    what = sys.argv[4] if len(sys.argv) > 4 else "loop"
    switch = SWITCH[what]
    if what == "epilogue16":
        os.environ["HFAGP_DEV_CONV9_LEGACY"] = "1"
    dev = torch.device("cuda:0")
    tot = {"new": 0.0, "legacy": 0.0}
    clean = 0
    for H, cin, cout in SHAPES:
        g = torch.Generator(device=dev).manual_seed(H + cin)
        x = torch.randn(B, H, H, cin, device=dev, generator=g)
        w = torch.randn(cout, cin, 3, 3, device=dev, generator=g) / math.sqrt(9 * cin)
        wt = ops.weight_prep_prec(w, "f16x3")
        s = torch.randn(B, cin, device=dev, generator=g) + 1.0
        dcoef = torch.rand(B, cout, device=dev, generator=g)
        bias = torch.randn(cout, device=dev, generator=g)

        def run():
            return ops.modconv(x, wt, cout, ops.CONV3X3, styles=s, dcoef=dcoef, bias=bias, act="lrelu", gain=math.sqrt(2),
                               clamp=256.0)
        times = {"new": [], "legacy": []}
        for _ in range(pairs):
            for arm in ("legacy", "new"):
                if arm == "legacy":
                    os.environ[switch] = "1"
                else:
                    os.environ.pop(switch, None)
                for _ in range(2):
                    run()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    run()
                e1.record()
                torch.cuda.synchronize()
                times[arm].append(e0.elapsed_time(e1) / iters * 1e3)
        os.environ.pop(switch, None)
        med = {a: statistics.median(t) for a, t in times.items()}
        for a in tot:
            tot[a] += med[a]
        flops = 2.0 * B * H * H * cin * cout * 9
        line = (f"B={B} {H}^2 {cin}->{cout}: legacy {med['legacy']:.1f} us [{min(times['legacy']):.1f}, {max(times['legacy']):.1f}]  "
                f"new {med['new']:.1f} us [{min(times['new']):.1f}, {max(times['new']):.1f}]  new/legacy {med['new'] / med['legacy']:.3f}  "
                f"({flops / med['new'] / 1e6:.0f} vs {flops / med['legacy'] / 1e6:.0f} TFLOP/s)")
        if what != "loop":
            blocks = B * ((H + 7) // 8) * ((H + 15) // 16) * (cout // 128)
            fixed = FIXED_US_PER_BLOCK * blocks / 512
            sep = max(times["new"]) < min(times["legacy"])
            clean += sep
            line += (f"  drop {med['legacy'] - med['new']:.1f} us of a fixed share of {fixed:.0f} us ({blocks} blocks); slowest new "
                     f"{'below' if sep else 'NOT below'} fastest legacy")
        print(line, flush=True)
        del x, w, wt
        torch.cuda.empty_cache()
    print(f"B={B} 9-tap family ({what}), sum of medians: legacy {tot['legacy']:.0f} us, new {tot['new']:.0f} us, "
          f"new/legacy {tot['new'] / tot['legacy']:.3f}" + (f"; ranges apart on {clean} of {len(SHAPES)} layers" if what != "loop" else ""),
          flush=True)


if __name__ == "__main__":
    main()
