"""Developer A/B of the merged up-conv GEMM at F16X3: the 32-channel 16x16x32 loop against the 16-channel loop
(HFAGP_DEV_UP_LEGACY_LOOP=1), alternating in ONE process on the same seeded random data, per flagship layer.
(profiles/r08_upconv16_ab.log also holds a third arm, the 32-channel loop with 4-byte stores of y_t, which was removed from the
library after that measurement.)
usage: upconv_ab.py [B] [pairs] [iters]   -> one line per layer: median [min, max] us of each arm and the ratio"""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops  # noqa: E402

# input H, Cin -> Cout of the seven up-conv GEMMs of the flagship render
SHAPES = [(4, 512, 512), (8, 512, 512), (16, 512, 512), (32, 512, 512), (64, 512, 256), (128, 256, 128), (256, 256, 128)]
ARMS = {"legacy": {"HFAGP_DEV_UP_LEGACY_LOOP": "1"}, "new16": {}}
SWITCHES = ("HFAGP_DEV_UP_LEGACY_LOOP",)


def _arm(name):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(ARMS[name])


def _expected_kernel(name, cin, cout):
    """The kernel the arm is EXPECTED to launch: modconv_plan.h's upconv_mfma16_takes restated for fp32 storage at these shapes,
    not read back from the library (which also falls back to the 16-channel loop for the 8-wave developer block and for a staged
    span beyond the 32-bit patch offsets; neither occurs here).  The up-conv never goes to the small-image kernel: smallconv_takes
    has no mode CONVT3X3_UP2.  A kernel trace of this tool (rocprofv3 --kernel-trace) shows what ran."""
    if name == "legacy" or cin % 32 or cout % 64 or os.environ.get("HFAGP_DEV_UP_WAVES") == "8":
        return "upconv_bf16_kernel<4, 4, 0>"
    return "upconv_bf16_kernel<4, 4, 0, 2>"


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    dev = torch.device("cuda:0")
    tot = {a: 0.0 for a in ARMS}
    for H, cin, cout in SHAPES:
        g = torch.Generator(device=dev).manual_seed(H + cin)
        x = torch.randn(B, H, H, cin, device=dev, generator=g)
        w = torch.randn(cout, cin, 3, 3, device=dev, generator=g) / math.sqrt(9 * cin)
        wt = ops.weight_prep_prec(w, "f16x3")
        s = torch.randn(B, cin, device=dev, generator=g) + 1.0

        def run():
            return ops.modconv(x, wt, cout, ops.CONVT3X3_UP2, styles=s)
        times = {a: [] for a in ARMS}
        for _ in range(pairs):
            for arm in ARMS:
                _arm(arm)
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
        _arm("new16")
        med = {a: statistics.median(t) for a, t in times.items()}
        for a in tot:
            tot[a] += med[a]
        flops = 2.0 * B * H * H * cin * cout * 9
        cells = "  ".join(f"{a} {med[a]:.1f} us [{min(times[a]):.1f}, {max(times[a]):.1f}]" for a in ARMS)
        print(f"B={B} {H}^2 {cin}->{cout}: {cells}  new16/legacy {med['new16'] / med['legacy']:.3f}  "
              f"({flops / med['new16'] / 1e6:.0f} vs {flops / med['legacy'] / 1e6:.0f} TFLOP/s)  expected kernels: "
              f"{_expected_kernel('new16', cin, cout)} vs {_expected_kernel('legacy', cin, cout)}", flush=True)
        del x, w, wt
        torch.cuda.empty_cache()
    print(f"B={B} up-conv family, sum of medians: legacy {tot['legacy']:.0f} us, new16 {tot['new16']:.0f} us, "
          f"new16/legacy {tot['new16'] / tot['legacy']:.3f}", flush=True)


if __name__ == "__main__":
    main()
