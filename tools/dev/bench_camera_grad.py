"""Developer timing of the camera gradient (GPU box), ffhq512_128, B frames.
usage: bench_camera_grad.py kernels [B] [iters]     ops.raymarch_bwd (sort + gather, forward state) and ops.raymarch_bwd_camera,
                                                    HIP events around each call; under `rocprofv3 --kernel-trace --stats` the
                                                    per-kernel durations (dL/dF producer beside the camera pass)
       bench_camera_grad.py step [B] [steps] [runs] [both|plain]
                                                    the 3DMM-driven fitting step (bench.py's train leg: generator frozen, L2 at
                                                    256^2, Adam) with a plain label and with label = base + delta, delta requiring
                                                    grad; arms alternating, `runs` runs of `steps` steps each
The image-only arm is what bench.py times: run the same command on the parent commit for the A/B."""
import gc
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops                                  # noqa: E402
from hfa_gp_amd.config import ffhq512_128                   # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator          # noqa: E402
from hfa_gp_amd.synthetic import look_at_label, make_inputs, perturb_state    # noqa: E402

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
        out = call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


if mode == "kernels":
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    cfg = ffhq512_128()
    gen = TriPlaneGenerator(cfg, seed=0).to(dev)
    ws, c, us, ui = [t.to(dev) for t in make_inputs(cfg, B)]
    with torch.no_grad():
        planes = gen.backbone_planes(ws)
        u_s, u_i = gen._uniforms(B, dev, us, ui)
        g = torch.randn(B, 128 * 128, 32, device=dev)
        kw = gen._render_args(c)
        pam = getattr(gen, "_planes_absmax", None)
        st = ops.raymarch_state(B, 128, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
        ops.raymarch(planes, u_strat=u_s, u_imp=u_i, planes_absmax=pam, state=st, **kw)
        rec = []
        ms_bwd, _ = timed(lambda: ops.raymarch_bwd(g, planes, u_strat=u_s, u_imp=u_i, planes_absmax=pam, state=st, rec_out=rec, **kw),
                          iters)
        ms_cam, out = timed(lambda: ops.raymarch_bwd_camera(g, planes, rec[-1], u_strat=u_s, u_imp=u_i, planes_absmax=pam, **kw), iters)
        again = ops.raymarch_bwd_camera(g, planes, rec[-1], u_strat=u_s, u_imp=u_i, planes_absmax=pam, **kw)
    print(f"B={B}: raymarch_bwd (pass 1 from state + sort + dL/dF + gather) {ms_bwd:.3f} ms/call; raymarch_bwd_camera (ray pass + "
          f"reduction) {ms_cam:.3f} ms/call; repeatable bits: {all(torch.equal(x, y) for x, y in zip(out, again))}; "
          f"|d_cam2world| max {out[0].abs().max().item():.3e}")
else:
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    arms = sys.argv[5] if len(sys.argv) > 5 else "both"          # "plain": the image-only arm alone (runs on the parent commit too)
    from hfa_gp_amd.trainer import Trainer

    import bench            # (_FitArgs: the arguments of bench.py's train leg)
    fa = bench._FitArgs()
    fa.generator_preset = "ffhq512_128"
    torch.manual_seed(0)
    tr = Trainer(fa, dev, rank=0, world_size=1, mode="3dmm", lpips="none")
    perturb_state(tr.gen.generator)
    gg = torch.Generator().manual_seed(40)
    real = (0.5 * torch.randn(B, 3, fa.size, fa.size, generator=gg)).clamp(-1, 1).to(dev)
    params = torch.randn(B, fa.params_len, generator=gg).to(dev)
    label = look_at_label(math.pi / 2 + 0.3 * torch.randn(B, generator=gg), math.pi / 2 + 0.155 * torch.randn(B, generator=gg),
                          flipped=False).to(dev)
    delta = torch.zeros(B, 25, device=dev, requires_grad=True)

    def plain():
        return tr.gen_update(real, label.clone(), params)

    def camera():
        delta.grad = None
        return tr.gen_update(real, label + delta, params)

    todo = (("image-only", plain),) + ((("with d c", camera),) if arms == "both" else ())
    for _ in range(5):
        for _, call in todo:
            call()
    torch.cuda.synchronize()
    assert arms != "both" or (delta.grad is not None and bool(delta.grad.abs().max() > 0))
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
    for name, v in res.items():
        print(f"B={B} fitting step (3DMM-driven, generator frozen), {name}: median ms per step of each run: "
              + ", ".join(f"{x:.3f}" for x in v))
