"""Developer timing of the camera gradient of the per-ray surface normals (GPU box), ffhq512_128, B frames (default 2: the fitting batch).
usage: bench_normal_camera_grad.py [B] [iters] [runs]   on the planes of one backbone pass and the state of one forward ray march:
           ops.raymarch_normals_bwd (generator frozen), ops.raymarch_bwd_camera (on the records of one ops.raymarch_bwd) and
           ops.raymarch_normals_bwd_camera — on its own with the reduction, and adding into the camera pass's records (the call the
           fitting step makes) — HIP events around `iters` calls of each, arms alternating, `runs` runs; prints every run's ms per
           call and the medians."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops                                  # noqa: E402
from hfa_gp_amd.config import ffhq512_128                   # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator          # noqa: E402
from hfa_gp_amd.synthetic import make_inputs, perturb_state  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
cfg = ffhq512_128()
gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
ws, c, us, ui = [t.to(dev) for t in make_inputs(cfg, B)]


def median(v):
    return sorted(v)[len(v) // 2]


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


with torch.no_grad():
    res = cfg.neural_rendering_resolution
    planes = gen.backbone_planes(ws)
    u_s, u_i = gen._uniforms(B, dev, us, ui)
    kw = dict(gen._render_args(c), u_strat=u_s, u_imp=u_i, planes_absmax=getattr(gen, "_planes_absmax", None))
    st = ops.raymarch_state(B, res, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
    ops.raymarch(planes, state=st, **kw)
    g = torch.Generator().manual_seed(1)
    g_feat = torch.randn(B, res * res, 32, generator=g).to(dev)
    g_normal = torch.randn(B, res * res, 3, generator=g).to(dev)
    d_planes = torch.zeros_like(planes)
    rec = []
    ops.raymarch_bwd(g_feat, planes, state=st, rec_out=rec, **kw)
    _, _, ray_grad = ops.raymarch_bwd_camera(g_feat, planes, rec[0], reduce=False, **kw)
    arms = [("raymarch_normals_bwd", lambda: ops.raymarch_normals_bwd(g_normal, planes, st, d_planes=d_planes, **kw)),
            ("raymarch_bwd_camera", lambda: ops.raymarch_bwd_camera(g_feat, planes, rec[0], **kw)),
            ("raymarch_normals_bwd_camera", lambda: ops.raymarch_normals_bwd_camera(g_normal, planes, st, **kw)),
            ("raymarch_normals_bwd_camera (into ray_grad)",
             lambda: ops.raymarch_normals_bwd_camera(g_normal, planes, st, ray_grad=ray_grad, **kw))]
    for _ in range(2):
        for _, call in arms:
            call()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in arms}
    for _ in range(runs):
        for name, call in arms:
            ms[name].append(timed(call))
    print(f"B={B} ({B * res * res} rays x {cfg.depth_resolution + cfg.depth_resolution_importance} samples), ms per call of each run:")
    for name, v in ms.items():
        print(f"  {name}: " + ", ".join(f"{x:.3f}" for x in v) + f"; median {median(v):.3f} ms")
