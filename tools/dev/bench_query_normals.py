"""Developer timing of the query-point normals (GPU box).
usage: bench_query_normals.py kernels [B] [iters]   ops.planes_query_normals beside ops.planes_query, and ops.planes_query_normals_bwd
                                                    beside ops.planes_query_bwd ({f16x3, fp32} x {planes only, + decoder gradients}),
                                                    at M = 2000 and M = 2^20 on ffhq512_128's 256^2 planes; HIP events around the
                                                    calls, 2 warm-up calls + `iters` (20)
       bench_query_normals.py mesh [N]              the vertex normals of an N^3 (512) ffhq512_128 mesh (want=('normal',)) beside
                                                    the `colors=True` query at the same vertices
For the A/B of the unchanged image-only step against the parent commit run tools/dev/bench_camera_grad.py step ... plain (which
exists on both sides) from each tree."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops                                  # noqa: E402
from hfa_gp_amd.config import ffhq512_128                   # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator          # noqa: E402
from hfa_gp_amd.synthetic import make_inputs, perturb_state    # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
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


cfg = ffhq512_128()
if mode == "kernels":
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
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
            gg, gn = torch.randn(B, m, 3, generator=g).to(dev), torch.randn(B, m, 3, generator=g).to(dev)
            for prec in ("f16x3", "fp32"):
                kw = dict(gen._query_kwargs(), decoder_precision=prec, planes_absmax=pam if prec == "f16x3" else None)
                line = [f"query {timed(lambda: ops.planes_query(planes, coords, **kw), iters) * 1e3:9.1f} us"]
                for name, want in (("all four", ("sigma", "rgb", "grad", "normal")), ("grad+normal", ("grad", "normal")),
                                   ("normal", ("normal",))):
                    ms = timed(lambda: ops.planes_query_normals(planes, coords, want=want, **kw), iters)
                    line.append(f"normals[{name}] {ms * 1e3:9.1f} us")
                print(f"B={B} M={m:8d} {prec:5s} forward : " + "  ".join(line))
                line = []
                for name, extra in (("planes", {}), ("planes+dec", dict(decoder_grads=True))):
                    q = timed(lambda: ops.planes_query_bwd(planes, coords, gs, gr, d_planes=d_planes, **kw, **extra), iters)
                    n = timed(lambda: ops.planes_query_normals_bwd(planes, coords, gg, gn, d_planes=d_planes, **kw, **extra), iters)
                    line.append(f"{name}: query_bwd {q * 1e3:9.1f} us  normals_bwd {n * 1e3:9.1f} us")
                # 12 line atomics of 128 B per point in either backward
                print(f"B={B} M={m:8d} {prec:5s} backward: " + "  ".join(line) + f"   ({B * m * 12 / 1e6:.2f} M line atomics)")
else:
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    ws = torch.randn(1, cfg.num_ws, cfg.w_dim, generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        vol = gen.density_grid(ws, resolution=n)
        p = int(30 * n / 256)
        level = float(vol[..., p:n - p, p:n - p, p:n - p].median())
        del vol
        verts = gen.extract_mesh(ws, resolution=n, level=level)[0]["vertices"]
        planes, pam = gen._query_planes(ws)
        kw = dict(gen._query_kwargs(), planes_absmax=pam)
        col = timed(lambda: ops.planes_query(planes, verts[None], **kw), 20)
        nrm = timed(lambda: ops.planes_query_normals(planes, verts[None], want=("normal",), **kw), 20)
        print(f"{n}^3 mesh, {verts.shape[0]} vertices: colours query {col * 1e3:.1f} us, vertex normals {nrm * 1e3:.1f} us")
