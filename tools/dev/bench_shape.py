"""Point-query / shape-export rates at ffhq512_128 on one GPU, in one process (run on the GPU box):

  * the grid-mode query kernel, sigma only, N = 512, B = 1, in points per second (HIP events around the launch alone);
  * the same with rgb (a 128-plane x slab: the full 512^3 rgb output would be 17 GB);
  * density_grid end to end (backbone + query, device-synchronised), N = 256 and 512;
  * the EG3D-shaped loop: `sample` per 1 M-point chunk of a materialised lattice, mapping + backbone re-run for each chunk;
  * the ray marcher's samples per second at B = 32 (32 * 128^2 * 96 samples over its launch time), the reference rate.

    python tools/dev/bench_shape.py [reps] [out.json]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hfa_gp_amd import ops  # noqa: E402
from hfa_gp_amd.config import ffhq512_128  # noqa: E402
from hfa_gp_amd.generator import TriPlaneGenerator  # noqa: E402
from hfa_gp_amd.synthetic import make_inputs, perturb_state  # noqa: E402


def timed(fn, reps):
    """median ms of `reps` calls (HIP events; one warm-up call)"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    dev = torch.device("cuda:0")
    cfg = ffhq512_128()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    res = {}
    with torch.no_grad():
        ws, c, us, ui = [t.to(dev) for t in make_inputs(cfg, 32)]
        # ---- the reference rate: ray marcher at B = 32
        planes32 = gen.backbone_planes(ws)
        pam32 = gen._planes_absmax
        ms = timed(lambda: gen.render(planes32, c, us, ui, planes_absmax=pam32), reps)
        samples = 32 * cfg.neural_rendering_resolution ** 2 * (cfg.depth_resolution + cfg.depth_resolution_importance)
        res["raymarch_B32_ms"] = ms
        res["raymarch_samples_per_s"] = samples / ms * 1e3
        del planes32
        torch.cuda.empty_cache()
        # ---- query kernel, grid mode, B = 1
        w1 = ws[:1].contiguous()
        planes, pam = gen._query_planes(w1)
        kw = gen._query_kwargs()
        n = 512
        vol = torch.empty(1, n, n, n, device=dev)
        ms = timed(lambda: ops.planes_query(planes, grid=(n, cfg.box_warp, 0, n), planes_absmax=pam, want_rgb=False, out=vol, **kw), reps)
        res["query_sigma_N512_ms"] = ms
        res["query_sigma_points_per_s"] = n ** 3 / ms * 1e3
        xs = 128
        ms = timed(lambda: ops.planes_query(planes, grid=(n, cfg.box_warp, 0, xs), planes_absmax=pam, **kw), reps)
        res["query_rgb_slab128_ms"] = ms
        res["query_rgb_points_per_s"] = xs * n * n / ms * 1e3
        torch.cuda.empty_cache()
        # ---- density_grid end to end
        for nn_ in (256, 512):
            torch.cuda.synchronize()
            def run(nn_=nn_):
                gen.density_grid(w1, resolution=nn_)
            res[f"density_grid_N{nn_}_ms"] = timed(run, reps)
        # ---- EG3D-shaped loop: sample() per 1 M points, mapping + backbone per chunk
        z = torch.randn(1, cfg.z_dim, device=dev)
        c1 = c[:1].contiguous()
        i = torch.arange(n, dtype=torch.float32, device=dev) * (cfg.box_warp / (n - 1)) - cfg.box_warp / 2
        lat = torch.stack(torch.meshgrid(i, i, i, indexing="ij"), -1).reshape(1, -1, 3)
        chunk = 1 << 20
        def eg3d_loop():
            for k in range(0, lat.shape[1], chunk):
                gen.sample(lat[:, k:k + chunk], None, z, c1)["sigma"]
        ms = timed(eg3d_loop, max(1, reps // 2))
        res["eg3d_loop_N512_ms"] = ms
        res["eg3d_loop_chunks"] = (lat.shape[1] + chunk - 1) // chunk
        res["density_grid_speedup_vs_eg3d_loop"] = ms / res["density_grid_N512_ms"]
        res["query_sigma_vs_raymarch_rate"] = res["query_sigma_points_per_s"] / res["raymarch_samples_per_s"]
    res["device"] = torch.cuda.get_device_name(0)
    res["time"] = time.strftime("%Y-%m-%d %H:%M:%S")
    line = json.dumps(res, sort_keys=True)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
