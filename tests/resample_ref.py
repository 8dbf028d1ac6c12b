"""Reference for `synthesis(neural_rendering_resolution=N)`: the oracle has no resample, so EG3D's path is composed here from the
oracle's own functions — ray_sampler at N, backbone_synthesis, importance_renderer at N, torch's antialiased bilinear
F.interpolate of the feature image to the super-resolution input resolution r0 (per channel, hence of rgb = its first three channels
too, as SuperresolutionHybrid8XDC resizes both), superresolution.  Plain differentiable PyTorch on the CPU (the style of
test_gpu_geometry_grad._oracle_synthesis_geom).  At N == r0 nothing is resampled and the tensors are O.synthesis's."""
import dataclasses

import torch.nn.functional as F


def inputs(cfg, batch, n, seed=10):
    """util.make_inputs with the renderer's uniforms sized for n x n rays: (ws, c, u_strat, u_imp)."""
    from tests.util import make_inputs
    return make_inputs(dataclasses.replace(cfg, neural_rendering_resolution=n), batch, seed)


def synthesis(P, cfg, ws, c, u_strat, u_imp, n=None):
    """{'image' [B,3,4 r0,4 r0], 'image_raw' [B,3,n,n], 'image_depth' [B,1,n,n], 'image_mask' [B,1,n,n], 'feature_image' [B,32,n,n]}
    for rays marched at n x n (None: r0 = cfg.neural_rendering_resolution)."""
    from oracle import eg3d_oracle as O
    r0 = cfg.neural_rendering_resolution
    n = r0 if n is None else n
    b = ws.shape[0]
    o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:25].reshape(-1, 3, 3), n)
    planes = O.backbone_synthesis(P, cfg, ws)
    planes5 = planes.reshape(b, 3, cfg.plane_channels, planes.shape[-2], planes.shape[-1])
    feat, depth, wsum = O.importance_renderer(P, dataclasses.replace(cfg, neural_rendering_resolution=n), planes5, o, d, u_strat, u_imp)
    feat_img = feat.permute(0, 2, 1).reshape(b, feat.shape[-1], n, n).contiguous()
    resized = feat_img
    if n != r0:
        resized = F.interpolate(feat_img, (r0, r0), mode="bilinear", align_corners=False, antialias=True)
    img = O.superresolution(P, cfg, resized[:, :3], resized, ws)
    return {"image": img, "image_raw": feat_img[:, :3], "image_depth": depth.permute(0, 2, 1).reshape(b, 1, n, n),
            "image_mask": wsum.permute(0, 2, 1).reshape(b, 1, n, n), "feature_image": feat_img}
