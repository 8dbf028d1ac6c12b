"""The call path behind `TriPlaneGenerator.synthesis` (its docstring is the public description): `resolve` turns the call's keywords
into a `SynthesisCall`, every check in its order; `synthesis` then takes the one forward (`TriPlaneGenerator._forward_impl`) without
grad or through the one autograd function (`autograd.SynthesisFn`), whatever the call asked for, and assembles the dict.  The record
lives as long as the call: nothing of a request is kept on the generator.  A label [B,V,25] (V views of every latent) is flattened
to frames f = b·V + v here on the way in, and the per-frame outputs get their view axis back on the way out."""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional

import torch

from .autograd import SynthesisFn


@dataclasses.dataclass(eq=False)
class SynthesisCall:
    """What `synthesis` was asked for, resolved: the keyword implications applied (`normal_camera_grad` → `normal_grad` →
    `normals`), `query` the points as a detached contiguous fp32 tensor — None without points to evaluate (no keyword, M = 0 or
    B = 0) —, `res` the rays per side of this call, the uniforms as the caller gave them, `views` the V of a label [B,V,25] (None
    for a 2-D label: one camera per latent).  The forward fills `planes` and
    `feature_image` (for `return_planes`), and the autograd function leaves a detached 'image_normal' in `image_normal`: as an
    output it would have autograd build a zero gradient image for it where unused gradients are materialised."""
    geometry: bool
    query: Optional[torch.Tensor]
    query_normals: bool
    normals: bool
    normal_grad: bool
    normal_camera_grad: bool
    return_planes: bool
    res: int
    u_strat: Optional[torch.Tensor]
    u_imp: Optional[torch.Tensor]
    planes: Optional[torch.Tensor] = None
    feature_image: Optional[torch.Tensor] = None
    image_normal: Optional[torch.Tensor] = None
    views: Optional[int] = None


def resolve(gen, ws, c, noise_mode, u_strat, u_imp, return_planes, geometry, query, normals, normal_grad, normal_camera_grad,
            query_normals, neural_rendering_resolution) -> SynthesisCall:
    """Everything `synthesis` does before its first launch: the checks, in this order (the resolution is stored before the later ones
    can raise)."""
    gen._check_inputs(ws, c, noise_mode)
    views = c.shape[1] if c.dim() == 3 else None
    frames = ws.shape[0] * (1 if views is None else views)        # flat frame index f = b·V + v: the uniforms are sized for them
    gen._set_resolution(frames, neural_rendering_resolution, u_strat, u_imp)
    normal_grad = bool(normal_grad or normal_camera_grad)
    if query_normals:
        if query is None:
            raise ValueError("TriPlaneGenerator.synthesis: query_normals=True needs query=coords")
        if normal_grad:
            raise NotImplementedError("TriPlaneGenerator.synthesis: query_normals=True together with normal_grad=True / "
                                      "normal_camera_grad=True is not implemented")
        if torch.is_grad_enabled() and query.requires_grad:
            raise NotImplementedError("TriPlaneGenerator.synthesis: 'query_sigma_grad' / 'query_normal' have no gradient w.r.t. the "
                                      "points (it needs the mixed second derivative of the gather); detach `query`")
    if normal_grad and torch.is_grad_enabled():
        gen._check_normal_grad(ws, c, normal_camera_grad)
    if query is not None:
        if query.dim() != 3 or query.shape[-1] != 3 or query.shape[0] not in (1, ws.shape[0]) or not query.is_cuda:
            raise ValueError(f"expected query [B or 1, M, 3] on the device for ws of batch {ws.shape[0]}, got "
                             f"{tuple(query.shape)} on {query.device}")
        if views == 0 and ws.shape[0] and query.shape[1]:
            raise ValueError("TriPlaneGenerator.synthesis: query= with a label of V = 0 views launches nothing, so the points would go "
                             "unevaluated; use `sample_mixed` for points without an image")
        if query.shape[1] == 0 or frames == 0:       # nothing to evaluate: `synthesis` makes the keys
            query = None
    return SynthesisCall(geometry=bool(geometry), query=None if query is None else query.detach().float().contiguous(),
                         query_normals=bool(query_normals), normals=bool(normals or normal_grad), normal_grad=normal_grad,
                         normal_camera_grad=bool(normal_camera_grad), return_planes=bool(return_planes),
                         res=gen.neural_rendering_resolution, u_strat=u_strat, u_imp=u_imp, views=views)


def _no_frames(gen, call: SynthesisCall, ws, c):
    """The outputs of a call without frames (the ragged last batch of a frame shard; a label of V = 0 views), nothing launched, flat
    over the frames as the forward returns them: 'image' keeps the autograd edges to ws and c, a differentiable 'image_normal' the
    one to ws."""
    cfg, dev, r = gen.cfg, ws.device, call.res
    img = torch.zeros(0, cfg.img_channels, cfg.img_resolution, cfg.img_resolution, device=dev) + 0.0 * ws.sum() + 0.0 * c.sum()
    normal = torch.zeros(0, 3, r, r, device=dev)
    if call.normal_grad and torch.is_grad_enabled():
        normal = normal + 0.0 * ws.sum()
    return (img, torch.zeros(0, 3, r, r, device=dev), torch.zeros(0, 1, r, r, device=dev), torch.zeros(0, 1, r, r, device=dev),
            None, None, None, None, normal)


def synthesis(gen, ws, c, noise_mode, u_strat, u_imp, return_planes, geometry, query, normals, normal_grad, normal_camera_grad,
              query_normals, neural_rendering_resolution) -> Dict[str, torch.Tensor]:
    """`TriPlaneGenerator.synthesis`, its parameters in its order."""
    call = resolve(gen, ws, c, noise_mode, u_strat, u_imp, return_planes, geometry, query, normals, normal_grad, normal_camera_grad,
                   query_normals, neural_rendering_resolution)
    b, dev, views = ws.shape[0], ws.device, call.views
    frames = b if views is None else b * views
    if views is not None:
        c = c.reshape(frames, c.shape[-1])        # frame f = b·V + v; a view of the label, so its gradient comes back [B,V,25]
    params = [p for n, p in gen.named_parameters() if not n.startswith("backbone.mapping.")]
    cam_grad = torch.is_grad_enabled() and c.requires_grad
    grad = frames > 0 and torch.is_grad_enabled() and (ws.requires_grad or cam_grad or any(p.requires_grad for p in params) or
                                                       (call.query is not None and query.requires_grad))
    if frames == 0:
        outs = _no_frames(gen, call, ws, c)
    elif grad:
        outs = SynthesisFn.apply(ws, c if cam_grad else c.detach(), u_strat, u_imp, None if call.query is None else query, call, gen,
                                 *params)
    else:
        with torch.no_grad():
            outs = gen._forward_impl(call, ws.detach().float().contiguous(), c.detach().float().contiguous(), None)
    img, rgb_raw, depth, mask, q_sigma, q_rgb, q_grad, q_normal, normal = outs
    if views is not None:
        # the view axis after the batch axis; the planes and the query keys belong to the identity (an output the call did not ask for
        # is None, or the autograd function's empty 1-D placeholder)
        img, rgb_raw, depth, mask, normal, call.feature_image, call.image_normal = (
            t.unflatten(0, (b, views)) if t is not None and t.dim() == 4 else t
            for t in (img, rgb_raw, depth, mask, normal, call.feature_image, call.image_normal))
    out = {"image": img, "image_raw": rgb_raw, "image_depth": depth}
    if call.geometry:
        out["image_mask"] = mask
    if query is not None:
        if call.query is None:            # no points or no frames: the keys, with the autograd edge of the points
            m = query.shape[1]
            zero = 0.0 * query.sum() if query.requires_grad else 0.0
            q_sigma, q_rgb = torch.zeros(b, m, 1, device=dev) + zero, torch.zeros(b, m, 32, device=dev) + zero
            q_grad, q_normal = torch.zeros(b, m, 3, device=dev), torch.zeros(b, m, 3, device=dev)
        out["query_sigma"], out["query_rgb"] = q_sigma, q_rgb
        if call.query_normals:
            out["query_sigma_grad"], out["query_normal"] = q_grad, q_normal
    # (a differentiable 'image_normal' has always come before the planes, a detached one after them)
    if call.normal_grad and grad:
        out["image_normal"] = normal
    if call.return_planes and frames:
        out["planes"], out["feature_image"] = call.planes, call.feature_image
    if call.normals and not (call.normal_grad and grad):
        out["image_normal"] = normal if call.image_normal is None else call.image_normal
    return out
