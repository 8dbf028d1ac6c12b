"""The list renderer behind `TriPlaneGenerator.render_rays` (its docstring is the public description): `resolve` turns the call's
keywords into a `RayCall`, `march` is the one forward path — with and without grad, whole or in ray chunks above
generator.RAY_STATE_CAP_BYTES — and `RenderRaysFn` the one autograd function, whatever the call asked for.  Every launch is an
`ops.<name>` looked up at call time, and the cap is read from the generator module at call time.
`trace_rays` (behind `TriPlaneGenerator.trace_rays`) takes the same lists with the same limits — the checks of `resolve` it shares
are the four helpers in front of it — to the first hit with the density iso-surface."""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional, Tuple

import torch

from . import generator, ops
from .autograd import _Backward, _backbone_backward


@dataclasses.dataclass(eq=False)
class RayCall:
    """What `render_rays` was asked for, resolved: the keyword implications applied, the limits as detached fp32 tensors (None
    without; `has_limits` also for an empty list, whose limits are never computed), the uniforms drawn, `grad` = the call is
    differentiated, `params` = the generator parameters the autograd function takes."""
    gen: object
    b: int
    r: int
    limits: Optional[Tuple[torch.Tensor, torch.Tensor]]
    has_limits: bool
    u_strat: Optional[torch.Tensor]
    u_imp: Optional[torch.Tensor]
    normals: bool
    normal_grad: bool
    normal_ray_grad: bool
    samples: bool
    compact: bool
    grad: bool
    params: list

    @property
    def lim(self) -> dict:
        return {} if self.limits is None else dict(t_near=self.limits[0], t_far=self.limits[1])


def check_limit_keywords(who: str, t_near, t_far, ray_limits):
    """The keyword rules of per-ray limits, shared by `render_rays` and `trace_rays` → the OccupancyGrid of ``ray_limits`` or None."""
    from .occupancy import OccupancyGrid
    occ = ray_limits if isinstance(ray_limits, OccupancyGrid) else None
    if ray_limits is not None and occ is None and not (isinstance(ray_limits, str) and ray_limits == "box"):
        raise ValueError(f"TriPlaneGenerator.{who}: ray_limits must be None or 'box' or an OccupancyGrid, got {ray_limits!r}")
    if (t_near is None) != (t_far is None):
        raise ValueError(f"TriPlaneGenerator.{who}: t_near and t_far go together (both or neither)")
    if ray_limits is not None and t_near is not None:
        raise ValueError(f"TriPlaneGenerator.{who}: ray_limits='box' / an OccupancyGrid and explicit t_near / t_far are "
                         "mutually exclusive")
    return occ


def check_rays(who: str, gen, ws, ray_origins, ray_directions, occ) -> None:
    """The checks of an occupancy grid against the call and of the rays' shapes and dtypes (before the device is looked at)."""
    if occ is not None:
        if occ.batch not in (1, ws.shape[0]):
            raise ValueError(f"TriPlaneGenerator.{who}: the occupancy grid's batch must be B = {ws.shape[0]} or 1, got "
                             f"{occ.batch}")
        if float(occ.cube_length) != float(gen.cfg.box_warp):
            raise ValueError(f"TriPlaneGenerator.{who}: the occupancy grid's cube_length {occ.cube_length} differs from "
                             f"cfg.box_warp = {gen.cfg.box_warp}")
        if not occ.bits.is_cuda or occ.bits.device != ws.device:
            raise RuntimeError(f"TriPlaneGenerator.{who}: the occupancy grid lives on {occ.bits.device}, ws on {ws.device}; "
                               f"the MI355X path needs CUDA/ROCm tensors; there is no CPU fallback")
    for name, t in (("ray_origins", ray_origins), ("ray_directions", ray_directions)):
        if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] != ws.shape[0]:
            raise ValueError(f"expected {name} [B, R, 3] for ws of batch {ws.shape[0]}, got {tuple(t.shape)}")
        if not t.is_floating_point():
            raise TypeError(f"TriPlaneGenerator.{who}: {name} must be a floating-point tensor, got {t.dtype}")
    if ray_origins.shape != ray_directions.shape:
        raise ValueError(f"ray_directions {tuple(ray_directions.shape)} must match ray_origins {tuple(ray_origins.shape)}")


def limit_tensors(who: str, b: int, r: int, dev, t_near, t_far):
    """Explicit t_near / t_far (tensors [B,R] or floats) as detached fp32 tensors; None when the call gave none."""
    if t_near is None:
        return None
    limits = []
    for name, t in (("t_near", t_near), ("t_far", t_far)):
        if isinstance(t, torch.Tensor):
            if t.shape != (b, r):
                raise ValueError(f"TriPlaneGenerator.{who}: {name} must be [B, R] = [{b}, {r}] or a float, got "
                                 f"{tuple(t.shape)}")
            if not t.is_floating_point():
                raise TypeError(f"TriPlaneGenerator.{who}: {name} must be a floating-point tensor, got {t.dtype}")
            if torch.is_grad_enabled() and t.requires_grad:
                raise NotImplementedError(f"TriPlaneGenerator.{who}: {name} requires grad, but the ray limits are not "
                                          f"differentiated (pass {name}.detach())")
            if not t.is_cuda:
                raise RuntimeError(f"TriPlaneGenerator.{who}: the MI355X path needs CUDA/ROCm tensors; there is no CPU "
                                   "fallback")
            limits.append(t.detach().float().contiguous())
        else:
            limits.append(torch.full((b, r), float(t), device=dev, dtype=torch.float32))
    return tuple(limits)


def box_or_grid_limits(gen, ray_origins, ray_directions, occ):
    """`ray_limits="box"` / an OccupancyGrid as tensors: one launch under no_grad, from detached rays."""
    with torch.no_grad():
        o, d = ray_origins.detach().float().contiguous(), ray_directions.detach().float().contiguous()
        return ops.ray_limits_box(o, d, gen.cfg.box_warp) if occ is None else ops.ray_limits_grid(o, d, occ)


def resolve(gen, ws, ray_origins, ray_directions, u_strat, u_imp, noise_mode, t_near, t_far, ray_limits, normals, normal_grad,
            normal_ray_grad, samples, compact) -> RayCall:
    """Everything `render_rays` does before its first launch of the renderer: the checks (every refusal comes before the device is
    looked at, in this order), the limits as tensors (`ops.ray_limits_box` / `ops.ray_limits_grid` from detached rays) and the
    uniforms.  For B = 0 or R = 0 neither limits nor uniforms are made."""
    if noise_mode != "const":
        raise NotImplementedError("HFA-GP always passes noise_mode='const' (headnerf.py:112)")
    normal_grad = bool(normal_grad or normal_ray_grad)
    normals = bool(normals or normal_grad)
    occ = check_limit_keywords("render_rays", t_near, t_far, ray_limits)
    if compact and ray_limits is None and t_near is None:
        raise ValueError("TriPlaneGenerator.render_rays: compact=True needs ray limits (t_near / t_far or ray_limits=): without "
                         "them every ray is marched")
    check_rays("render_rays", gen, ws, ray_origins, ray_directions, occ)
    if normal_grad and not normal_ray_grad and torch.is_grad_enabled() and (ray_origins.requires_grad or
                                                                             ray_directions.requires_grad):
        raise NotImplementedError("TriPlaneGenerator.render_rays(normal_grad=True): the rays' gradient of the normal term is opt-in "
                                  "(ray_origins / ray_directions require grad): pass normal_ray_grad=True for it, detach the rays, "
                                  "or use normals=True for a detached map")
    gen._query_guard("render_rays", ws, differentiable=True)
    if not (ray_origins.is_cuda and ray_directions.is_cuda):
        raise RuntimeError("TriPlaneGenerator.render_rays: the MI355X path needs CUDA/ROCm tensors; there is no CPU fallback")
    cfg = gen.cfg
    b, r = ray_origins.shape[0], ray_origins.shape[1]
    dev = ws.device
    limits = limit_tensors("render_rays", b, r, dev, t_near, t_far)
    params = [p for n, p in gen.named_parameters() if not n.startswith("backbone.mapping.")]
    grad = torch.is_grad_enabled() and (ws.requires_grad or ray_origins.requires_grad or ray_directions.requires_grad or
                                        any(p.requires_grad for p in params))
    call = RayCall(gen=gen, b=b, r=r, limits=limits, has_limits=limits is not None or ray_limits is not None, u_strat=None, u_imp=None,
                   normals=normals, normal_grad=normal_grad, normal_ray_grad=bool(normal_ray_grad), samples=bool(samples),
                   compact=bool(compact), grad=grad, params=params)
    if b == 0 or r == 0:
        return call
    cap = generator.RAY_STATE_CAP_BYTES
    state_bytes = b * r * (cfg.depth_resolution + cfg.depth_resolution_importance) * 140
    if grad and normal_grad and state_bytes > cap and not compact:      # (compact: the check of the inner call)
        raise RuntimeError(f"TriPlaneGenerator.render_rays(normal_grad=True): the backward of 'normal' reads the ray marcher's "
                           f"per-sample state, {state_bytes} bytes for {b} x {r} rays, above RAY_STATE_CAP_BYTES = "
                           f"{cap}; {cap // (state_bytes // (b * r))} rays fit")
    if ray_limits is not None:
        call.limits = box_or_grid_limits(gen, ray_origins, ray_directions, occ)
    if u_strat is None:
        u_strat = torch.rand(b, r, cfg.depth_resolution, device=dev)
    if u_imp is None:
        u_imp = torch.rand(b * r, cfg.depth_resolution_importance, device=dev)
    call.u_strat, call.u_imp = u_strat.detach().float().reshape(b, r, -1).contiguous(), u_imp.detach().float().contiguous()
    return call


def march(gen, planes, pam, o, d, u_strat, u_imp, lim: dict, normals: bool, samples: bool, keep_state: bool):
    """The forward launches of a list, under no_grad: `ops.raymarch_rays`, with ``normals`` `ops.raymarch_rays_normals` on the
    per-sample state of the march, `ops.depth_clamp_` → ((feature, depth [clamped], mask, normal, sample_weights, sample_depths) —
    None for what was not asked for —, the state or None, the clamp's depth range or None).  ``keep_state``: the caller's backward
    reads the state and the depth range (the autograd function); a state is then kept whenever it fits under the cap, not only for
    the normals.  A state above the cap is not allocated, and normals are then taken in chunks of rays through one state buffer of
    the cap's size: a list may be cut at any ray, and every ray is computed as in the whole-list launch (the decoder's bound on
    |planes| is the call's, taken once), so the results equal the unchunked ones bit for bit."""
    b, r = o.shape[0], o.shape[1]
    sc, sf = u_strat.shape[-1], u_imp.shape[-1]
    smp = dict(samples=True) if samples else {}
    cap = generator.RAY_STATE_CAP_BYTES
    state_bytes = b * r * (sc + sf) * 140
    state = normal = depth_range = None
    empty = dict(empty_rays=True) if lim else {}

    def clamp():
        return (ops.depth_range(tmm, **empty) if keep_state else None), ops.depth_clamp_(depth, tmm, **empty)

    if normals and state_bytes > cap:
        rays = max(1, cap // (state_bytes // r))
        bound = ops._decoder_bound(planes, gen.cfg.decoder_precision, pam)
        buf = ops.raymarch_rays_state(b, min(rays, r), sc, sf, planes.device)
        u_imp = u_imp.view(b, r, sf)
        parts = []
        for r0 in range(0, r, rays):
            n = min(rays, r - r0)
            cut = lambda t: t[:, r0:r0 + n].contiguous()      # noqa: E731
            part = buf.view(-1)[:b * n * (sc + sf) * 35].view(b, n, (sc + sf) * 35)
            oc, dc, us, ui = cut(o), cut(d), cut(u_strat), cut(u_imp).view(b * n, sf)
            lc = {k: cut(t) for k, t in lim.items()}
            out = ops.raymarch_rays(planes, oc, dc, us, ui, planes_absmax=bound, state=part, **lc, **smp, **gen._rays_kwargs())
            parts.append(out + (ops.raymarch_rays_normals(planes, part, ray_origins=oc, ray_directions=dc, u_strat=us, u_imp=ui,
                                                          planes_absmax=bound, **lc, **gen._rays_kwargs()),))
        feat, depth, wsum, tmm, *ws_ts, normal = (torch.cat(t, 1) for t in zip(*parts))
        depth_range, depth = clamp()
    else:
        if (keep_state or normals) and state_bytes <= cap:
            state = ops.raymarch_rays_state(b, r, sc, sf, planes.device)
        feat, depth, wsum, tmm, *ws_ts = gen._timed("raymarch_rays", float(b), ops.raymarch_rays, planes, o, d, u_strat, u_imp,
                                                    planes_absmax=pam, state=state, **lim, **smp, **gen._rays_kwargs())
        if keep_state:           # (a differentiated call has always clamped before its normals launch, a plain one after it)
            depth_range, depth = clamp()
        if normals:
            normal = gen._timed("raymarch_rays_normals", float(b), ops.raymarch_rays_normals, planes, state, ray_origins=o,
                                ray_directions=d, u_strat=u_strat, u_imp=u_imp, planes_absmax=pam, **lim, **gen._rays_kwargs())
        if not keep_state:
            depth_range, depth = clamp()
    return (feat, depth, wsum, normal) + (tuple(ws_ts) if samples else (None, None)), state, depth_range


class RenderRaysFn(torch.autograd.Function):
    """`render_rays` under grad: inputs ws, ray_origins, ray_directions, the RayCall (no tensor: uniforms and limits are detached
    and carry no autograd edge), *parameters; outputs feature [B,R,32], depth [B,R] (clamped to the call's global sample range),
    mask [B,R], normal [B,R,3], sample_weights [B,R,S-1], sample_depths [B,R,S] — None for what the call did not ask for; 'normal'
    is non-differentiable without ``normal_grad``, 'sample_depths' always (importance depths are detached as in EG3D, stratified
    ones are constants of the uniforms).  Forward: a backbone pass with a tape, then `march` keeping the state.
    With limits, d origins / d directions are the derivative with the limits held fixed (EG3D's autograd would also move the sample
    positions through a box intersection: left out on purpose, as the importance depths are), an empty ray gets exactly zero
    gradient and the g_depth it receives is dropped."""
    @staticmethod
    def forward(ctx, ws, ray_origins, ray_directions, call, *params):
        gen = call.gen
        ws_c = ws.detach().float().contiguous()
        o, d = ray_origins.detach().float().contiguous(), ray_directions.detach().float().contiguous()
        tape = []
        with torch.no_grad():
            planes = gen.backbone_planes(ws_c, tape)
            pam = getattr(gen, "_planes_absmax", None)
            out, state, depth_range = march(gen, planes, pam, o, d, call.u_strat, call.u_imp, call.lim, call.normals, call.samples,
                                            keep_state=True)
        ctx.call, ctx.tape, ctx.ws_c, ctx.planes, ctx.pam, ctx.state = call, tape, ws_c, planes, pam, state
        ctx.rays, ctx.depth_range = (o, d), depth_range
        ctx.params = params
        ctx.pg = any(p.requires_grad for p in params)
        ctx.ws_shape, ctx.ray_dtypes = ws.shape, (ray_origins.dtype, ray_directions.dtype)
        ctx.mark_non_differentiable(*(t for t in (None if call.normal_grad else out[3], out[5]) if t is not None))
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.no_grad()
    def backward(ctx, g_feat, g_depth, g_wsum, g_normal, g_weights, _g_depths):
        """Nothing if no gradient arrived.  The colour term (`ops.raymarch_rays_bwd`, with the decoder gradients when parameters
        require grad) only if feature, depth, mask or sample_weights carry a gradient — the weights' is one more addend of its pass 1,
        so it runs for them alone too — and BEFORE the normal term: on mirrored planes it overwrites plane 2, while
        `ops.raymarch_rays_normals_bwd` adds to every plane at its true texels.  That one runs only if g_normal arrived, into the same
        d_planes and decoder gradients, or fresh zeros.  Then, when the rays require grad, the rays' passes: the colour term's (it
        reads that launch's records, which carry the depth, opacity and weight terms), then with ``normal_ray_grad`` the normal
        term's accumulated into it (into fresh records without a colour term) — the per-ray record is itself the answer, torch
        autograd carries it on to a camera model.  Last the one backbone backward `synthesis` runs."""
        call, gen = ctx.call, ctx.call.gen
        if ctx.tape is None:
            raise RuntimeError("TriPlaneGenerator.render_rays: backward called a second time — the saved activations are released "
                               "by the first backward pass (retain_graph is not supported)")
        if g_feat is None and g_depth is None and g_wsum is None and g_normal is None and g_weights is None:
            return (None,) * (4 + len(ctx.params))
        if g_normal is not None and ctx.state is None:
            raise RuntimeError("TriPlaneGenerator.render_rays(normal_grad=True): the forward kept no per-sample state "
                               "(RAY_STATE_CAP_BYTES)")
        planes = ctx.planes
        b, dev = planes.shape[0], planes.device
        o, d = ctx.rays
        r = o.shape[1]
        d_ws = torch.zeros(ctx.ws_shape, device=dev, dtype=torch.float32)
        bw = _Backward(gen, None, d_ws, ctx.ws_c, ctx.pg)
        g_feat = None if g_feat is None else g_feat.float().contiguous()
        geom = {}
        if g_depth is not None:
            geom.update(g_depth=g_depth.float().reshape(b, r).contiguous(), depth_range=ctx.depth_range)
        if g_wsum is not None:
            geom.update(g_wsum=g_wsum.float().reshape(b, r).contiguous())
        if g_weights is not None:
            geom.update(g_weights=g_weights.float().reshape(b, r, -1).contiguous())
        colour = g_feat is not None or bool(geom)
        need_rays = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        rays = dict(ray_origins=o, ray_directions=d, u_strat=call.u_strat, u_imp=call.u_imp, planes_absmax=ctx.pam, **call.lim,
                    **gen._rays_kwargs())
        d_planes = dec = d_o = d_d = None
        rec_out = [] if need_rays else None
        if colour:
            rb = gen._timed("raymarch_rays_bwd", float(b), ops.raymarch_rays_bwd, g_feat, planes, decoder_grads=ctx.pg, state=ctx.state,
                            rec_out=rec_out, **geom, **rays)
            d_planes, dec = rb if ctx.pg else (rb, None)
        if g_normal is not None:
            g_normal = g_normal.float().reshape(b, r, 3).contiguous()
            d_planes, dec = gen._timed("raymarch_rays_normals_bwd", float(b), ops.raymarch_rays_normals_bwd, g_normal, planes, ctx.state,
                                       d_planes=d_planes, decoder_grads=ctx.pg, dec_out=dec, **rays)
        if need_rays:
            if colour:
                d_o, d_d = gen._timed("raymarch_rays_bwd_rays", float(b), ops.raymarch_rays_bwd_rays, g_feat, planes, rec_out[0], **rays)
            if g_normal is not None and call.normal_ray_grad:
                d_o, d_d = gen._timed("raymarch_rays_normals_bwd_rays", float(b), ops.raymarch_rays_normals_bwd_rays, g_normal, planes,
                                      ctx.state, d_origins=d_o, d_directions=d_d, **rays)
            if d_o is not None:
                d_o, d_d = (d_o.to(ctx.ray_dtypes[0]) if ctx.needs_input_grad[1] else None,
                            d_d.to(ctx.ray_dtypes[1]) if ctx.needs_input_grad[2] else None)
        if ctx.pg:
            for prm, g in zip(gen.decoder_params(), dec):
                bw._acc(prm, g)
        _backbone_backward(bw, gen, ctx.tape, d_planes, b, dev)
        ctx.tape = ctx.planes = ctx.state = None
        pgrads = tuple(bw.grads.get(id(p)) if p.requires_grad else None for p in ctx.params)
        return (d_ws, d_o, d_d, None) + pgrads


def _empty(b: int, r: int, dev, zero, limits: bool, normals: bool, normal_grad: bool, samples: int = 0) -> Dict[str, torch.Tensor]:
    """`render_rays` of no rays (B = 0 or R = 0): the dict of a call with these keywords, nothing launched.  ``zero``: 0.0, or
    under grad a zero scalar that hangs on the call's inputs and keeps their autograd edges."""
    feat = torch.zeros(b, r, 32, device=dev) + zero
    out = {"feature": feat, "rgb": feat[..., :3], "depth": torch.zeros(b, r, device=dev) + zero,
           "mask": torch.zeros(b, r, device=dev) + zero}
    if limits:
        out["valid"] = torch.zeros(b, r, device=dev, dtype=torch.bool)
    if normals:          # (detached unless normal_grad, as in a call with rays)
        out["normal"] = torch.zeros(b, r, 3, device=dev) + (zero if normal_grad else 0.0)
    if samples:          # (S = Sc + Sf of the config; the depths are detached, as in a call with rays)
        out["sample_weights"] = torch.zeros(b, r, samples - 1, device=dev) + zero
        out["sample_depths"] = torch.zeros(b, r, samples, device=dev)
    return out


def _empty_of(call: RayCall, ws, ray_origins, ray_directions) -> Dict[str, torch.Tensor]:
    """`_empty` for the keywords of ``call``."""
    cfg = call.gen.cfg
    zero = 0.0 * ws.sum() + 0.0 * ray_origins.sum() + 0.0 * ray_directions.sum() if call.grad else 0.0      # keeps the autograd edges
    return _empty(call.b, call.r, ws.device, zero, call.has_limits, call.normals, call.normal_grad,
                  cfg.depth_resolution + cfg.depth_resolution_importance if call.samples else 0)


def _compact(call: RayCall, ws, ray_origins, ray_directions):
    """`render_rays(compact=True)` once the limits are tensors: the valid rays of every frame first (stable), the first R' + 1 of
    them marched by a plain `render_rays(t_near=, t_far=)` call, the results scattered back over the empty-ray values.  None when
    a frame has no empty ray (nothing to leave out: the caller goes on as without the keyword).  The + 1: an empty ray is not
    marched, and its 'depth' is what every empty ray of the call gets — the upper end of the clamp range over the valid rays,
    which are the same rays in both calls."""
    from .cam_utils import ray_limits_valid
    gen, b, r = call.gen, call.b, call.r
    u_strat, u_imp = call.u_strat, call.u_imp
    background = 1.0 if gen.cfg.white_back else -1.0
    valid = ray_limits_valid(*call.limits)
    n_valid = int(valid.sum(1).max())                  # (the one host sync)
    if n_valid == r:
        return None
    if n_valid == 0:
        out = _empty_of(call, ws, ray_origins, ray_directions)
        out["feature"] = out["feature"] + background
        out["rgb"] = out["feature"][..., :3]
        return out
    m = n_valid + 1
    idx = torch.argsort((~valid).to(torch.uint8), dim=1, stable=True)[:, :m]              # [B, m]: the valid rays, then empty ones
    idx3 = idx[..., None].expand(b, m, 3)
    sf = u_imp.shape[-1]
    sub = gen.render_rays(ws, ray_origins.gather(1, idx3), ray_directions.gather(1, idx3),
                          u_strat.gather(1, idx[..., None].expand(b, m, u_strat.shape[-1])),
                          u_imp.view(b, r, sf).gather(1, idx[..., None].expand(b, m, sf)).reshape(b * m, sf),
                          t_near=call.limits[0].gather(1, idx), t_far=call.limits[1].gather(1, idx), normals=call.normals,
                          normal_grad=call.normal_grad, normal_ray_grad=call.normal_ray_grad, samples=call.samples)
    fill = {"feature": background, "depth": sub["depth"][0, -1].detach(), "mask": 0.0, "normal": 0.0, "sample_weights": 0.0,
            "sample_depths": 0.0}
    out = {}
    for key, val in sub.items():
        if key in ("rgb", "valid"):
            continue
        full = torch.empty(b, r, *val.shape[2:], device=ws.device, dtype=val.dtype)
        full[...] = fill[key]
        out[key] = full.scatter(1, idx.reshape(b, m, *([1] * (val.dim() - 2))).expand_as(val), val)
    out["rgb"] = out["feature"][..., :3]
    out["valid"] = valid
    return out


def render_rays(gen, ws, ray_origins, ray_directions, *options) -> Dict[str, torch.Tensor]:
    """`TriPlaneGenerator.render_rays`; ``options``: the other parameters of the method, in its order (`resolve` names them)."""
    call = resolve(gen, ws, ray_origins, ray_directions, *options)
    if call.b == 0 or call.r == 0:
        return _empty_of(call, ws, ray_origins, ray_directions)
    if call.compact:
        out = _compact(call, ws, ray_origins, ray_directions)
        if out is not None:
            return out
    if call.grad:
        if getattr(gen, "_grad_sink", None) is not None or getattr(gen, "_grad_inplace", False):
            raise RuntimeError("TriPlaneGenerator.render_rays under grad inside a trainer step scope: its backward is a second "
                               "backbone pass and would release every parameter to the gradient sink twice")
        feat, depth, mask, normal, weights, depths = RenderRaysFn.apply(ws, ray_origins, ray_directions, call, *call.params)
    else:
        with torch.no_grad():
            planes, pam = gen._query_planes(ws)
            o, d = ray_origins.detach().float().contiguous(), ray_directions.detach().float().contiguous()
            (feat, depth, mask, normal, weights, depths), _, _ = march(gen, planes, pam, o, d, call.u_strat, call.u_imp, call.lim,
                                                                       call.normals, call.samples, keep_state=False)
    out = {"feature": feat, "rgb": feat[..., :3], "depth": depth, "mask": mask}
    if call.normals:
        out["normal"] = normal
    if call.samples:
        out["sample_weights"], out["sample_depths"] = weights, depths
    if call.limits is not None:
        from .cam_utils import ray_limits_valid
        out["valid"] = ray_limits_valid(*call.limits)
    return out


# ------------------------------------------------------------------ the first hit with the density iso-surface
def trace_rays(gen, ws, ray_origins, ray_directions, level, steps, refine, t_near, t_far, ray_limits, normals,
               differentiable) -> Dict[str, torch.Tensor]:
    """`TriPlaneGenerator.trace_rays` (its docstring is the public description): the checks and the limits of `render_rays`, one
    backbone pass, one launch (`ops.trace_rays`); with ``differentiable`` the root's implicit gradient (`ray_losses.implicit_depth`)
    through the differentiable point query."""
    who = "trace_rays"
    occ = check_limit_keywords(who, t_near, t_far, ray_limits)
    check_rays(who, gen, ws, ray_origins, ray_directions, occ)
    if not 1 <= int(steps) <= 4096:
        raise ValueError(f"TriPlaneGenerator.{who}: steps must be in [1, 4096], got {steps}")
    if not 0 <= int(refine) <= 30:
        raise ValueError(f"TriPlaneGenerator.{who}: refine must be in [0, 30], got {refine}")
    params = [p for n, p in gen.named_parameters() if not n.startswith("backbone.mapping.")]
    grad = bool(differentiable) and torch.is_grad_enabled() and (
        ws.requires_grad or ray_origins.requires_grad or ray_directions.requires_grad or any(p.requires_grad for p in params))
    gen._query_guard(who, ws, *(() if differentiable else (ray_origins, ray_directions)), differentiable=bool(differentiable))
    if not (ray_origins.is_cuda and ray_directions.is_cuda):
        raise RuntimeError(f"TriPlaneGenerator.{who}: the MI355X path needs CUDA/ROCm tensors; there is no CPU fallback")
    cfg = gen.cfg
    b, r = ray_origins.shape[0], ray_origins.shape[1]
    dev = ws.device
    limits = limit_tensors(who, b, r, dev, t_near, t_far)
    has_limits = limits is not None or ray_limits is not None
    if b == 0 or r == 0:
        zero = 0.0 * ws.sum() + 0.0 * ray_origins.sum() + 0.0 * ray_directions.sum() if grad else 0.0     # keeps the autograd edges
        out = {"hit": torch.zeros(b, r, device=dev, dtype=torch.bool), "cell": torch.zeros(b, r, device=dev, dtype=torch.int32),
               "t": torch.zeros(b, r, device=dev) + zero, "point": torch.zeros(b, r, 3, device=dev) + zero,
               "sigma": torch.zeros(b, r, device=dev)}
        if normals or grad:
            out.update(sigma_grad=torch.zeros(b, r, 3, device=dev), normal=torch.zeros(b, r, 3, device=dev))
        if has_limits:
            out["valid"] = torch.zeros(b, r, device=dev, dtype=torch.bool)
        return out
    if grad and (getattr(gen, "_grad_sink", None) is not None or getattr(gen, "_grad_inplace", False)):
        raise RuntimeError("TriPlaneGenerator.trace_rays(differentiable=True) inside a trainer step scope: its backward is a second "
                           "backbone pass and would release every parameter to the gradient sink twice — trace under no_grad and "
                           "pass the points through `synthesis(..., query=)` with `ray_losses.implicit_depth` instead")
    if ray_limits is not None:
        limits = box_or_grid_limits(gen, ray_origins, ray_directions, occ)
    elif limits is None:
        limits = tuple(torch.full((b, r), float(v), device=dev, dtype=torch.float32) for v in (cfg.ray_start, cfg.ray_end))
    want = ops._TRACE_OUT if (normals or grad) else tuple(k for k in ops._TRACE_OUT if k not in ("sigma_grad", "normal"))
    with torch.no_grad():
        planes, pam = gen._query_planes(ws)
        o, d = ray_origins.detach().float().contiguous(), ray_directions.detach().float().contiguous()
        out = gen._timed("trace_rays", float(b), ops.trace_rays, planes, o, d, limits[0], limits[1], float(level), int(steps),
                         int(refine), pam, want, **gen._query_kwargs())
    out["hit"] = out["hit"].bool()
    if has_limits:
        from .cam_utils import ray_limits_valid
        out["valid"] = ray_limits_valid(*limits)
    if grad:
        from .ray_losses import implicit_depth, transversal
        # the rays on the formula; every other ray keeps 't' and 'point' as constants
        carries = out["hit"] & (out["cell"] > 0) & transversal(out["sigma_grad"], d)
        t0, x0 = out["t"], out["point"]
        # the hit point as a function of the rays (t held fixed), so that the point query's backward reaches them
        x = torch.where(carries[..., None], ray_origins + t0[..., None] * ray_directions, x0)
        sig = gen.sample_mixed(x, None, ws, differentiable=True)["sigma"]
        out["t"] = t = implicit_depth(t0, sig, out["sigma_grad"], d, mask=carries)
        out["point"] = torch.where(carries[..., None], ray_origins + t[..., None] * ray_directions, x0)
        if not normals:
            del out["sigma_grad"], out["normal"]
    return out
