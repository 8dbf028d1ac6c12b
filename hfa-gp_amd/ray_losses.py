"""Ray regularisers and depth statistics on the per-sample outputs of ``TriPlaneGenerator.render_rays(samples=True)``.

Plain torch, any device and dtype; differentiable w.r.t. ``sample_weights`` (``sample_depths`` is a constant of the renderer).
Inputs throughout: ``sample_depths`` [..., S], ascending, and ``sample_weights`` [..., S-1], where w_e is the compositing weight
of the interval [t_e, t_{e+1}] with midpoint t̄_e = (t_e + t_{e+1}) / 2 and width Δ_e = t_{e+1} - t_e.  An empty ray (all-zero rows
in both) gives 0 in `distortion_loss` and `depth_variance`, and its upper end — 0 — in `quantile_depth`.
`implicit_depth` is the odd one out: it works on the outputs of ``TriPlaneGenerator.trace_rays`` and makes a traced surface depth
differentiable.
"""
from __future__ import annotations

import torch

__all__ = ["distortion_loss", "quantile_depth", "depth_variance", "implicit_depth", "transversal"]


def _check(sample_depths: torch.Tensor, sample_weights: torch.Tensor) -> None:
    if sample_depths.shape[-1] < 2 or sample_weights.shape != sample_depths.shape[:-1] + (sample_depths.shape[-1] - 1,):
        raise ValueError(f"expected sample_depths [..., S] and sample_weights [..., S-1], got {tuple(sample_depths.shape)} and "
                         f"{tuple(sample_weights.shape)}")


def distortion_loss(sample_depths: torch.Tensor, sample_weights: torch.Tensor, t_range=None) -> torch.Tensor:
    """The distortion loss of mip-NeRF 360 per ray, [...]:  Σ_{i,j} w_i w_j |t̄_i − t̄_j| + ⅓ Σ_i w_i² Δ_i  — small when the weight
    sits in one compact place along the ray; against floaters and semi-transparent shells.  O(S): the midpoints ascend, so the
    double sum is 2 Σ_i w_i (t̄_i Σ_{j<i} w_j − Σ_{j<i} w_j t̄_j), two exclusive cumulative sums.
    ``t_range`` = (near, far), scalars or tensors broadcastable to [...]: the depths are first mapped to [0, 1], s = (t − near) /
    (far − near), which makes the loss independent of the scene's scale (the per-ray limits of the call, or the config's
    interval).  A ray whose range is not finite or not positive (an empty ray) is mapped to s = 0 and contributes 0."""
    _check(sample_depths, sample_weights)
    t = sample_depths.detach().to(sample_weights.dtype)
    if t_range is not None:
        near, far = (torch.as_tensor(x, dtype=t.dtype, device=t.device) for x in t_range)
        span = far - near
        ok = torch.isfinite(near) & torch.isfinite(far) & (span > 0)
        near, span = torch.where(ok, near, torch.zeros_like(near)), torch.where(ok, span, torch.ones_like(span))
        t = torch.where(ok.unsqueeze(-1), (t - near.unsqueeze(-1)) / span.unsqueeze(-1), torch.zeros_like(t))
    w = sample_weights
    mid, delta = 0.5 * (t[..., 1:] + t[..., :-1]), t[..., 1:] - t[..., :-1]
    cw = torch.cumsum(w, -1) - w                   # exclusive: Σ_{j<i} w_j
    cwm = torch.cumsum(w * mid, -1) - w * mid      # Σ_{j<i} w_j t̄_j
    return 2.0 * (w * (mid * cw - cwm)).sum(-1) + (w * w * delta).sum(-1) / 3.0


def quantile_depth(sample_depths: torch.Tensor, sample_weights: torch.Tensor, q: float = 0.5) -> torch.Tensor:
    """The depth at which the cumulative weight reaches q·Σw, [...] (q = 0.5: the median depth — unlike the expected depth it does not
    blur across a depth edge: unprojection, point clouds).  The weight of an interval is taken as spread evenly over it: linear
    interpolation inside the first interval whose cumulative weight reaches q·Σw.  Where Σw = 0 (nothing hit, an empty ray): the
    upper end of the ray, t_{S−1}.  Not differentiable in a useful way (piecewise in the weights): computed under no_grad."""
    _check(sample_depths, sample_weights)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"q must lie in [0, 1], got {q}")
    with torch.no_grad():
        t, w = sample_depths, sample_weights.to(sample_depths.dtype)
        cum = torch.cumsum(w, -1)
        total = cum[..., -1:]
        target = q * total
        e = torch.searchsorted(cum.contiguous(), target.contiguous()).clamp_(max=w.shape[-1] - 1)      # first e with cum_e >= target
        we = w.gather(-1, e)
        before = cum.gather(-1, e) - we
        frac = torch.where(we > 0, (target - before) / torch.where(we > 0, we, torch.ones_like(we)), torch.zeros_like(we)).clamp_(0, 1)
        t0, t1 = t.gather(-1, e), t.gather(-1, e + 1)
        out = t0 + frac * (t1 - t0)
        return torch.where(total > 0, out, t[..., -1:]).squeeze(-1)


def depth_variance(sample_depths: torch.Tensor, sample_weights: torch.Tensor) -> torch.Tensor:
    """Σ_e w_e (t̄_e − d)² / Σ_e w_e with d = Σ_e w_e t̄_e / Σ_e w_e the expected depth, [...]: the spread of the ray's termination
    depth, an uncertainty map.  0 where Σw = 0."""
    _check(sample_depths, sample_weights)
    t = sample_depths.detach().to(sample_weights.dtype)
    w = sample_weights
    mid = 0.5 * (t[..., 1:] + t[..., :-1])
    total = w.sum(-1, keepdim=True)
    hit = total > 0
    safe = torch.where(hit, total, torch.ones_like(total))
    d = (w * mid).sum(-1, keepdim=True) / safe
    var = (w * (mid - d) ** 2).sum(-1, keepdim=True) / safe
    return torch.where(hit, var, torch.zeros_like(var)).squeeze(-1)


def transversal(sigma_grad: torch.Tensor, directions: torch.Tensor, slope_floor: float = 0.01) -> torch.Tensor:
    """The rays that enter the surface at a slope `implicit_depth` accepts, bool [...]: g·d ≥ ``slope_floor``·‖g‖·‖d‖ and g·d > 0 for
    g = ``sigma_grad`` [..., 3] and d = ``directions`` [..., 3] (the density rises along the ray; a grazing crossing is left out)."""
    gd = (sigma_grad * directions).sum(-1)
    return (gd >= slope_floor * sigma_grad.norm(dim=-1) * directions.norm(dim=-1)) & (gd > 0)


def implicit_depth(t: torch.Tensor, sigma: torch.Tensor, sigma_grad: torch.Tensor, directions: torch.Tensor,
                   slope_floor: float = 0.01, mask=None) -> torch.Tensor:
    """A traced surface depth made differentiable by the implicit function theorem, [...]: the value of ``t`` with the gradient of
    the root of σ(o + t·d) = level.  ``t`` [...]: the root a trace found (`TriPlaneGenerator.trace_rays` under no_grad), a constant
    here; ``sigma`` [...] (or [..., 1]): the raw density at the hit point o + t·d, evaluated DIFFERENTIABLY — `sample_mixed(...,
    differentiable=True)`, or `synthesis(query=)` inside a trainer step, so that the surface term shares the image's backward pass;
    when the rays need a gradient too, form the point from them (t detached); ``sigma_grad`` [..., 3]: g = ∂σ/∂x there, a constant;
    ``directions`` [..., 3]: d, a constant.  Returns

        t − (σ − σ.detach()) / (g·d)        dt = −dσ / (g·d): moving the field by dσ at the hit moves the root by that much

    A ray carries this gradient only where the crossing is transversal, g·d ≥ ``slope_floor``·‖g‖·‖d‖ (and g·d > 0), and, with
    ``mask`` (bool [...]), inside the mask — pass ``hit & (cell > 0)``: a miss has no root and a ray that starts inside has the
    constant t = t_near.  Every other ray returns ``t`` as a constant: exactly zero gradient.  Plain torch, any device and dtype."""
    if sigma.dim() == t.dim() + 1 and sigma.shape[-1] == 1:
        sigma = sigma.squeeze(-1)
    if sigma.shape != t.shape or sigma_grad.shape != t.shape + (3,) or directions.shape != sigma_grad.shape:
        raise ValueError(f"expected t [...], sigma [...] or [..., 1], sigma_grad and directions [..., 3], got {tuple(t.shape)}, "
                         f"{tuple(sigma.shape)}, {tuple(sigma_grad.shape)}, {tuple(directions.shape)}")
    t = t.detach().to(sigma.dtype)
    g, d = sigma_grad.detach().to(sigma.dtype), directions.detach().to(sigma.dtype)
    gd = (g * d).sum(-1)
    ok = transversal(g, d, slope_floor)
    if mask is not None:
        ok = ok & mask
    step = (sigma - sigma.detach()) / torch.where(ok, gd, torch.ones_like(gd))
    return t - torch.where(ok, step, torch.zeros_like(step))
