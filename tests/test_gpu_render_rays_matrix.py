"""Every keyword combination of TriPlaneGenerator.render_rays on the device: which ops it launches in which order and with which
optional arguments (against a table recorded on the commit before hfa-gp_amd/ray_list.py existed), that a keyword leaves the
entries it shares with the plain call bit-identical, which outputs require grad, and the march above RAY_STATE_CAP_BYTES.
Needs an MI355X:  python -m pytest tests -m gpu

The tiny64 generator of tests/test_gpu_normal_grad.py with every non-mapping parameter requiring grad (so the decoder gradients
accumulate across the colour and the normal term), B = 2, R = 101 (not a multiple of 64): test_gpu_render_rays.ray_list() — every
ray meets the box, so `compact=True` finds nothing to leave out — and ray_limits_ref.miss_list(), 20 of whose rays per frame are
empty under "box", in both frames.  No tolerance anywhere: the comparisons are of launch traces and of bits."""
import inspect
import itertools

import pytest
import torch

from tests import ray_limits_ref as RL
from tests.test_gpu_normal_grad import _cfg, _gen, _inputs

pytestmark = pytest.mark.gpu

B, R = RL.B, RL.R
MODES = {"none": {}, "normals": dict(normals=True), "normal_grad": dict(normal_grad=True), "normal_ray_grad": dict(normal_ray_grad=True)}
LIMITS = ("none", "explicit", "box")
LOSSES = ("all", "normal", "feature")
TRACED_EXTRA = ("ray_limits_box", "depth_clamp_")
TRACKED = ("state", "t_near", "samples", "g_depth", "g_wsum", "g_weights", "d_planes", "dec_out", "d_origins")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gen(dev):
    return _gen(dev, tuned=True)


class Recorder:
    """Wraps every ops.raymarch_rays*, ops.ray_limits_box and ops.depth_clamp_; `trace` is the list of "name:arg,arg" of the calls
    so far, the args being those of TRACKED that the call got as something other than None / False."""
    def __init__(self, ops):
        self.ops, self.trace, self.saved = ops, [], {}
        self.names = sorted(n for n in dir(ops) if n.startswith("raymarch_rays") and callable(getattr(ops, n))) + list(TRACED_EXTRA)

    def __enter__(self):
        for name in self.names:
            inner = self.saved[name] = getattr(self.ops, name)
            setattr(self.ops, name, self._wrap(name, inner, inspect.signature(inner)))
        return self

    def __exit__(self, *exc):
        for name, inner in self.saved.items():
            setattr(self.ops, name, inner)

    def _wrap(self, name, inner, sig):
        def recorded(*a, **k):
            given = sig.bind(*a, **k).arguments
            self.trace.append(name + ":" + ",".join(t for t in TRACKED if given.get(t) is not None and given.get(t) is not False))
            return inner(*a, **k)
        return recorded

    def take(self):
        out, self.trace = " | ".join(self.trace), []
        return out


def cells():
    """(samples, mode, limits, compact, list) of the matrix; compact only where limits exist, the all-valid list only where it takes
    another path than the list with empty rays (no limits; compact=True with nothing to leave out)."""
    for samples, mode, limits in itertools.product((False, True), MODES, LIMITS):
        if limits == "none":
            yield samples, mode, limits, False, "r27"
            continue
        for compact in (False, True):
            yield samples, mode, limits, compact, "miss"
        yield samples, mode, limits, True, "r27"


def cell_id(samples, mode, limits, compact, rays):
    return f"{'samples' if samples else 'plain'}/{mode}/{limits}/{'compact' if compact else 'whole'}/{rays}"


def inputs(dev, rays, limits, grad_rays):
    """ws (requires grad), the list, its uniforms and the limit keywords; "explicit" = the box's limits as tensors."""
    from hfa_gp_amd import ops
    cfg = _cfg()
    ws = _inputs(dev)[0].requires_grad_(True)
    o, d = (t.to(dev).requires_grad_(grad_rays) for t in RL.LISTS[rays]())
    g = torch.Generator().manual_seed(31)
    us = torch.rand(B, R, cfg.depth_resolution, generator=g).to(dev)
    ui = torch.rand(B * R, cfg.depth_resolution_importance, generator=g).to(dev)
    kw = {}
    if limits == "box":
        kw = dict(ray_limits="box")
    elif limits == "explicit":
        kw = dict(zip(("t_near", "t_far"), ops.ray_limits_box(o.detach(), d.detach(), cfg.box_warp)))
    return ws, o, d, us, ui, kw


def loss_of(out, which):
    if which == "normal":
        return out["normal"].sum()
    if which == "feature":
        return out["feature"].sum()
    return sum(v.sum() for k, v in out.items() if k != "rgb" and v.requires_grad)


def run_cell(gen, dev, rec, samples, mode, limits, compact, rays):
    """One cell without grad and under grad (the rays requiring grad, but for normal_grad without the opt-in, which refuses them)
    -> ({"nograd" / loss name: trace}, the no-grad dict, the under-grad dict of the "all" loss)."""
    kw = dict(MODES[mode], samples=samples, compact=compact)
    traces = {}
    ws, o, d, us, ui, lim = inputs(dev, rays, limits, False)
    rec.take()
    with torch.no_grad():
        plain = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, **lim, **kw)
    traces["nograd"] = rec.take()
    under = None
    for which in LOSSES:
        if which == "normal" and mode not in ("normal_grad", "normal_ray_grad"):
            continue
        ws, o, d, us, ui, lim = inputs(dev, rays, limits, mode != "normal_grad")
        rec.take()
        out = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, **lim, **kw)
        loss_of(out, which).backward()
        traces[which] = rec.take()
        assert ws.grad is not None and bool(torch.isfinite(ws.grad).all())
        if which == "all":
            under = out
    gen.zero_grad(set_to_none=True)
    return traces, plain, under


# The launch traces of the commit before this file, de54b8d ("Occupancy grids for ray lists"), recorded there with the Recorder
# above on the cells above: trace -> the cells (cell id @ "nograd" or the loss) that gave it.
PARENT_TRACES = {
    "raymarch_rays: | depth_clamp_:":
        "plain/none/none/whole/r27@nograd",
    ("raymarch_rays_state: | raymarch_rays:state | depth_clamp_: | raymarch_rays_bwd:state,g_depth,g_wsum | "
     "raymarch_rays_bwd_rays:"):
        "plain/none/none/whole/r27@all",
    "raymarch_rays_state: | raymarch_rays:state | depth_clamp_: | raymarch_rays_bwd:state | raymarch_rays_bwd_rays:":
        "plain/none/none/whole/r27@feature",
    "raymarch_rays:t_near | depth_clamp_:":
        "plain/none/explicit/whole/miss@nograd plain/none/explicit/compact/miss@nograd plain/none/explicit/compact/r27@nograd",
    ("raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_bwd:state,t_near,g_depth,g_wsum | "
     "raymarch_rays_bwd_rays:t_near"):
        "plain/none/explicit/whole/miss@all plain/none/explicit/compact/miss@all plain/none/explicit/compact/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_bwd:state,t_near | "
     "raymarch_rays_bwd_rays:t_near"):
        "plain/none/explicit/whole/miss@feature plain/none/explicit/compact/miss@feature "
        "plain/none/explicit/compact/r27@feature",
    "ray_limits_box: | raymarch_rays:t_near | depth_clamp_:":
        "plain/none/box/whole/miss@nograd plain/none/box/compact/miss@nograd plain/none/box/compact/r27@nograd",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | "
     "raymarch_rays_bwd:state,t_near,g_depth,g_wsum | raymarch_rays_bwd_rays:t_near"):
        "plain/none/box/whole/miss@all plain/none/box/compact/miss@all plain/none/box/compact/r27@all",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_bwd:state,t_near | "
     "raymarch_rays_bwd_rays:t_near"):
        "plain/none/box/whole/miss@feature plain/none/box/compact/miss@feature plain/none/box/compact/r27@feature",
    "raymarch_rays_state: | raymarch_rays:state | raymarch_rays_normals:state | depth_clamp_:":
        "plain/normals/none/whole/r27@nograd plain/normal_grad/none/whole/r27@nograd "
        "plain/normal_ray_grad/none/whole/r27@nograd",
    ("raymarch_rays_state: | raymarch_rays:state | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_bwd:state,g_depth,g_wsum | raymarch_rays_bwd_rays:"):
        "plain/normals/none/whole/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state | depth_clamp_: | raymarch_rays_normals:state | raymarch_rays_bwd:state | "
     "raymarch_rays_bwd_rays:"):
        "plain/normals/none/whole/r27@feature plain/normal_ray_grad/none/whole/r27@feature",
    "raymarch_rays_state: | raymarch_rays:state,t_near | raymarch_rays_normals:state,t_near | depth_clamp_:":
        "plain/normals/explicit/whole/miss@nograd plain/normals/explicit/compact/miss@nograd "
        "plain/normals/explicit/compact/r27@nograd plain/normal_grad/explicit/whole/miss@nograd "
        "plain/normal_grad/explicit/compact/miss@nograd plain/normal_grad/explicit/compact/r27@nograd "
        "plain/normal_ray_grad/explicit/whole/miss@nograd plain/normal_ray_grad/explicit/compact/miss@nograd "
        "plain/normal_ray_grad/explicit/compact/r27@nograd",
    ("raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near,g_depth,g_wsum | raymarch_rays_bwd_rays:t_near"):
        "plain/normals/explicit/whole/miss@all plain/normals/explicit/compact/miss@all plain/normals/explicit/compact/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near | raymarch_rays_bwd_rays:t_near"):
        "plain/normals/explicit/whole/miss@feature plain/normals/explicit/compact/miss@feature "
        "plain/normals/explicit/compact/r27@feature plain/normal_ray_grad/explicit/whole/miss@feature "
        "plain/normal_ray_grad/explicit/compact/miss@feature plain/normal_ray_grad/explicit/compact/r27@feature",
    "ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | raymarch_rays_normals:state,t_near | depth_clamp_:":
        "plain/normals/box/whole/miss@nograd plain/normals/box/compact/miss@nograd plain/normals/box/compact/r27@nograd "
        "plain/normal_grad/box/whole/miss@nograd plain/normal_grad/box/compact/miss@nograd "
        "plain/normal_grad/box/compact/r27@nograd plain/normal_ray_grad/box/whole/miss@nograd "
        "plain/normal_ray_grad/box/compact/miss@nograd plain/normal_ray_grad/box/compact/r27@nograd",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near,g_depth,g_wsum | raymarch_rays_bwd_rays:t_near"):
        "plain/normals/box/whole/miss@all plain/normals/box/compact/miss@all plain/normals/box/compact/r27@all",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near | raymarch_rays_bwd_rays:t_near"):
        "plain/normals/box/whole/miss@feature plain/normals/box/compact/miss@feature plain/normals/box/compact/r27@feature "
        "plain/normal_ray_grad/box/whole/miss@feature plain/normal_ray_grad/box/compact/miss@feature "
        "plain/normal_ray_grad/box/compact/r27@feature",
    ("raymarch_rays_state: | raymarch_rays:state | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_bwd:state,g_depth,g_wsum | raymarch_rays_normals_bwd:state,d_planes,dec_out"):
        "plain/normal_grad/none/whole/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_normals_bwd:state"):
        "plain/normal_grad/none/whole/r27@normal",
    "raymarch_rays_state: | raymarch_rays:state | depth_clamp_: | raymarch_rays_normals:state | raymarch_rays_bwd:state":
        "plain/normal_grad/none/whole/r27@feature",
    ("raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near,g_depth,g_wsum | raymarch_rays_normals_bwd:state,t_near,d_planes,dec_out"):
        "plain/normal_grad/explicit/whole/miss@all plain/normal_grad/explicit/compact/miss@all "
        "plain/normal_grad/explicit/compact/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_normals_bwd:state,t_near"):
        "plain/normal_grad/explicit/whole/miss@normal plain/normal_grad/explicit/compact/miss@normal "
        "plain/normal_grad/explicit/compact/r27@normal",
    ("raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near"):
        "plain/normal_grad/explicit/whole/miss@feature plain/normal_grad/explicit/compact/miss@feature "
        "plain/normal_grad/explicit/compact/r27@feature",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near,g_depth,g_wsum | "
     "raymarch_rays_normals_bwd:state,t_near,d_planes,dec_out"):
        "plain/normal_grad/box/whole/miss@all plain/normal_grad/box/compact/miss@all plain/normal_grad/box/compact/r27@all",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_normals_bwd:state,t_near"):
        "plain/normal_grad/box/whole/miss@normal plain/normal_grad/box/compact/miss@normal "
        "plain/normal_grad/box/compact/r27@normal",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near"):
        "plain/normal_grad/box/whole/miss@feature plain/normal_grad/box/compact/miss@feature "
        "plain/normal_grad/box/compact/r27@feature",
    ("raymarch_rays_state: | raymarch_rays:state | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_bwd:state,g_depth,g_wsum | raymarch_rays_normals_bwd:state,d_planes,dec_out | raymarch_rays_bwd_rays: | "
     "raymarch_rays_normals_bwd_rays:state,d_origins"):
        "plain/normal_ray_grad/none/whole/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_normals_bwd:state | raymarch_rays_normals_bwd_rays:state"):
        "plain/normal_ray_grad/none/whole/r27@normal",
    ("raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near,g_depth,g_wsum | raymarch_rays_normals_bwd:state,t_near,d_planes,dec_out | "
     "raymarch_rays_bwd_rays:t_near | raymarch_rays_normals_bwd_rays:state,t_near,d_origins"):
        "plain/normal_ray_grad/explicit/whole/miss@all plain/normal_ray_grad/explicit/compact/miss@all "
        "plain/normal_ray_grad/explicit/compact/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_normals_bwd:state,t_near | raymarch_rays_normals_bwd_rays:state,t_near"):
        "plain/normal_ray_grad/explicit/whole/miss@normal plain/normal_ray_grad/explicit/compact/miss@normal "
        "plain/normal_ray_grad/explicit/compact/r27@normal",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near,g_depth,g_wsum | "
     "raymarch_rays_normals_bwd:state,t_near,d_planes,dec_out | raymarch_rays_bwd_rays:t_near | "
     "raymarch_rays_normals_bwd_rays:state,t_near,d_origins"):
        "plain/normal_ray_grad/box/whole/miss@all plain/normal_ray_grad/box/compact/miss@all "
        "plain/normal_ray_grad/box/compact/r27@all",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_normals_bwd:state,t_near | raymarch_rays_normals_bwd_rays:state,t_near"):
        "plain/normal_ray_grad/box/whole/miss@normal plain/normal_ray_grad/box/compact/miss@normal "
        "plain/normal_ray_grad/box/compact/r27@normal",
    "raymarch_rays:samples | depth_clamp_:":
        "samples/none/none/whole/r27@nograd",
    ("raymarch_rays_state: | raymarch_rays:state,samples | depth_clamp_: | raymarch_rays_bwd:state,g_depth,g_wsum,g_weights | "
     "raymarch_rays_bwd_rays:"):
        "samples/none/none/whole/r27@all",
    "raymarch_rays_state: | raymarch_rays:state,samples | depth_clamp_: | raymarch_rays_bwd:state | raymarch_rays_bwd_rays:":
        "samples/none/none/whole/r27@feature",
    "raymarch_rays:t_near,samples | depth_clamp_:":
        "samples/none/explicit/whole/miss@nograd samples/none/explicit/compact/miss@nograd "
        "samples/none/explicit/compact/r27@nograd",
    ("raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_bwd:state,t_near,g_depth,g_wsum,g_weights | raymarch_rays_bwd_rays:t_near"):
        "samples/none/explicit/whole/miss@all samples/none/explicit/compact/miss@all samples/none/explicit/compact/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | raymarch_rays_bwd:state,t_near | "
     "raymarch_rays_bwd_rays:t_near"):
        "samples/none/explicit/whole/miss@feature samples/none/explicit/compact/miss@feature "
        "samples/none/explicit/compact/r27@feature",
    "ray_limits_box: | raymarch_rays:t_near,samples | depth_clamp_:":
        "samples/none/box/whole/miss@nograd samples/none/box/compact/miss@nograd samples/none/box/compact/r27@nograd",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_bwd:state,t_near,g_depth,g_wsum,g_weights | raymarch_rays_bwd_rays:t_near"):
        "samples/none/box/whole/miss@all samples/none/box/compact/miss@all samples/none/box/compact/r27@all",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_bwd:state,t_near | raymarch_rays_bwd_rays:t_near"):
        "samples/none/box/whole/miss@feature samples/none/box/compact/miss@feature samples/none/box/compact/r27@feature",
    "raymarch_rays_state: | raymarch_rays:state,samples | raymarch_rays_normals:state | depth_clamp_:":
        "samples/normals/none/whole/r27@nograd samples/normal_grad/none/whole/r27@nograd "
        "samples/normal_ray_grad/none/whole/r27@nograd",
    ("raymarch_rays_state: | raymarch_rays:state,samples | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_bwd:state,g_depth,g_wsum,g_weights | raymarch_rays_bwd_rays:"):
        "samples/normals/none/whole/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,samples | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_bwd:state | raymarch_rays_bwd_rays:"):
        "samples/normals/none/whole/r27@feature samples/normal_ray_grad/none/whole/r27@feature",
    "raymarch_rays_state: | raymarch_rays:state,t_near,samples | raymarch_rays_normals:state,t_near | depth_clamp_:":
        "samples/normals/explicit/whole/miss@nograd samples/normals/explicit/compact/miss@nograd "
        "samples/normals/explicit/compact/r27@nograd samples/normal_grad/explicit/whole/miss@nograd "
        "samples/normal_grad/explicit/compact/miss@nograd samples/normal_grad/explicit/compact/r27@nograd "
        "samples/normal_ray_grad/explicit/whole/miss@nograd samples/normal_ray_grad/explicit/compact/miss@nograd "
        "samples/normal_ray_grad/explicit/compact/r27@nograd",
    ("raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near,g_depth,g_wsum,g_weights | raymarch_rays_bwd_rays:t_near"):
        "samples/normals/explicit/whole/miss@all samples/normals/explicit/compact/miss@all "
        "samples/normals/explicit/compact/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near | raymarch_rays_bwd_rays:t_near"):
        "samples/normals/explicit/whole/miss@feature samples/normals/explicit/compact/miss@feature "
        "samples/normals/explicit/compact/r27@feature samples/normal_ray_grad/explicit/whole/miss@feature "
        "samples/normal_ray_grad/explicit/compact/miss@feature samples/normal_ray_grad/explicit/compact/r27@feature",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | raymarch_rays_normals:state,t_near | "
     "depth_clamp_:"):
        "samples/normals/box/whole/miss@nograd samples/normals/box/compact/miss@nograd samples/normals/box/compact/r27@nograd "
        "samples/normal_grad/box/whole/miss@nograd samples/normal_grad/box/compact/miss@nograd "
        "samples/normal_grad/box/compact/r27@nograd samples/normal_ray_grad/box/whole/miss@nograd "
        "samples/normal_ray_grad/box/compact/miss@nograd samples/normal_ray_grad/box/compact/r27@nograd",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near,g_depth,g_wsum,g_weights | "
     "raymarch_rays_bwd_rays:t_near"):
        "samples/normals/box/whole/miss@all samples/normals/box/compact/miss@all samples/normals/box/compact/r27@all",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near | raymarch_rays_bwd_rays:t_near"):
        "samples/normals/box/whole/miss@feature samples/normals/box/compact/miss@feature "
        "samples/normals/box/compact/r27@feature samples/normal_ray_grad/box/whole/miss@feature "
        "samples/normal_ray_grad/box/compact/miss@feature samples/normal_ray_grad/box/compact/r27@feature",
    ("raymarch_rays_state: | raymarch_rays:state,samples | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_bwd:state,g_depth,g_wsum,g_weights | raymarch_rays_normals_bwd:state,d_planes,dec_out"):
        "samples/normal_grad/none/whole/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,samples | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_normals_bwd:state"):
        "samples/normal_grad/none/whole/r27@normal",
    ("raymarch_rays_state: | raymarch_rays:state,samples | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_bwd:state"):
        "samples/normal_grad/none/whole/r27@feature",
    ("raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near,g_depth,g_wsum,g_weights | raymarch_rays_normals_bwd:state,t_near,d_planes,dec_out"):
        "samples/normal_grad/explicit/whole/miss@all samples/normal_grad/explicit/compact/miss@all "
        "samples/normal_grad/explicit/compact/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_normals_bwd:state,t_near"):
        "samples/normal_grad/explicit/whole/miss@normal samples/normal_grad/explicit/compact/miss@normal "
        "samples/normal_grad/explicit/compact/r27@normal",
    ("raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near"):
        "samples/normal_grad/explicit/whole/miss@feature samples/normal_grad/explicit/compact/miss@feature "
        "samples/normal_grad/explicit/compact/r27@feature",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near,g_depth,g_wsum,g_weights | "
     "raymarch_rays_normals_bwd:state,t_near,d_planes,dec_out"):
        "samples/normal_grad/box/whole/miss@all samples/normal_grad/box/compact/miss@all "
        "samples/normal_grad/box/compact/r27@all",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_normals_bwd:state,t_near"):
        "samples/normal_grad/box/whole/miss@normal samples/normal_grad/box/compact/miss@normal "
        "samples/normal_grad/box/compact/r27@normal",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near"):
        "samples/normal_grad/box/whole/miss@feature samples/normal_grad/box/compact/miss@feature "
        "samples/normal_grad/box/compact/r27@feature",
    ("raymarch_rays_state: | raymarch_rays:state,samples | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_bwd:state,g_depth,g_wsum,g_weights | raymarch_rays_normals_bwd:state,d_planes,dec_out | "
     "raymarch_rays_bwd_rays: | raymarch_rays_normals_bwd_rays:state,d_origins"):
        "samples/normal_ray_grad/none/whole/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,samples | depth_clamp_: | raymarch_rays_normals:state | "
     "raymarch_rays_normals_bwd:state | raymarch_rays_normals_bwd_rays:state"):
        "samples/normal_ray_grad/none/whole/r27@normal",
    ("raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_bwd:state,t_near,g_depth,g_wsum,g_weights | raymarch_rays_normals_bwd:state,t_near,d_planes,dec_out | "
     "raymarch_rays_bwd_rays:t_near | raymarch_rays_normals_bwd_rays:state,t_near,d_origins"):
        "samples/normal_ray_grad/explicit/whole/miss@all samples/normal_ray_grad/explicit/compact/miss@all "
        "samples/normal_ray_grad/explicit/compact/r27@all",
    ("raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | raymarch_rays_normals:state,t_near | "
     "raymarch_rays_normals_bwd:state,t_near | raymarch_rays_normals_bwd_rays:state,t_near"):
        "samples/normal_ray_grad/explicit/whole/miss@normal samples/normal_ray_grad/explicit/compact/miss@normal "
        "samples/normal_ray_grad/explicit/compact/r27@normal",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_bwd:state,t_near,g_depth,g_wsum,g_weights | "
     "raymarch_rays_normals_bwd:state,t_near,d_planes,dec_out | raymarch_rays_bwd_rays:t_near | "
     "raymarch_rays_normals_bwd_rays:state,t_near,d_origins"):
        "samples/normal_ray_grad/box/whole/miss@all samples/normal_ray_grad/box/compact/miss@all "
        "samples/normal_ray_grad/box/compact/r27@all",
    ("ray_limits_box: | raymarch_rays_state: | raymarch_rays:state,t_near,samples | depth_clamp_: | "
     "raymarch_rays_normals:state,t_near | raymarch_rays_normals_bwd:state,t_near | raymarch_rays_normals_bwd_rays:state,t_near"):
        "samples/normal_ray_grad/box/whole/miss@normal samples/normal_ray_grad/box/compact/miss@normal "
        "samples/normal_ray_grad/box/compact/r27@normal",
}
EXPECTED = {cell: trace for trace, cs in PARENT_TRACES.items() for cell in cs.split()}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("samples", [False, True], ids=["plain", "samples"])
def test_matrix(dev, gen, samples, mode):
    from hfa_gp_amd import ops
    base = {}
    with Recorder(ops) as rec:
        for cell in cells():
            if cell[:2] != (samples, mode):
                continue
            _, _, limits, compact, rays = cell
            cid = cell_id(*cell)
            traces, plain, under = run_cell(gen, dev, rec, *cell)
            # 1. the launch trace
            for which, trace in traces.items():
                assert trace == EXPECTED[f"{cid}@{which}"], f"{cid}@{which}"
            # 2. forward bits: against the call without the keywords, under grad against no grad, compact against whole
            if (rays, limits) not in base:
                ws, o, d, us, ui, lim = inputs(dev, rays, limits, False)
                with torch.no_grad():
                    base[rays, limits] = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, **lim)
            ref = base[rays, limits]
            assert set(ref) == {"feature", "rgb", "depth", "mask"} | ({"valid"} if limits != "none" else set())
            want = set(ref) | ({"normal"} if mode != "none" else set()) | ({"sample_weights", "sample_depths"} if samples else set())
            assert set(plain) == want and set(under) == want, cid
            for k in ref:
                assert torch.equal(plain[k], ref[k]), f"{cid}: {k} against the plain call"
            for k in plain:
                assert torch.equal(plain[k], under[k].detach()), f"{cid}: {k} under grad"
                assert not plain[k].requires_grad, f"{cid}: {k} without grad"
            if not compact:
                base[rays, limits, "whole"] = plain
            else:
                whole = base.get((rays, limits, "whole"))
                if whole is None:        # (the all-valid list has no whole cell of its own under limits)
                    ws, o, d, us, ui, lim = inputs(dev, rays, limits, False)
                    with torch.no_grad():
                        whole = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, **lim, **MODES[mode], samples=samples)
                for k in whole:
                    assert torch.equal(plain[k], whole[k]), f"{cid}: {k} compact against whole"
            # 3. what requires grad
            for k in ("feature", "rgb", "depth", "mask"):
                assert under[k].requires_grad, f"{cid}: {k}"
            if mode != "none":
                assert under["normal"].requires_grad == (mode in ("normal_grad", "normal_ray_grad")), cid
            if samples:
                assert under["sample_weights"].requires_grad and not under["sample_depths"].requires_grad, cid
            if limits != "none":
                assert not under["valid"].requires_grad
                assert bool(under["valid"].all()) == (rays == "r27") and bool(under["valid"].any(1).all())


@pytest.mark.parametrize("rays,limits", [("r27", "none"), ("miss", "box")])
def test_above_the_cap_the_list_is_marched_once_in_chunks(dev, gen, monkeypatch, rays, limits):
    from hfa_gp_amd import generator, ops
    cfg = _cfg()
    ws, o, d, us, ui, lim = inputs(dev, rays, limits, True)
    whole = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normals=True, samples=True, **lim)
    per_ray = B * (cfg.depth_resolution + cfg.depth_resolution_importance) * 140
    monkeypatch.setattr(generator, "RAY_STATE_CAP_BYTES", 17 * per_ray)
    with Recorder(ops) as rec:
        parts = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normals=True, samples=True, **lim)
        forward = rec.take().split(" | ")
        loss_of(parts, "all").backward()
        backward = rec.take().split(" | ")
    assert set(parts) == set(whole)
    for k in whole:
        assert torch.equal(whole[k].detach(), parts[k].detach()), k
        assert whole[k].requires_grad == parts[k].requires_grad, k
    chunks = -(-R // 17)
    assert sum(c.startswith("raymarch_rays:") for c in forward) == chunks
    assert sum(c.startswith("raymarch_rays_normals:") for c in forward) == chunks
    assert all("state" in c for c in forward if c.startswith("raymarch_rays:"))
    # the backward has no state to read: the recomputing pass 1
    assert [c.split(":")[0] for c in backward] == ["raymarch_rays_bwd", "raymarch_rays_bwd_rays"] and "state" not in backward[0]
    assert bool(torch.isfinite(ws.grad).all()) and float(ws.grad.abs().max()) > 0 and float(o.grad.abs().max()) > 0
    gen.zero_grad(set_to_none=True)
    with pytest.raises(RuntimeError, match=rf"RAY_STATE_CAP_BYTES = {17 * per_ray}; 34 rays fit"):
        gen.render_rays(ws, o.detach(), d.detach(), u_strat=us, u_imp=ui, normal_grad=True, samples=True, **lim)
