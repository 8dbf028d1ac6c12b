"""Every keyword combination of TriPlaneGenerator.synthesis on the device: which ops it launches in which order and with which
optional arguments, and which outputs require grad in which order (against a table recorded on the commit before
hfa-gp_amd/synthesis_call.py existed), that a keyword leaves the entries it shares with the plain call bit-identical, and that a
call leaves nothing on the generator.  The same for the stand-alone `sample_mixed(differentiable=True)`.
Needs an MI355X:  python -m pytest tests -m gpu

The tiny64 generator of tests/test_gpu_normal_grad.py (10^2 rays, a 40^2 image, fp32 convs), frozen and with every non-mapping
parameter requiring grad, B = 2, `ws` requiring grad; the query is one point set [1, 37, 3] inside the box for both frames (37 is
not a multiple of the wave, and a batch of 1 takes the sum over the frames in the points' gradient).  No tolerance anywhere: the
comparisons are of launch traces and of bits."""
import dataclasses
import inspect
import itertools

import pytest
import torch

from tests.test_gpu_normal_grad import _cfg, _gen, B
from tests.util import SYNTHESIS_CALL_STATE, make_inputs

pytestmark = pytest.mark.gpu

M = 37
QUERIES = ("none", "coords", "coords_grad", "coords_qn")
MODES = {"none": {}, "normals": dict(normals=True), "normal_grad": dict(normal_grad=True),
         "normal_camera_grad": dict(normal_camera_grad=True)}
LOSSES = ("image", "all", "normal")
TRACED = ("raymarch", "raymarch_state", "raymarch_normals", "raymarch_bwd", "raymarch_bwd_camera", "raymarch_normals_bwd",
          "raymarch_normals_bwd_camera", "planes_query", "planes_query_bwd", "planes_query_normals", "planes_query_normals_bwd",
          "depth_clamp_", "depth_range", "resize_aa", "resize_aa_bwd", "pointwise_bwd")
TRACKED = ("state", "g_depth", "g_wsum", "rec_out", "ray_grad", "reduce", "d_planes", "dec_out", "coords_grad", "g_sigma", "g_rgb",
           "g_grad", "g_normal", "g_nchw3", "g_nchw3_a", "g_nchw3_b")
# (geometry, query, mode, c requires grad, return_planes, rays per side): the handful of cells that also run with return_planes
# and / or at another neural_rendering_resolution than the configured 10
EXTRA = ((False, "none", "none", False, True, 10), (False, "none", "none", False, False, 7),
         (True, "none", "normals", False, True, 10), (True, "coords", "normal_camera_grad", True, True, 7),
         (False, "coords_qn", "normals", True, True, 7), (True, "coords_grad", "normal_grad", False, False, 7))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gens(dev):
    """{tuned: generator}.  (The frozen one is the instance the other test files share: this file leaves it as it found it.)"""
    return {False: _gen(dev), True: _gen(dev, tuned=True)}


class Recorder:
    """Wraps the ops of TRACED; `trace` is the list of "name:arg,arg" of the calls so far, the args being those of TRACKED that the
    call got as something other than None / False."""
    def __init__(self, ops):
        self.ops, self.trace, self.saved = ops, [], {}

    def __enter__(self):
        for name in TRACED:
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

    def take(self, keep=lambda call: True):
        """The calls since the last take, " | "-joined; a run of n equal calls is written once, "name:args xn"."""
        runs, self.trace = [(t, len(list(g))) for t, g in itertools.groupby(filter(keep, self.trace))], []
        return " | ".join(t if n == 1 else f"{t} x{n}" for t, n in runs)


def refused(query, mode, c_grad):
    """The combinations `synthesis` refuses under grad (tests/test_gpu_query_normals.py, test_gpu_normal_grad.py have them)."""
    return (query == "coords_qn" and mode in ("normal_grad", "normal_camera_grad")) or (mode == "normal_grad" and c_grad)


def cells():
    """(geometry, query, mode, c requires grad, return_planes, rays per side) of the matrix."""
    for geometry, query, mode, c_grad in itertools.product((False, True), QUERIES, MODES, (False, True)):
        if not refused(query, mode, c_grad):
            yield geometry, query, mode, c_grad, False, 10
    yield from EXTRA


def cell_id(tuned, geometry, query, mode, c_grad, planes, res):
    return (f"{'tuned' if tuned else 'frozen'}/{'geometry' if geometry else 'plain'}/{query}/{mode}/{'c_grad' if c_grad else 'c'}"
            f"{'/planes' if planes else ''}{'' if res == 10 else f'/r{res}'}")


def inputs(dev, res=10, query="none", c_grad=False):
    """ws (requires grad), c, the uniforms for res^2 rays -> (positional arguments, keywords) of a synthesis call."""
    ws, c, us, ui = (t.to(dev) for t in make_inputs(dataclasses.replace(_cfg(), neural_rendering_resolution=res), B))
    ws.requires_grad_(True)
    c.requires_grad_(c_grad)
    kw = dict(noise_mode="const", u_strat=us, u_imp=ui, neural_rendering_resolution=res)
    if query != "none":
        q = (torch.rand(1, M, 3, generator=torch.Generator().manual_seed(37)) - 0.5) * (0.8 * _cfg().box_warp)
        kw.update(query=q.to(dev).requires_grad_(query == "coords_grad"), query_normals=query == "coords_qn")
    return (ws, c), kw


def loss_of(out, which):
    if which == "all":
        return sum(v.sum() for v in out.values() if v.requires_grad)
    return out["image" if which == "image" else "image_normal"].sum()


def run_cell(gen, dev, rec, geometry, query, mode, c_grad, planes, res):
    """One cell without grad and under grad with each loss -> ({"nograd" / loss name: trace, "requires_grad": the keys of the dict
    under grad in their order, each with whether it requires grad}, the no-grad dict, the under-grad dict of the "all" loss)."""
    kw = dict(MODES[mode], geometry=geometry, return_planes=planes)
    traces = {}
    args, call = inputs(dev, res, query, c_grad)
    rec.take()
    with torch.no_grad():
        plain = gen.synthesis(*args, **call, **kw)
    traces["nograd"] = rec.take()
    under = None
    for which in LOSSES:
        if which == "normal" and mode not in ("normal_grad", "normal_camera_grad"):
            continue
        args, call = inputs(dev, res, query, c_grad)
        rec.take()
        out = gen.synthesis(*args, **call, **kw)
        loss_of(out, which).backward()
        traces[which] = rec.take()
        assert args[0].grad is not None and bool(torch.isfinite(args[0].grad).all())
        if which == "all":
            under = out
            traces["requires_grad"] = " ".join(f"{k}:{int(v.requires_grad)}" for k, v in out.items())
    gen.zero_grad(set_to_none=True)
    return traces, plain, under


# The launch traces and the outputs' requires_grad of the commit before this file, 64cdd15 ("Ray lists: one module, one autograd
# function, one forward path"), recorded there with the Recorder above on the cells above: trace -> the cells (cell id @ "nograd",
# the loss or "requires_grad") that gave it.
PARENT_TRACES = {
    'raymarch: | depth_clamp_:':
        ('frozen/plain/none/none/c@nograd frozen/plain/none/none/c_grad@nograd frozen/geometry/none/none/c@nograd '
         'frozen/geometry/none/none/c_grad@nograd frozen/plain/none/none/c/planes@nograd tuned/plain/none/none/c@nograd '
         'tuned/plain/none/none/c_grad@nograd tuned/geometry/none/none/c@nograd tuned/geometry/none/none/c_grad@nograd '
         'tuned/plain/none/none/c/planes@nograd'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | '
     'raymarch_bwd:state | pointwise_bwd: x10'):
        ('frozen/plain/none/none/c@image frozen/plain/none/none/c@all frozen/plain/none/none/c/planes@image '
         'frozen/plain/none/none/c/planes@all tuned/plain/none/none/c@image tuned/plain/none/none/c@all '
         'tuned/plain/none/none/c/planes@image tuned/plain/none/none/c/planes@all'),
    'image:1 image_raw:1 image_depth:0':
        ('frozen/plain/none/none/c@requires_grad frozen/plain/none/none/c_grad@requires_grad '
         'frozen/plain/none/none/c/r7@requires_grad tuned/plain/none/none/c@requires_grad '
         'tuned/plain/none/none/c_grad@requires_grad tuned/plain/none/none/c/r7@requires_grad'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | '
     'raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        ('frozen/plain/none/none/c_grad@image frozen/plain/none/none/c_grad@all tuned/plain/none/none/c_grad@image '
         'tuned/plain/none/none/c_grad@all'),
    'raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_:':
        ('frozen/plain/none/normals/c@nograd frozen/plain/none/normals/c_grad@nograd frozen/plain/none/normal_grad/c@nograd '
         'frozen/plain/none/normal_camera_grad/c@nograd frozen/plain/none/normal_camera_grad/c_grad@nograd '
         'frozen/geometry/none/normals/c@nograd frozen/geometry/none/normals/c_grad@nograd '
         'frozen/geometry/none/normal_grad/c@nograd frozen/geometry/none/normal_camera_grad/c@nograd '
         'frozen/geometry/none/normal_camera_grad/c_grad@nograd frozen/geometry/none/normals/c/planes@nograd '
         'tuned/plain/none/normals/c@nograd tuned/plain/none/normals/c_grad@nograd tuned/plain/none/normal_grad/c@nograd '
         'tuned/plain/none/normal_camera_grad/c@nograd tuned/plain/none/normal_camera_grad/c_grad@nograd '
         'tuned/geometry/none/normals/c@nograd tuned/geometry/none/normals/c_grad@nograd '
         'tuned/geometry/none/normal_grad/c@nograd tuned/geometry/none/normal_camera_grad/c@nograd '
         'tuned/geometry/none/normal_camera_grad/c_grad@nograd tuned/geometry/none/normals/c/planes@nograd'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | pointwise_bwd: x10'):
        ('frozen/plain/none/normals/c@image frozen/plain/none/normals/c@all tuned/plain/none/normals/c@image '
         'tuned/plain/none/normals/c@all'),
    'image:1 image_raw:1 image_depth:0 image_normal:0':
        ('frozen/plain/none/normals/c@requires_grad frozen/plain/none/normals/c_grad@requires_grad '
         'tuned/plain/none/normals/c@requires_grad tuned/plain/none/normals/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        ('frozen/plain/none/normals/c_grad@image frozen/plain/none/normals/c_grad@all tuned/plain/none/normals/c_grad@image '
         'tuned/plain/none/normals/c_grad@all'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a '
     '| raymarch_bwd:state | pointwise_bwd: x10'):
        ('frozen/plain/none/normal_grad/c@image frozen/plain/none/normal_camera_grad/c@image '
         'tuned/plain/none/normal_grad/c@image tuned/plain/none/normal_camera_grad/c@image'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: '
     'x10'):
        'frozen/plain/none/normal_grad/c@all frozen/plain/none/normal_camera_grad/c@all',
    'image:1 image_raw:1 image_depth:0 image_normal:1':
        ('frozen/plain/none/normal_grad/c@requires_grad frozen/plain/none/normal_camera_grad/c@requires_grad '
         'frozen/plain/none/normal_camera_grad/c_grad@requires_grad tuned/plain/none/normal_grad/c@requires_grad '
         'tuned/plain/none/normal_camera_grad/c@requires_grad tuned/plain/none/normal_camera_grad/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a '
     '| raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/plain/none/normal_grad/c@normal frozen/plain/none/normal_camera_grad/c@normal',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a '
     '| raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        'frozen/plain/none/normal_camera_grad/c_grad@image tuned/plain/none/normal_camera_grad/c_grad@image',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/plain/none/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a '
     '| raymarch_bwd:state,rec_out | raymarch_bwd_camera: | raymarch_normals_bwd_camera:state,ray_grad,g_normal | '
     'raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/plain/none/normal_camera_grad/c_grad@normal',
    'raymarch: | depth_clamp_: | planes_query:':
        ('frozen/plain/coords/none/c@nograd frozen/plain/coords/none/c_grad@nograd frozen/plain/coords_grad/none/c@nograd '
         'frozen/plain/coords_grad/none/c_grad@nograd frozen/geometry/coords/none/c@nograd '
         'frozen/geometry/coords/none/c_grad@nograd frozen/geometry/coords_grad/none/c@nograd '
         'frozen/geometry/coords_grad/none/c_grad@nograd tuned/plain/coords/none/c@nograd '
         'tuned/plain/coords/none/c_grad@nograd tuned/plain/coords_grad/none/c@nograd '
         'tuned/plain/coords_grad/none/c_grad@nograd tuned/geometry/coords/none/c@nograd '
         'tuned/geometry/coords/none/c_grad@nograd tuned/geometry/coords_grad/none/c@nograd '
         'tuned/geometry/coords_grad/none/c_grad@nograd'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | '
     'raymarch_bwd:state | pointwise_bwd: x10'):
        ('frozen/plain/coords/none/c@image frozen/plain/coords_grad/none/c@image tuned/plain/coords/none/c@image '
         'tuned/plain/coords_grad/none/c@image'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b'
     ' | raymarch_bwd:state | planes_query_bwd:d_planes,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/plain/coords/none/c@all',
    'image:1 image_raw:1 image_depth:0 query_sigma:1 query_rgb:1':
        ('frozen/plain/coords/none/c@requires_grad frozen/plain/coords/none/c_grad@requires_grad '
         'frozen/plain/coords_grad/none/c@requires_grad frozen/plain/coords_grad/none/c_grad@requires_grad '
         'tuned/plain/coords/none/c@requires_grad tuned/plain/coords/none/c_grad@requires_grad '
         'tuned/plain/coords_grad/none/c@requires_grad tuned/plain/coords_grad/none/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | '
     'raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        ('frozen/plain/coords/none/c_grad@image frozen/plain/coords_grad/none/c_grad@image '
         'tuned/plain/coords/none/c_grad@image tuned/plain/coords_grad/none/c_grad@image'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b'
     ' | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,g_sigma,g_rgb | pointwise_bwd: '
     'x10'):
        'frozen/plain/coords/none/c_grad@all',
    'raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query:':
        ('frozen/plain/coords/normals/c@nograd frozen/plain/coords/normals/c_grad@nograd '
         'frozen/plain/coords/normal_grad/c@nograd frozen/plain/coords/normal_camera_grad/c@nograd '
         'frozen/plain/coords/normal_camera_grad/c_grad@nograd frozen/plain/coords_grad/normals/c@nograd '
         'frozen/plain/coords_grad/normals/c_grad@nograd frozen/plain/coords_grad/normal_grad/c@nograd '
         'frozen/plain/coords_grad/normal_camera_grad/c@nograd frozen/plain/coords_grad/normal_camera_grad/c_grad@nograd '
         'frozen/geometry/coords/normals/c@nograd frozen/geometry/coords/normals/c_grad@nograd '
         'frozen/geometry/coords/normal_grad/c@nograd frozen/geometry/coords/normal_camera_grad/c@nograd '
         'frozen/geometry/coords/normal_camera_grad/c_grad@nograd frozen/geometry/coords_grad/normals/c@nograd '
         'frozen/geometry/coords_grad/normals/c_grad@nograd frozen/geometry/coords_grad/normal_grad/c@nograd '
         'frozen/geometry/coords_grad/normal_camera_grad/c@nograd frozen/geometry/coords_grad/normal_camera_grad/c_grad@nograd'
         ' tuned/plain/coords/normals/c@nograd tuned/plain/coords/normals/c_grad@nograd '
         'tuned/plain/coords/normal_grad/c@nograd tuned/plain/coords/normal_camera_grad/c@nograd '
         'tuned/plain/coords/normal_camera_grad/c_grad@nograd tuned/plain/coords_grad/normals/c@nograd '
         'tuned/plain/coords_grad/normals/c_grad@nograd tuned/plain/coords_grad/normal_grad/c@nograd '
         'tuned/plain/coords_grad/normal_camera_grad/c@nograd tuned/plain/coords_grad/normal_camera_grad/c_grad@nograd '
         'tuned/geometry/coords/normals/c@nograd tuned/geometry/coords/normals/c_grad@nograd '
         'tuned/geometry/coords/normal_grad/c@nograd tuned/geometry/coords/normal_camera_grad/c@nograd '
         'tuned/geometry/coords/normal_camera_grad/c_grad@nograd tuned/geometry/coords_grad/normals/c@nograd '
         'tuned/geometry/coords_grad/normals/c_grad@nograd tuned/geometry/coords_grad/normal_grad/c@nograd '
         'tuned/geometry/coords_grad/normal_camera_grad/c@nograd tuned/geometry/coords_grad/normal_camera_grad/c_grad@nograd'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state | pointwise_bwd: x10'):
        ('frozen/plain/coords/normals/c@image frozen/plain/coords/normal_grad/c@image '
         'frozen/plain/coords/normal_camera_grad/c@image frozen/plain/coords_grad/normals/c@image '
         'frozen/plain/coords_grad/normal_grad/c@image frozen/plain/coords_grad/normal_camera_grad/c@image '
         'tuned/plain/coords/normals/c@image tuned/plain/coords/normal_grad/c@image '
         'tuned/plain/coords/normal_camera_grad/c@image tuned/plain/coords_grad/normals/c@image '
         'tuned/plain/coords_grad/normal_grad/c@image tuned/plain/coords_grad/normal_camera_grad/c@image'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/plain/coords/normals/c@all',
    'image:1 image_raw:1 image_depth:0 query_sigma:1 query_rgb:1 image_normal:0':
        ('frozen/plain/coords/normals/c@requires_grad frozen/plain/coords/normals/c_grad@requires_grad '
         'frozen/plain/coords_grad/normals/c@requires_grad frozen/plain/coords_grad/normals/c_grad@requires_grad '
         'tuned/plain/coords/normals/c@requires_grad tuned/plain/coords/normals/c_grad@requires_grad '
         'tuned/plain/coords_grad/normals/c@requires_grad tuned/plain/coords_grad/normals/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        ('frozen/plain/coords/normals/c_grad@image frozen/plain/coords/normal_camera_grad/c_grad@image '
         'frozen/plain/coords_grad/normals/c_grad@image frozen/plain/coords_grad/normal_camera_grad/c_grad@image '
         'tuned/plain/coords/normals/c_grad@image tuned/plain/coords/normal_camera_grad/c_grad@image '
         'tuned/plain/coords_grad/normals/c_grad@image tuned/plain/coords_grad/normal_camera_grad/c_grad@image'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/plain/coords/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/plain/coords/normal_grad/c@all frozen/plain/coords/normal_camera_grad/c@all',
    'image:1 image_raw:1 image_depth:0 query_sigma:1 query_rgb:1 image_normal:1':
        ('frozen/plain/coords/normal_grad/c@requires_grad frozen/plain/coords/normal_camera_grad/c@requires_grad '
         'frozen/plain/coords/normal_camera_grad/c_grad@requires_grad frozen/plain/coords_grad/normal_grad/c@requires_grad '
         'frozen/plain/coords_grad/normal_camera_grad/c@requires_grad '
         'frozen/plain/coords_grad/normal_camera_grad/c_grad@requires_grad tuned/plain/coords/normal_grad/c@requires_grad '
         'tuned/plain/coords/normal_camera_grad/c@requires_grad tuned/plain/coords/normal_camera_grad/c_grad@requires_grad '
         'tuned/plain/coords_grad/normal_grad/c@requires_grad tuned/plain/coords_grad/normal_camera_grad/c@requires_grad '
         'tuned/plain/coords_grad/normal_camera_grad/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        ('frozen/plain/coords/normal_grad/c@normal frozen/plain/coords/normal_camera_grad/c@normal '
         'frozen/plain/coords_grad/normal_grad/c@normal frozen/plain/coords_grad/normal_camera_grad/c@normal'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | planes_query_bwd:d_planes,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/plain/coords/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/plain/coords/normal_camera_grad/c_grad@normal frozen/plain/coords_grad/normal_camera_grad/c_grad@normal',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b'
     ' | raymarch_bwd:state | planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/plain/coords_grad/none/c@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b'
     ' | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | '
     'pointwise_bwd: x10'):
        'frozen/plain/coords_grad/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | '
     'pointwise_bwd: x10'):
        'frozen/plain/coords_grad/normals/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/plain/coords_grad/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/plain/coords_grad/normal_grad/c@all frozen/plain/coords_grad/normal_camera_grad/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/plain/coords_grad/normal_camera_grad/c_grad@all',
    'raymarch: | depth_clamp_: | planes_query_normals:':
        ('frozen/plain/coords_qn/none/c@nograd frozen/plain/coords_qn/none/c_grad@nograd '
         'frozen/geometry/coords_qn/none/c@nograd frozen/geometry/coords_qn/none/c_grad@nograd '
         'tuned/plain/coords_qn/none/c@nograd tuned/plain/coords_qn/none/c_grad@nograd tuned/geometry/coords_qn/none/c@nograd '
         'tuned/geometry/coords_qn/none/c_grad@nograd'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a |'
     ' raymarch_bwd:state | pointwise_bwd: x10'):
        'frozen/plain/coords_qn/none/c@image tuned/plain/coords_qn/none/c@image',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,g_sigma,g_rgb | '
     'planes_query_normals_bwd:d_planes,g_grad,g_normal | pointwise_bwd: x10'):
        'frozen/plain/coords_qn/none/c@all',
    'image:1 image_raw:1 image_depth:0 query_sigma:1 query_rgb:1 query_sigma_grad:1 query_normal:1':
        ('frozen/plain/coords_qn/none/c@requires_grad frozen/plain/coords_qn/none/c_grad@requires_grad '
         'tuned/plain/coords_qn/none/c@requires_grad tuned/plain/coords_qn/none/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a |'
     ' raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        'frozen/plain/coords_qn/none/c_grad@image tuned/plain/coords_qn/none/c_grad@image',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,g_grad,g_normal | pointwise_bwd: x10'):
        'frozen/plain/coords_qn/none/c_grad@all',
    'raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query_normals:':
        ('frozen/plain/coords_qn/normals/c@nograd frozen/plain/coords_qn/normals/c_grad@nograd '
         'frozen/geometry/coords_qn/normals/c@nograd frozen/geometry/coords_qn/normals/c_grad@nograd '
         'tuned/plain/coords_qn/normals/c@nograd tuned/plain/coords_qn/normals/c_grad@nograd '
         'tuned/geometry/coords_qn/normals/c@nograd tuned/geometry/coords_qn/normals/c_grad@nograd'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state | pointwise_bwd: x10'):
        'frozen/plain/coords_qn/normals/c@image tuned/plain/coords_qn/normals/c@image',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,g_sigma,g_rgb | '
     'planes_query_normals_bwd:d_planes,g_grad,g_normal | pointwise_bwd: x10'):
        'frozen/plain/coords_qn/normals/c@all',
    'image:1 image_raw:1 image_depth:0 query_sigma:1 query_rgb:1 query_sigma_grad:1 query_normal:1 image_normal:0':
        ('frozen/plain/coords_qn/normals/c@requires_grad frozen/plain/coords_qn/normals/c_grad@requires_grad '
         'tuned/plain/coords_qn/normals/c@requires_grad tuned/plain/coords_qn/normals/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        'frozen/plain/coords_qn/normals/c_grad@image tuned/plain/coords_qn/normals/c_grad@image',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,g_grad,g_normal | pointwise_bwd: x10'):
        'frozen/plain/coords_qn/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | '
     'raymarch_bwd:state | pointwise_bwd: x10'):
        'frozen/geometry/none/none/c@image tuned/geometry/none/none/c@image',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b '
     '| raymarch_bwd:state,g_depth,g_wsum | pointwise_bwd: x10'):
        'frozen/geometry/none/none/c@all tuned/geometry/none/none/c@all',
    'image:1 image_raw:1 image_depth:1 image_mask:1':
        ('frozen/geometry/none/none/c@requires_grad frozen/geometry/none/none/c_grad@requires_grad '
         'tuned/geometry/none/none/c@requires_grad tuned/geometry/none/none/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | '
     'raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        'frozen/geometry/none/none/c_grad@image tuned/geometry/none/none/c_grad@image',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b '
     '| raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        'frozen/geometry/none/none/c_grad@all tuned/geometry/none/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state | pointwise_bwd: x10'):
        ('frozen/geometry/none/normals/c@image frozen/geometry/none/normal_grad/c@image '
         'frozen/geometry/none/normal_camera_grad/c@image frozen/geometry/none/normals/c/planes@image '
         'tuned/geometry/none/normals/c@image tuned/geometry/none/normal_grad/c@image '
         'tuned/geometry/none/normal_camera_grad/c@image tuned/geometry/none/normals/c/planes@image'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | pointwise_bwd: x10'):
        ('frozen/geometry/none/normals/c@all frozen/geometry/none/normals/c/planes@all tuned/geometry/none/normals/c@all '
         'tuned/geometry/none/normals/c/planes@all'),
    'image:1 image_raw:1 image_depth:1 image_mask:1 image_normal:0':
        ('frozen/geometry/none/normals/c@requires_grad frozen/geometry/none/normals/c_grad@requires_grad '
         'tuned/geometry/none/normals/c@requires_grad tuned/geometry/none/normals/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        ('frozen/geometry/none/normals/c_grad@image frozen/geometry/none/normal_camera_grad/c_grad@image '
         'tuned/geometry/none/normals/c_grad@image tuned/geometry/none/normal_camera_grad/c_grad@image'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:reduce | '
     'pointwise_bwd: x10'):
        'frozen/geometry/none/normals/c_grad@all tuned/geometry/none/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | raymarch_normals_bwd:state,d_planes,g_normal | '
     'pointwise_bwd: x10'):
        'frozen/geometry/none/normal_grad/c@all frozen/geometry/none/normal_camera_grad/c@all',
    'image:1 image_raw:1 image_depth:1 image_mask:1 image_normal:1':
        ('frozen/geometry/none/normal_grad/c@requires_grad frozen/geometry/none/normal_camera_grad/c@requires_grad '
         'frozen/geometry/none/normal_camera_grad/c_grad@requires_grad tuned/geometry/none/normal_grad/c@requires_grad '
         'tuned/geometry/none/normal_camera_grad/c@requires_grad tuned/geometry/none/normal_camera_grad/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/none/normal_grad/c@normal frozen/geometry/none/normal_camera_grad/c@normal',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/none/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/none/normal_camera_grad/c_grad@normal',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state | pointwise_bwd: x10'):
        ('frozen/geometry/coords/none/c@image frozen/geometry/coords_grad/none/c@image tuned/geometry/coords/none/c@image '
         'tuned/geometry/coords_grad/none/c@image'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | planes_query_bwd:d_planes,g_sigma,g_rgb | '
     'pointwise_bwd: x10'):
        'frozen/geometry/coords/none/c@all',
    'image:1 image_raw:1 image_depth:1 image_mask:1 query_sigma:1 query_rgb:1':
        ('frozen/geometry/coords/none/c@requires_grad frozen/geometry/coords/none/c_grad@requires_grad '
         'frozen/geometry/coords_grad/none/c@requires_grad frozen/geometry/coords_grad/none/c_grad@requires_grad '
         'tuned/geometry/coords/none/c@requires_grad tuned/geometry/coords/none/c_grad@requires_grad '
         'tuned/geometry/coords_grad/none/c@requires_grad tuned/geometry/coords_grad/none/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        ('frozen/geometry/coords/none/c_grad@image frozen/geometry/coords_grad/none/c_grad@image '
         'tuned/geometry/coords/none/c_grad@image tuned/geometry/coords_grad/none/c_grad@image'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/geometry/coords/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | raymarch_bwd:state | pointwise_bwd: x10'):
        ('frozen/geometry/coords/normals/c@image frozen/geometry/coords/normal_grad/c@image '
         'frozen/geometry/coords/normal_camera_grad/c@image frozen/geometry/coords_grad/normals/c@image '
         'frozen/geometry/coords_grad/normal_grad/c@image frozen/geometry/coords_grad/normal_camera_grad/c@image '
         'tuned/geometry/coords/normals/c@image tuned/geometry/coords/normal_grad/c@image '
         'tuned/geometry/coords/normal_camera_grad/c@image tuned/geometry/coords_grad/normals/c@image '
         'tuned/geometry/coords_grad/normal_grad/c@image tuned/geometry/coords_grad/normal_camera_grad/c@image'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/geometry/coords/normals/c@all',
    'image:1 image_raw:1 image_depth:1 image_mask:1 query_sigma:1 query_rgb:1 image_normal:0':
        ('frozen/geometry/coords/normals/c@requires_grad frozen/geometry/coords/normals/c_grad@requires_grad '
         'frozen/geometry/coords_grad/normals/c@requires_grad frozen/geometry/coords_grad/normals/c_grad@requires_grad '
         'tuned/geometry/coords/normals/c@requires_grad tuned/geometry/coords/normals/c_grad@requires_grad '
         'tuned/geometry/coords_grad/normals/c@requires_grad tuned/geometry/coords_grad/normals/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: '
     'x10'):
        ('frozen/geometry/coords/normals/c_grad@image frozen/geometry/coords/normal_camera_grad/c_grad@image '
         'frozen/geometry/coords_grad/normals/c_grad@image frozen/geometry/coords_grad/normal_camera_grad/c_grad@image '
         'tuned/geometry/coords/normals/c_grad@image tuned/geometry/coords/normal_camera_grad/c_grad@image '
         'tuned/geometry/coords_grad/normals/c_grad@image tuned/geometry/coords_grad/normal_camera_grad/c_grad@image'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | '
     'raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/geometry/coords/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,g_sigma,g_rgb | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords/normal_grad/c@all frozen/geometry/coords/normal_camera_grad/c@all',
    'image:1 image_raw:1 image_depth:1 image_mask:1 query_sigma:1 query_rgb:1 image_normal:1':
        ('frozen/geometry/coords/normal_grad/c@requires_grad frozen/geometry/coords/normal_camera_grad/c@requires_grad '
         'frozen/geometry/coords/normal_camera_grad/c_grad@requires_grad '
         'frozen/geometry/coords_grad/normal_grad/c@requires_grad '
         'frozen/geometry/coords_grad/normal_camera_grad/c@requires_grad '
         'frozen/geometry/coords_grad/normal_camera_grad/c_grad@requires_grad '
         'frozen/geometry/coords_grad/normal_grad/c/r7@requires_grad tuned/geometry/coords/normal_grad/c@requires_grad '
         'tuned/geometry/coords/normal_camera_grad/c@requires_grad '
         'tuned/geometry/coords/normal_camera_grad/c_grad@requires_grad tuned/geometry/coords_grad/normal_grad/c@requires_grad'
         ' tuned/geometry/coords_grad/normal_camera_grad/c@requires_grad '
         'tuned/geometry/coords_grad/normal_camera_grad/c_grad@requires_grad '
         'tuned/geometry/coords_grad/normal_grad/c/r7@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,g_normal | '
     'pointwise_bwd: x10'):
        ('frozen/geometry/coords/normal_grad/c@normal frozen/geometry/coords/normal_camera_grad/c@normal '
         'frozen/geometry/coords_grad/normal_grad/c@normal frozen/geometry/coords_grad/normal_camera_grad/c@normal'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:'
     ' | raymarch_normals_bwd_camera:state,ray_grad,g_normal | planes_query_bwd:d_planes,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords/normal_camera_grad/c_grad@normal frozen/geometry/coords_grad/normal_camera_grad/c_grad@normal',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/geometry/coords_grad/none/c@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/geometry/coords_grad/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/geometry/coords_grad/normals/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | '
     'raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'frozen/geometry/coords_grad/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords_grad/normal_grad/c@all frozen/geometry/coords_grad/normal_camera_grad/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:'
     ' | raymarch_normals_bwd_camera:state,ray_grad,g_normal | planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords_grad/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state | pointwise_bwd: x10'):
        'frozen/geometry/coords_qn/none/c@image tuned/geometry/coords_qn/none/c@image',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | planes_query_bwd:d_planes,g_sigma,g_rgb | '
     'planes_query_normals_bwd:d_planes,g_grad,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords_qn/none/c@all',
    'image:1 image_raw:1 image_depth:1 image_mask:1 query_sigma:1 query_rgb:1 query_sigma_grad:1 query_normal:1':
        ('frozen/geometry/coords_qn/none/c@requires_grad frozen/geometry/coords_qn/none/c_grad@requires_grad '
         'tuned/geometry/coords_qn/none/c@requires_grad tuned/geometry/coords_qn/none/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: x10'):
        'frozen/geometry/coords_qn/none/c_grad@image tuned/geometry/coords_qn/none/c_grad@image',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,g_grad,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords_qn/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query_normals: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | raymarch_bwd:state | pointwise_bwd: x10'):
        'frozen/geometry/coords_qn/normals/c@image tuned/geometry/coords_qn/normals/c@image',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query_normals: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,g_grad,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords_qn/normals/c@all',
    ('image:1 image_raw:1 image_depth:1 image_mask:1 query_sigma:1 query_rgb:1 query_sigma_grad:1 query_normal:1 '
     'image_normal:0'):
        ('frozen/geometry/coords_qn/normals/c@requires_grad frozen/geometry/coords_qn/normals/c_grad@requires_grad '
         'tuned/geometry/coords_qn/normals/c@requires_grad tuned/geometry/coords_qn/normals/c_grad@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query_normals: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | pointwise_bwd: '
     'x10'):
        'frozen/geometry/coords_qn/normals/c_grad@image tuned/geometry/coords_qn/normals/c_grad@image',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query_normals: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | '
     'raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,g_grad,g_normal'
     ' | pointwise_bwd: x10'):
        'frozen/geometry/coords_qn/normals/c_grad@all',
    'image:1 image_raw:1 image_depth:0 planes:0 feature_image:0':
        'frozen/plain/none/none/c/planes@requires_grad tuned/plain/none/none/c/planes@requires_grad',
    'raymarch: | depth_clamp_: | resize_aa:':
        'frozen/plain/none/none/c/r7@nograd tuned/plain/none/none/c/r7@nograd',
    ('raymarch_state: | raymarch:state | depth_clamp_: | resize_aa: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | '
     'resize_aa_bwd:g_nchw3 | raymarch_bwd:state | pointwise_bwd: x10'):
        ('frozen/plain/none/none/c/r7@image frozen/plain/none/none/c/r7@all tuned/plain/none/none/c/r7@image '
         'tuned/plain/none/none/c/r7@all'),
    'image:1 image_raw:1 image_depth:1 image_mask:1 planes:0 feature_image:0 image_normal:0':
        'frozen/geometry/none/normals/c/planes@requires_grad tuned/geometry/none/normals/c/planes@requires_grad',
    'raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | planes_query:':
        ('frozen/geometry/coords/normal_camera_grad/c_grad/planes/r7@nograd '
         'frozen/geometry/coords_grad/normal_grad/c/r7@nograd tuned/geometry/coords/normal_camera_grad/c_grad/planes/r7@nograd'
         ' tuned/geometry/coords_grad/normal_grad/c/r7@nograd'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd: | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce |'
     ' pointwise_bwd: x10'):
        ('frozen/geometry/coords/normal_camera_grad/c_grad/planes/r7@image '
         'tuned/geometry/coords/normal_camera_grad/c_grad/planes/r7@image'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd:g_nchw3 | raymarch_bwd:state,g_depth,g_wsum,rec_out | '
     'raymarch_bwd_camera: | raymarch_normals_bwd_camera:state,ray_grad,g_normal | planes_query_bwd:d_planes,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords/normal_camera_grad/c_grad/planes/r7@all',
    'image:1 image_raw:1 image_depth:1 image_mask:1 query_sigma:1 query_rgb:1 image_normal:1 planes:0 feature_image:0':
        ('frozen/geometry/coords/normal_camera_grad/c_grad/planes/r7@requires_grad '
         'tuned/geometry/coords/normal_camera_grad/c_grad/planes/r7@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd: | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords/normal_camera_grad/c_grad/planes/r7@normal',
    'raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | planes_query_normals:':
        'frozen/plain/coords_qn/normals/c_grad/planes/r7@nograd tuned/plain/coords_qn/normals/c_grad/planes/r7@nograd',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | planes_query_normals: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd: | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce |'
     ' pointwise_bwd: x10'):
        'frozen/plain/coords_qn/normals/c_grad/planes/r7@image tuned/plain/coords_qn/normals/c_grad/planes/r7@image',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | planes_query_normals: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd:g_nchw3 | raymarch_bwd:state,rec_out | '
     'raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,g_grad,g_normal'
     ' | pointwise_bwd: x10'):
        'frozen/plain/coords_qn/normals/c_grad/planes/r7@all',
    ('image:1 image_raw:1 image_depth:0 query_sigma:1 query_rgb:1 query_sigma_grad:1 query_normal:1 planes:0 feature_image:0 '
     'image_normal:0'):
        ('frozen/plain/coords_qn/normals/c_grad/planes/r7@requires_grad '
         'tuned/plain/coords_qn/normals/c_grad/planes/r7@requires_grad'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd: | raymarch_bwd:state | pointwise_bwd: x10'):
        'frozen/geometry/coords_grad/normal_grad/c/r7@image tuned/geometry/coords_grad/normal_grad/c/r7@image',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd:g_nchw3 | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,coords_grad,g_sigma,g_rgb | raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords_grad/normal_grad/c/r7@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd: | raymarch_bwd:state | '
     'raymarch_normals_bwd:state,d_planes,g_normal | pointwise_bwd: x10'):
        'frozen/geometry/coords_grad/normal_grad/c/r7@normal',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/plain/none/normal_grad/c@all tuned/plain/none/normal_camera_grad/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a '
     '| raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/plain/none/normal_grad/c@normal tuned/plain/none/normal_camera_grad/c@normal',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/plain/none/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a '
     '| raymarch_bwd:state,rec_out | raymarch_bwd_camera: | raymarch_normals_bwd_camera:state,ray_grad,g_normal | '
     'raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/plain/none/normal_camera_grad/c_grad@normal',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b'
     ' | raymarch_bwd:state | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/plain/coords/none/c@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b'
     ' | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | '
     'pointwise_bwd: x10'):
        'tuned/plain/coords/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | '
     'pointwise_bwd: x10'):
        'tuned/plain/coords/normals/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/plain/coords/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/plain/coords/normal_grad/c@all tuned/plain/coords/normal_camera_grad/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        ('tuned/plain/coords/normal_grad/c@normal tuned/plain/coords/normal_camera_grad/c@normal '
         'tuned/plain/coords_grad/normal_grad/c@normal tuned/plain/coords_grad/normal_camera_grad/c@normal'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/plain/coords/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/plain/coords/normal_camera_grad/c_grad@normal tuned/plain/coords_grad/normal_camera_grad/c_grad@normal',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b'
     ' | raymarch_bwd:state | planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/plain/coords_grad/none/c@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b'
     ' | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb'
     ' | pointwise_bwd: x10'):
        'tuned/plain/coords_grad/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | '
     'pointwise_bwd: x10'):
        'tuned/plain/coords_grad/normals/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/plain/coords_grad/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/plain/coords_grad/normal_grad/c@all tuned/plain/coords_grad/normal_camera_grad/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/plain/coords_grad/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | '
     'planes_query_normals_bwd:d_planes,dec_out,g_grad,g_normal | pointwise_bwd: x10'):
        'tuned/plain/coords_qn/none/c@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,dec_out,g_grad,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/plain/coords_qn/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | '
     'planes_query_normals_bwd:d_planes,dec_out,g_grad,g_normal | pointwise_bwd: x10'):
        'tuned/plain/coords_qn/normals/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,dec_out,g_grad,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/plain/coords_qn/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/geometry/none/normal_grad/c@all tuned/geometry/none/normal_camera_grad/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/geometry/none/normal_grad/c@normal tuned/geometry/none/normal_camera_grad/c@normal',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/geometry/none/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/geometry/none/normal_camera_grad/c_grad@normal',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb '
     '| pointwise_bwd: x10'):
        'tuned/geometry/coords/none/c@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/geometry/coords/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/geometry/coords/normals/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | '
     'raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/geometry/coords/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: '
     'x10'):
        'tuned/geometry/coords/normal_grad/c@all tuned/geometry/coords/normal_camera_grad/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | raymarch_bwd:state | raymarch_normals_bwd:state,d_planes,dec_out,g_normal '
     '| pointwise_bwd: x10'):
        ('tuned/geometry/coords/normal_grad/c@normal tuned/geometry/coords/normal_camera_grad/c@normal '
         'tuned/geometry/coords_grad/normal_grad/c@normal tuned/geometry/coords_grad/normal_camera_grad/c@normal'),
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:'
     ' | raymarch_normals_bwd_camera:state,ray_grad,g_normal | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/geometry/coords/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/geometry/coords/normal_camera_grad/c_grad@normal tuned/geometry/coords_grad/normal_camera_grad/c_grad@normal',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/geometry/coords_grad/none/c@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/geometry/coords_grad/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/geometry/coords_grad/normals/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | '
     'raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | pointwise_bwd: x10'):
        'tuned/geometry/coords_grad/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/geometry/coords_grad/normal_grad/c@all tuned/geometry/coords_grad/normal_camera_grad/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:'
     ' | raymarch_normals_bwd_camera:state,ray_grad,g_normal | planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | '
     'raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/geometry/coords_grad/normal_camera_grad/c_grad@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb '
     '| planes_query_normals_bwd:d_planes,dec_out,g_grad,g_normal | pointwise_bwd: x10'):
        'tuned/geometry/coords_qn/none/c@all',
    ('raymarch_state: | raymarch:state | depth_clamp_: | depth_range: | planes_query_normals: | pointwise_bwd: x4 | '
     'pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | raymarch_bwd_camera:reduce | '
     'planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,dec_out,g_grad,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/geometry/coords_qn/none/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query_normals: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | planes_query_normals_bwd:d_planes,dec_out,g_grad,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/geometry/coords_qn/normals/c@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | depth_range: | planes_query_normals: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a,g_nchw3_b | raymarch_bwd:state,g_depth,g_wsum,rec_out | '
     'raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | '
     'planes_query_normals_bwd:d_planes,dec_out,g_grad,g_normal | pointwise_bwd: x10'):
        'tuned/geometry/coords_qn/normals/c_grad@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd:g_nchw3 | raymarch_bwd:state,g_depth,g_wsum,rec_out | '
     'raymarch_bwd_camera: | raymarch_normals_bwd_camera:state,ray_grad,g_normal | '
     'planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: '
     'x10'):
        'tuned/geometry/coords/normal_camera_grad/c_grad/planes/r7@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd: | raymarch_bwd:state,rec_out | raymarch_bwd_camera: | '
     'raymarch_normals_bwd_camera:state,ray_grad,g_normal | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/geometry/coords/normal_camera_grad/c_grad/planes/r7@normal',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | planes_query_normals: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd:g_nchw3 | raymarch_bwd:state,rec_out | '
     'raymarch_bwd_camera:reduce | planes_query_bwd:d_planes,dec_out,g_sigma,g_rgb | '
     'planes_query_normals_bwd:d_planes,dec_out,g_grad,g_normal | pointwise_bwd: x10'):
        'tuned/plain/coords_qn/normals/c_grad/planes/r7@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd:g_nchw3 | raymarch_bwd:state,g_depth,g_wsum | '
     'planes_query_bwd:d_planes,dec_out,coords_grad,g_sigma,g_rgb | raymarch_normals_bwd:state,d_planes,dec_out,g_normal | '
     'pointwise_bwd: x10'):
        'tuned/geometry/coords_grad/normal_grad/c/r7@all',
    ('raymarch_state: | raymarch:state | raymarch_normals:state | depth_clamp_: | resize_aa: | depth_range: | planes_query: | '
     'pointwise_bwd: x4 | pointwise_bwd:g_nchw3_a | resize_aa_bwd: | raymarch_bwd:state | '
     'raymarch_normals_bwd:state,d_planes,dec_out,g_normal | pointwise_bwd: x10'):
        'tuned/geometry/coords_grad/normal_grad/c/r7@normal',
}
EXPECTED = {cell: trace for trace, cs in PARENT_TRACES.items() for cell in cs.split()}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geometry", [False, True], ids=["plain", "geometry"])
@pytest.mark.parametrize("tuned", [False, True], ids=["frozen", "tuned"])
def test_matrix(dev, gens, tuned, geometry, mode):
    from hfa_gp_amd import ops
    gen = gens[tuned]
    base = {}
    with Recorder(ops) as rec:
        for cell in cells():
            if (cell[0], cell[2]) != (geometry, mode):
                continue
            _, query, _, c_grad, planes, res = cell
            cid = cell_id(tuned, *cell)
            traces, plain, under = run_cell(gen, dev, rec, *cell)
            # 1. the launch traces, and which outputs require grad
            for which, trace in traces.items():
                assert trace == EXPECTED[f"{cid}@{which}"], f"{cid}@{which}"
            # 2. forward bits: against the call without the keywords, under grad against no grad
            if res not in base:
                args, call = inputs(dev, res)
                with torch.no_grad():
                    base[res] = gen.synthesis(*args, **call)
            ref = base[res]
            assert set(ref) == {"image", "image_raw", "image_depth"}
            want = set(ref) | ({"image_mask"} if geometry else set()) | ({"image_normal"} if mode != "none" else set()) \
                | ({"query_sigma", "query_rgb"} if query != "none" else set()) \
                | ({"query_sigma_grad", "query_normal"} if query == "coords_qn" else set()) \
                | ({"planes", "feature_image"} if planes else set())
            assert set(plain) == want and set(under) == want, cid
            for k in ref:
                assert torch.equal(plain[k], ref[k]), f"{cid}: {k} against the plain call"
            for k in plain:
                assert torch.equal(plain[k], under[k].detach()), f"{cid}: {k} under grad"
                assert not plain[k].requires_grad, f"{cid}: {k} without grad"
            assert not SYNTHESIS_CALL_STATE & set(vars(gen)), cid


def test_a_call_leaves_nothing_on_the_generator(dev, gens, monkeypatch):
    """After a call with every normal keyword set, and after each refusal, none of the attributes that once carried a call's request
    on the module exists; a plain call then has EG3D's three keys and the bits of a plain call made before."""
    from hfa_gp_amd import generator as Gn
    gen, cfg = gens[True], _cfg()
    args, call = inputs(dev)
    with torch.no_grad():
        before = gen.synthesis(*args, **call)
    (ws, c), call = inputs(dev, query="coords", c_grad=True)
    out = gen.synthesis(ws, c, **call, normals=True, normal_grad=True, normal_camera_grad=True, geometry=True, return_planes=True)
    assert not SYNTHESIS_CALL_STATE & set(vars(gen))
    loss_of(out, "all").backward()
    gen.zero_grad(set_to_none=True)
    q = call.pop("query")
    call.pop("query_normals")
    frame = cfg.neural_rendering_resolution ** 2 * (cfg.depth_resolution + cfg.depth_resolution_importance) * 140
    refusals = (
        (ValueError, "query_normals=True needs query", dict(query_normals=True)),
        (NotImplementedError, "together with normal_grad=True", dict(query=q, query_normals=True, normal_grad=True)),
        (NotImplementedError, "no gradient w.r.t. the\\s+points", dict(query=q.clone().requires_grad_(True), query_normals=True,
                                                                    normals=True)),
        (NotImplementedError, "camera gradient of the normal term", dict(normal_grad=True)),
        (RuntimeError, f"RAY_STATE_CAP_BYTES = {frame}; 1 frames fit", dict(normal_camera_grad=True)),
        (ValueError, "expected query \\[B or 1, M, 3\\]", dict(query=q[0], normals=True)),
        (ValueError, "neural_rendering_resolution=1000 must be", dict(normals=True, neural_rendering_resolution=1000)),
    )
    for exc, match, kw in refusals:
        if exc is RuntimeError:
            monkeypatch.setattr(Gn, "RAY_STATE_CAP_BYTES", frame)
        with pytest.raises(exc, match=match):
            gen.synthesis(ws, c, **{**call, **kw})
        monkeypatch.undo()
        assert not SYNTHESIS_CALL_STATE & set(vars(gen)), match
    with torch.no_grad():
        after = gen.synthesis(*args, **call)
    assert list(after) == ["image", "image_raw", "image_depth"]
    for k in after:
        assert torch.equal(after[k], before[k]), k


# sample_mixed(differentiable=True) on the commit above: (normals, loss) -> the trace of the planes_query* ops, forward | backward
PARENT_SAMPLE_MIXED = {
    'frozen/plain@sigma': 'planes_query: | planes_query_bwd:g_sigma',
    'frozen/normals@sigma': 'planes_query_normals: | planes_query_bwd:g_sigma',
    'frozen/normals@normal': 'planes_query_normals: | planes_query_normals_bwd:g_normal',
    'frozen/normals@both': 'planes_query_normals: | planes_query_bwd:g_sigma | planes_query_normals_bwd:d_planes,g_normal',
    'tuned/plain@sigma': 'planes_query: | planes_query_bwd:dec_out,g_sigma',
    'tuned/normals@sigma': 'planes_query_normals: | planes_query_bwd:dec_out,g_sigma',
    'tuned/normals@normal': 'planes_query_normals: | planes_query_normals_bwd:dec_out,g_normal',
    'tuned/normals@both': ('planes_query_normals: | planes_query_bwd:dec_out,g_sigma | '
                           'planes_query_normals_bwd:d_planes,dec_out,g_normal'),
}


@pytest.mark.parametrize("tuned", [False, True], ids=["frozen", "tuned"])
def test_sample_mixed(dev, gens, tuned):
    from hfa_gp_amd import ops
    gen = gens[tuned]
    got = {}
    with Recorder(ops) as rec:
        for normals, which in ((False, "sigma"), (True, "sigma"), (True, "normal"), (True, "both")):
            (ws, _), call = inputs(dev, query="coords")
            out = gen.sample_mixed(call["query"], None, ws, differentiable=True, normals=normals)
            assert list(out) == ["rgb", "sigma"] + (["sigma_grad", "normal"] if normals else [])
            assert all(v.requires_grad for v in out.values())
            sum(out[k].sum() for k in {"sigma": ["sigma"], "normal": ["normal"], "both": ["sigma", "normal"]}[which]).backward()
            assert bool(torch.isfinite(ws.grad).all()) and float(ws.grad.abs().max()) > 0
            got[f"{'tuned' if tuned else 'frozen'}/{'normals' if normals else 'plain'}@{which}"] = rec.take(
                lambda call: call.startswith("planes_query"))
            gen.zero_grad(set_to_none=True)
    assert got == {k: v for k, v in PARENT_SAMPLE_MIXED.items() if k.startswith("tuned" if tuned else "frozen")}
