"""The structures the six renderer entry points of ops.py hand to the library (raymarch, raymarch_normals, raymarch_bwd,
raymarch_bwd_camera, planes_query, planes_query_bwd), field by field against expectations written out by hand; the frame chunks of
raymarch_bwd with every optional input on; and the calls the wrappers must refuse before anything reaches the library (it sees
pointers and integers, never a tensor's extent).  Needs an MI355X:  python -m pytest tests -m gpu

One shape throughout: B = 2, 20 x 20 planes, 10 x 10 rays, small128's 32 + 32 samples, built as test_gpu_camera_grad.device_call
builds its inputs (no oracle pass)."""
import ctypes as C
import dataclasses
import types

import pytest
import torch

from tests.util import look_at_label, perturb_state

pytestmark = pytest.mark.gpu

B, HW, RES, R, M = 2, 20, 10, 100, 37
NONNULL = object()           # a pointer the test cannot know (a buffer the wrapper allocates for itself): anything but null
AXES = [(1, "eg3d_fixed"), (0, "eg3d_original")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def S(dev):
    """The inputs, made once and never written."""
    from hfa_gp_amd import _lib, ops
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = dataclasses.replace(PRESETS["small128"](), neural_rendering_resolution=RES, img_resolution=4 * RES, white_back=True)
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).to(dev)
    g = torch.Generator().manual_seed(4)
    sc, sf = cfg.depth_resolution, cfg.depth_resolution_importance
    s = types.SimpleNamespace(cfg=cfg, sc=sc, sf=sf, dec=gen.decoder_params())
    s.planes = torch.randn(B, 3, 32, HW, HW, generator=g).permute(0, 1, 3, 4, 2).contiguous().to(dev)
    s.u_strat, s.u_imp = gen._uniforms(B, dev, torch.rand(B, R, sc, 1, generator=g).to(dev), torch.rand(B * R, sf, generator=g).to(dev))
    s.args = gen._render_args(look_at_label(torch.tensor([1.3, 1.8]), torch.tensor([1.5, 1.7])).to(dev))
    s.g_feat, s.g_depth, s.g_wsum = (torch.randn(*shape, generator=g).to(dev) for shape in ((B, R, 32), (B, R), (B, R)))
    s.bound = s.planes.abs().amax().expand(_lib.ABSMAX_FLOATS).contiguous()
    s.state = ops.raymarch_state(B, RES, sc, sf, dev)
    with torch.no_grad():
        tmm = ops.raymarch(s.planes, u_strat=s.u_strat, u_imp=s.u_imp, state=s.state, planes_absmax=s.bound, **s.args)[3]
        s.depth_range = ops.depth_range(tmm)
        s.rec = ops.raymarch_bwd(s.g_feat, s.planes, u_strat=s.u_strat, u_imp=s.u_imp, planes_absmax=s.bound, return_rec=True,
                                 **s.args)[1]
    s.coords = (0.4 * torch.randn(B, M, 3, generator=g)).to(dev)
    s.g_sigma, s.g_rgb = torch.randn(B, M, 1, generator=g).to(dev), torch.randn(B, M, 32, generator=g).to(dev)
    s.query = {k: s.args[k] for k in ("dec_w0", "dec_b0", "dec_w1", "dec_b1", "box_warp", "decoder_lr_mul", "decoder_precision")}
    return s


class Recorder:
    """Stands in for the library handle: forwards every call, keeping first a byte copy of each structure passed by reference."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.calls.append((name, [type(x._obj).from_buffer_copy(x._obj) for x in args if hasattr(x, "_obj")]))
            return fn(*args)
        return call

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture
def rec(dev, monkeypatch):
    from hfa_gp_amd import _lib
    monkeypatch.delenv("HFAGP_RAYBWD_ROWS", raising=False)
    monkeypatch.delenv("HFAGP_RAYBWD_SCRATCH_GIB", raising=False)
    r = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: r)
    return r


def ptr(t):
    return t if t is NONNULL or t is None else t.data_ptr()


def same(struct, expect, where=""):
    """EVERY field of `struct` against `expect`; a field `expect` does not name must be 0 / null."""
    unknown = set(expect) - {n for n, _ in struct._fields_}
    assert not unknown, f"{where}: the expectation names fields the structure does not have: {unknown}"
    for name, kind in struct._fields_:
        got, want = getattr(struct, name), expect.get(name, 0)
        if isinstance(got, C.Structure):
            same(got, want, f"{where}{name}.")
        elif want is NONNULL:
            assert got, f"{where}{name} is null"
        elif kind is C.c_void_p:
            assert (got or 0) == (want or 0), f"{where}{name}: {got} != {want}"
        else:
            assert got == kind(want).value, f"{where}{name}: {got} != {want}"


def ray_fields(S, axes, *, bound, state=None):
    """RaymarchArgs of the shared scene, without the forward's four output pointers."""
    a = S.args
    return dict(planes=ptr(S.planes), cam2world=ptr(a["cam2world"]), intrinsics=ptr(a["intrinsics"]), u_strat=ptr(S.u_strat),
                u_imp=ptr(S.u_imp), dec_w0=ptr(S.dec[0]), dec_b0=ptr(S.dec[1]), dec_w1=ptr(S.dec[2]), dec_b1=ptr(S.dec[3]),
                B=B, H=HW, W=HW, res=RES, Sc=S.sc, Sf=S.sf, plane_axes=axes, white_back=1, ray_start=S.cfg.ray_start,
                ray_end=S.cfg.ray_end, box_warp=S.cfg.box_warp, decoder_lr_mul=S.cfg.decoder_lr_mul, planes_absmax=ptr(bound),
                state=ptr(state))


def spellings(S, axes):
    """The scene keywords with plane_axes once as the library's code, once as the config's name."""
    return [dict(S.args, plane_axes=spelling) for spelling in axes]


@pytest.mark.parametrize("axes", AXES, ids=[a[1] for a in AXES])
def test_raymarch_and_normals_structures(S, rec, axes):
    from hfa_gp_amd import ops
    cases = [("fp32", None, None), ("f16x3", S.bound, S.bound), ("f16x3", None, NONNULL)]
    for kw in spellings(S, axes):
        for state in (None, S.state.clone()):
            for precision, given, want in cases:
                out = ops.raymarch(S.planes, u_strat=S.u_strat, u_imp=S.u_imp, state=state, planes_absmax=given,
                                   **dict(kw, decoder_precision=precision))
                (name, (a,)), = rec.take()
                assert name == "hfagp_raymarch_fwd"
                same(a, dict(ray_fields(S, axes[0], bound=want, state=state), feat=ptr(out[0]), depth=ptr(out[1]), wsum=ptr(out[2]),
                             tminmax=ptr(out[3])))
        ops.raymarch_normals(S.planes, S.state, u_strat=S.u_strat, u_imp=S.u_imp, planes_absmax=S.bound, **kw)
        (name, (a,)), = rec.take()
        assert name == "hfagp_raymarch_normals"
        same(a, ray_fields(S, axes[0], bound=S.bound, state=S.state))


def rows_bytes(S, axes):
    """hfagp_raymarch_bwd_rows_bytes of a forward structure filled here."""
    from hfa_gp_amd import _lib
    f = _lib.RaymarchArgs()
    for k, v in ray_fields(S, axes, bound=S.bound).items():
        setattr(f, k, v)
    return int(_lib.lib().real.hfagp_raymarch_bwd_rows_bytes(C.byref(f)))


@pytest.mark.parametrize("axes", AXES, ids=[a[1] for a in AXES])
def test_raymarch_bwd_structures(S, rec, axes):
    from hfa_gp_amd import ops
    need = rows_bytes(S, axes[0])
    assert need > 0, "the sort + gather backward must apply at this shape for the rows=True case to mean anything"
    dec_out = tuple(torch.zeros_like(p) for p in S.dec)
    for kw in spellings(S, axes):
        call = lambda **more: ops.raymarch_bwd(S.g_feat, S.planes, u_strat=S.u_strat, u_imp=S.u_imp, planes_absmax=S.bound,  # noqa: E731
                                               **kw, **more)
        fwd = ray_fields(S, axes[0], bound=S.bound)
        # plain: the default is the sort + gather pass 2, whose scratch the wrapper sizes by asking the library
        d_planes, r = call(return_rec=True)
        (n0, (f,)), (n1, (a,)) = rec.take()
        assert (n0, n1) == ("hfagp_raymarch_bwd_rows_bytes", "hfagp_raymarch_bwd")
        same(f, fwd)
        same(a, dict(fwd=fwd, g_feat=ptr(S.g_feat), d_planes=ptr(d_planes), rec=ptr(r), rows_scratch=NONNULL, rows_scratch_bytes=need))
        # rows=True says the same; rows=False asks the library nothing and brings no scratch
        d_planes, r = call(return_rec=True, rows=True)
        (n0, _), (n1, (a,)) = rec.take()
        assert (n0, n1) == ("hfagp_raymarch_bwd_rows_bytes", "hfagp_raymarch_bwd")
        same(a, dict(fwd=fwd, g_feat=ptr(S.g_feat), d_planes=ptr(d_planes), rec=ptr(r), rows_scratch=NONNULL, rows_scratch_bytes=need))
        d_planes, r = call(return_rec=True, rows=False)
        (name, (a,)), = rec.take()
        assert name == "hfagp_raymarch_bwd"
        same(a, dict(fwd=fwd, g_feat=ptr(S.g_feat), d_planes=ptr(d_planes), rec=ptr(r)))
        # decoder gradients into the caller's four tensors; the forward's state
        rec_out = []
        d_planes, dec = call(rows=False, decoder_grads=True, dec_out=dec_out, state=S.state, rec_out=rec_out)
        (name, (a,)), = rec.take()
        assert name == "hfagp_raymarch_bwd" and all(x is y for x, y in zip(dec, dec_out))
        same(a, dict(fwd=dict(fwd, state=ptr(S.state)), g_feat=ptr(S.g_feat), d_planes=ptr(d_planes), rec=ptr(rec_out[0]),
                     d_dec_w0=ptr(dec_out[0]), d_dec_b0=ptr(dec_out[1]), d_dec_w1=ptr(dec_out[2]), d_dec_b1=ptr(dec_out[3])))
        # depth and opacity gradients: the second structure, through the _geom entry
        d_planes, r = call(return_rec=True, rows=False, g_depth=S.g_depth, g_wsum=S.g_wsum, depth_range=S.depth_range)
        (name, (a, gg)), = rec.take()
        assert name == "hfagp_raymarch_bwd_geom"
        same(a, dict(fwd=fwd, g_feat=ptr(S.g_feat), d_planes=ptr(d_planes), rec=ptr(r)))
        same(gg, dict(g_depth=ptr(S.g_depth), g_wsum=ptr(S.g_wsum), depth_range=ptr(S.depth_range)))
        # the camera gradient reads the records of such a call
        out = ops.raymarch_bwd_camera(S.g_feat, S.planes, S.rec, u_strat=S.u_strat, u_imp=S.u_imp, planes_absmax=S.bound, **kw)
        (name, (a,)), = rec.take()
        assert name == "hfagp_raymarch_bwd_camera" and [tuple(t.shape) for t in out] == [(B, 16), (B, 9), (B, R, 6)]
        same(a, dict(fwd=fwd, g_feat=ptr(S.g_feat), rec=ptr(S.rec)))


@pytest.mark.parametrize("axes", AXES, ids=[a[1] for a in AXES])
def test_planes_query_structures(S, rec, axes):
    from hfa_gp_amd import ops
    cube, vol = 0.75, torch.zeros(B, 8, 8, 8, device=S.planes.device)
    for spelling in axes:
        kw = dict(S.query, plane_axes=spelling, planes_absmax=S.bound)
        common = dict(planes=ptr(S.planes), dec_w0=ptr(S.dec[0]), dec_b0=ptr(S.dec[1]), dec_w1=ptr(S.dec[2]), dec_b1=ptr(S.dec[3]),
                      planes_absmax=ptr(S.bound), B=B, H=HW, W=HW, plane_axes=axes[0], decoder_lr_mul=S.cfg.decoder_lr_mul,
                      box_warp=S.cfg.box_warp)
        for coords in (S.coords, S.coords[:1]):                      # one set of points per identity; one set for all of them
            sigma, rgb = ops.planes_query(S.planes, coords, **kw)
            (name, (a,)), = rec.take()
            assert name == "hfagp_planes_query" and sigma.shape == (B, M, 1) and rgb.shape == (B, M, 32)
            same(a, dict(common, coords=ptr(coords), Bc=coords.shape[0], M=M, sigma=ptr(sigma), rgb=ptr(rgb)))
        out = vol[:, 2:5]                                            # a slab of a whole volume: strided over the identities
        sigma, rgb = ops.planes_query(S.planes, grid=(8, cube, 2, 3), want_rgb=False, out=out, **kw)
        (name, (a,)), = rec.take()
        assert name == "hfagp_planes_query" and sigma is out and rgb is None
        same(a, dict(common, sigma=ptr(out), N=8, x_begin=2, x_count=3, cube_length=cube, out_stride=512))
        # the backward: everything on, then the plane gradient alone, then without it
        both = dict(common, coords=ptr(S.coords), Bc=B, M=M, g_sigma=ptr(S.g_sigma), g_rgb=ptr(S.g_rgb))
        d_planes, d_coords, dec = ops.planes_query_bwd(S.planes, S.coords, S.g_sigma, S.g_rgb, coords_grad=True, decoder_grads=True, **kw)
        (name, (a,)), = rec.take()
        assert name == "hfagp_planes_query_bwd"
        same(a, dict(both, d_planes=ptr(d_planes), d_coords=ptr(d_coords), d_dec_w0=ptr(dec[0]), d_dec_b0=ptr(dec[1]),
                     d_dec_w1=ptr(dec[2]), d_dec_b1=ptr(dec[3])))
        d_planes, d_coords, dec = ops.planes_query_bwd(S.planes, S.coords, S.g_sigma, S.g_rgb, **kw)
        (name, (a,)), = rec.take()
        assert d_coords is None and dec is None
        same(a, dict(both, d_planes=ptr(d_planes)))
        d_planes, d_coords, dec = ops.planes_query_bwd(S.planes, S.coords[:1], None, S.g_rgb, d_planes=False, coords_grad=True, **kw)
        (name, (a,)), = rec.take()
        assert d_planes is None and dec is None
        same(a, dict(common, coords=ptr(S.coords), Bc=1, M=M, g_rgb=ptr(S.g_rgb), d_coords=ptr(d_coords)))


def test_frame_chunks_with_every_optional_input(S, dev, monkeypatch):
    """Two chunks of one frame (the scratch cap forced to 1.2 frames' worth) against the one-piece call, with the forward's state,
    the depth and opacity gradients, the decoder gradients and rec_out all on: the record is bit-equal, the plane and decoder
    gradients agree to the run-to-run noise of their atomic adds (the bars of the round-6 chunk test)."""
    from hfa_gp_amd import ops
    monkeypatch.delenv("HFAGP_RAYBWD_SCRATCH_GIB", raising=False)

    def call():
        rec_out = []
        with torch.no_grad():
            d_planes, dec = ops.raymarch_bwd(S.g_feat, S.planes, u_strat=S.u_strat, u_imp=S.u_imp, planes_absmax=S.bound, rows=True,
                                             state=S.state, g_depth=S.g_depth, g_wsum=S.g_wsum, depth_range=S.depth_range,
                                             decoder_grads=True, rec_out=rec_out, **S.args)
        assert len(rec_out) == 1 and rec_out[0].shape == (B, R, S.sc + S.sf, 4)
        return d_planes, dec, rec_out[0]

    whole = call()
    assert ops.ROWS_STATS["path"] == "rows" and ops.ROWS_STATS["chunks"] == 1
    one_frame = ops.ROWS_STATS["bytes"] / B
    monkeypatch.setenv("HFAGP_RAYBWD_SCRATCH_GIB", str(1.2 * one_frame / 2 ** 30))
    parts = call()
    assert ops.ROWS_STATS["path"] == "rows" and ops.ROWS_STATS["chunks"] == 2, ops.ROWS_STATS
    assert torch.equal(parts[2], whole[2])
    scale = whole[0].abs().max().item()
    err = (parts[0] - whole[0]).abs().max().item()
    print(f"d planes: max |chunks - whole| {err:.3e} at scale {scale:.3e}")
    assert scale > 0 and err <= 1e-5 * scale
    for x, y in zip(parts[1], whole[1]):
        print(f"decoder gradient {tuple(y.shape)}: max |chunks - whole| {(x - y).abs().max().item():.3e} at scale {y.abs().max().item():.3e}")
        assert (x - y).abs().max().item() <= 2e-5 * y.abs().max().item()


def _short_dec_out(S):
    return tuple(torch.zeros_like(p)[:-1] if i == 2 else torch.zeros_like(p) for i, p in enumerate(S.dec))


REFUSALS = {     # what to change in a valid call -> the entry points that must refuse it
    "planes with 16 channels": (lambda S: dict(planes=S.planes[..., :16].contiguous()), ("raymarch_bwd", "raymarch_bwd_camera")),
    "u_imp one row short": (lambda S: dict(u_imp=S.u_imp[:-1]), ("raymarch_bwd", "raymarch_bwd_camera")),
    "dec_w0 on the host": (lambda S: dict(dec_w0=S.dec[0].cpu()), ("raymarch_bwd", "raymarch_bwd_camera")),
    "dec_w1 a transposed view": (lambda S: dict(dec_w1=S.dec[2].t().contiguous().t()), ("raymarch_bwd", "raymarch_bwd_camera")),
    "g_feat with 16 channels": (lambda S: dict(g_feat=S.g_feat[..., :16].contiguous()), ("raymarch_bwd",)),
    "dec_out with one wrong shape": (lambda S: dict(decoder_grads=True, dec_out=_short_dec_out(S)), ("raymarch_bwd", "planes_query_bwd")),
}


@pytest.mark.parametrize("what,who", [(k, w) for k, (_, whos) in REFUSALS.items() for w in whos])
def test_refusals_launch_nothing(S, rec, what, who):
    from hfa_gp_amd import ops
    change = REFUSALS[what][0](S)
    if who == "planes_query_bwd":
        kw = dict(S.query, planes=S.planes, coords=S.coords, g_sigma=S.g_sigma, g_rgb=S.g_rgb, plane_axes=0, planes_absmax=S.bound)
    else:
        kw = dict(S.args, g_feat=S.g_feat, planes=S.planes, u_strat=S.u_strat, u_imp=S.u_imp, planes_absmax=S.bound)
        if who == "raymarch_bwd_camera":
            kw["rec"] = S.rec
    with pytest.raises(RuntimeError, match=rf"^{who}: "):
        getattr(ops, who)(**{**kw, **change})
    assert rec.calls == [], f"{who} refused '{what}' only after {[n for n, _ in rec.calls]}"
