"""Explicit ray lists without a GPU: `cam_utils.ray_grid` against the oracle's RaySampler (values, crop window, gradient of the
label), the argument checks of the hfagp_raymarch_rays_* entry points through ctypes (nothing is launched), the unchanged layout
of the grid structs, and the CPU refusal of `TriPlaneGenerator.render_rays`."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.util import ROOT, look_at_label

BAR = 1e-6                 # absolute: 4 ulp of the largest value (the camera distance 2.7)


def labels():
    """Two look_at_label cameras and one label with skew and an off-centre principal point."""
    c = look_at_label(torch.tensor([1.3, 1.8, 1.55]), torch.tensor([1.5, 1.7, 1.45]))
    c[2, 16:25] = torch.tensor([3.9, 0.21, 0.47, 0.0, 4.4, 0.55, 0.0, 0.0, 1.0])
    return c


def oracle_rays(c, res):
    from oracle import eg3d_oracle as O
    return O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:25].reshape(-1, 3, 3), res)


@pytest.mark.parametrize("res", [1, 7, 10, 64])
def test_ray_grid_is_the_oracles_ray_sampler(res):
    from hfa_gp_amd.cam_utils import ray_grid
    c = labels()
    o, d = ray_grid(c, res)
    oo, dd = oracle_rays(c, res)
    assert o.shape == d.shape == (3, res * res, 3) and o.dtype == torch.float32
    print(f"res {res}: max |d origin| {float((o - oo).abs().max()):.3e}, max |d direction| {float((d - dd).abs().max()):.3e}, "
          f"bit-equal {torch.equal(o, oo) and torch.equal(d, dd)}")
    assert float((o - oo).abs().max()) <= BAR and float((d - dd).abs().max()) <= BAR
    assert float((d.norm(dim=-1) - 1).abs().max()) <= 1e-6


def test_window_is_a_crop_of_the_finer_grid():
    """The pixel centres of window (.25, .25, .75, .75) at res 10 are those of rows / columns 5..14 at res 20: 0.275 ... 0.725."""
    from hfa_gp_amd.cam_utils import ray_grid
    c = labels()
    o, d = ray_grid(c, 10, window=(.25, .25, .75, .75))
    of, df = ray_grid(c, 20)
    crop = lambda t: t.reshape(3, 20, 20, 3)[:, 5:15, 5:15].reshape(3, 100, 3)      # noqa: E731
    assert float((o - crop(of)).abs().max()) <= BAR and float((d - crop(df)).abs().max()) <= BAR
    # the whole image as a window is the plain grid; u runs along a row, v down the rows
    ow, dw = ray_grid(c, 10, window=(0, 0, 1, 1))
    assert float((dw - ray_grid(c, 10)[1]).abs().max()) <= BAR and torch.equal(ow, ray_grid(c, 10)[0])
    # (u0, v0, u1, v1): the top-right quarter is rows 0..3 (v) and columns 4..7 (u) of the 8 x 8 grid, not its transpose
    fine = ray_grid(c, 8)[1].reshape(3, 8, 8, 3)
    quarter = ray_grid(c, 4, window=(.5, 0, 1, .5))[1].reshape(3, 4, 4, 3)
    assert float((quarter - fine[:, 0:4, 4:8]).abs().max()) <= BAR
    assert float((quarter - fine[:, 4:8, 0:4]).abs().max()) > 1e-2


def test_label_gradient_through_ray_grid():
    """c.grad of a loss on the rays against the oracle's autograd of ray_sampler: the same graph, so the same bar as the values
    scaled by the gradient's size."""
    from hfa_gp_amd.cam_utils import ray_grid
    g = torch.Generator().manual_seed(5)
    res = 9
    wo, wd = torch.randn(3, res * res, 3, generator=g), torch.randn(3, res * res, 3, generator=g)
    c = labels().requires_grad_(True)
    o, d = ray_grid(c, res)
    ((o * wo).sum() + (d * wd).sum()).backward()
    cr = labels().requires_grad_(True)
    oo, dd = oracle_rays(cr, res)
    ((oo * wo).sum() + (dd * wd).sum()).backward()
    scale = float(cr.grad.abs().max())
    assert scale > 0 and float((c.grad - cr.grad).abs().max()) <= BAR * max(1.0, scale)
    # ... and through a window (float64: the graph itself, against central differences of one intrinsic)
    c64 = labels().double().requires_grad_(True)
    f = lambda t: (ray_grid(t, 5, window=(.1, .2, .6, .9))[1] * wd[:, :25].double()).sum()      # noqa: E731
    f(c64).backward()
    e = torch.zeros_like(c64)
    e[1, 16] = 1e-6
    num = (f(c64.detach() + e) - f(c64.detach() - e)) / 2e-6
    assert abs(float(num) - float(c64.grad[1, 16])) <= 1e-6 * max(1.0, abs(float(num)))


# ----------------------------------------------------------------------------- the C ABI, nothing launched
@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    _lib.lib()
    return _lib


def _filled_list(lib, cls):
    """A ray-list struct whose pointers are non-null and never dereferenced: every call below is refused before a launch."""
    a = cls()
    f = a.base if cls is lib.RayListArgs else a.bwd.fwd
    for k in ("planes", "u_strat", "u_imp", "dec_w0", "dec_b0", "dec_w1", "dec_b1", "feat", "depth", "wsum", "tminmax"):
        setattr(f, k, 256)
    f.B, f.H, f.W, f.Sc, f.Sf = 2, 20, 20, 24, 24            # 24 + 24 samples: unsupported, so a call that passes the other checks is -2
    f.ray_start, f.ray_end, f.box_warp, f.decoder_lr_mul = 2.25, 3.3, 1.0, 1.0
    a.ray_origins, a.ray_directions, a.R = 256, 256, 101
    if cls is lib.RayListBwdArgs:
        a.bwd.g_feat, a.bwd.d_planes, a.bwd.rec = 256, 256, 256
    return a


def test_abi_is_15_and_the_grid_structs_keep_their_layout(lib):
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    assert re.search(r"#define HFAGP_ABI_VERSION 15\b", text) and lib.ABI_VERSION == 15 and lib.lib().hfagp_abi_version() == 15
    # 13 pointers, 8 int32, 2 doubles, 2 floats, 2 pointers; then the backward's 8 pointers and the scratch size
    assert C.sizeof(lib.RaymarchArgs) == 176 and C.sizeof(lib.RaymarchBwdArgs) == 256
    off = {n: getattr(lib.RaymarchArgs, n).offset for n, _ in lib.RaymarchArgs._fields_}
    assert [off[n] for n in ("planes", "cam2world", "intrinsics", "u_strat", "tminmax", "B", "res", "Sc", "white_back", "ray_start",
                             "ray_end", "box_warp", "decoder_lr_mul", "planes_absmax", "state")] == \
        [0, 8, 16, 24, 96, 104, 116, 120, 132, 136, 144, 152, 156, 160, 168]
    offb = {n: getattr(lib.RaymarchBwdArgs, n).offset for n, _ in lib.RaymarchBwdArgs._fields_}
    assert [offb[n] for n in ("fwd", "g_feat", "d_planes", "rec", "d_dec_w0", "d_dec_b1", "df_scratch", "rows_scratch",
                              "rows_scratch_bytes")] == [0, 176, 184, 192, 200, 224, 232, 240, 248]
    # the new structs wrap the old ones: additive
    assert lib.RayListArgs.base.offset == 0 and lib.RayListArgs.ray_origins.offset == 176 and lib.RayListArgs.R.offset == 192
    assert lib.RayListBwdArgs.bwd.offset == 0 and lib.RayListBwdArgs.ray_origins.offset == 256 and lib.RayListBwdArgs.R.offset == 272
    nocomment = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("hfagp_raymarch_rays_fwd", "hfagp_raymarch_rays_bwd", "hfagp_raymarch_rays_bwd_rows_bytes",
                 "hfagp_raymarch_rays_bwd_rays"):
        assert re.search(r"\b%s\(" % name, nocomment) and name in lib.SYMBOLS, name


def test_forward_entry_checks_its_arguments(lib):
    h = lib.lib()
    fn = h.hfagp_raymarch_rays_fwd
    assert fn(None, None) == -1
    a = _filled_list(lib, lib.RayListArgs)
    assert fn(C.byref(a), None) == -2 and b"unsupported sample counts" in h.hfagp_last_error()      # camera NULL, res 0: ignored
    for field in ("ray_origins", "ray_directions"):
        a = _filled_list(lib, lib.RayListArgs)
        setattr(a, field, None)
        assert fn(C.byref(a), None) == -1 and b"null pointer" in h.hfagp_last_error(), field
    for r in (0, -3):
        a = _filled_list(lib, lib.RayListArgs)
        a.R = r
        assert fn(C.byref(a), None) == -1 and b"rays per frame" in h.hfagp_last_error(), r
    a = _filled_list(lib, lib.RayListArgs)
    a.base.feat = None
    assert fn(C.byref(a), None) == -1
    a = _filled_list(lib, lib.RayListArgs)
    a.base.Sc = a.base.Sf = 16
    a.base.B, a.R = 1 << 16, 1 << 15                      # B * R = 2^31
    assert fn(C.byref(a), None) == -2 and b"too many rays" in h.hfagp_last_error()


def test_backward_entries_check_their_arguments(lib):
    h = lib.lib()
    bwd, rays, nbytes = h.hfagp_raymarch_rays_bwd, h.hfagp_raymarch_rays_bwd_rays, h.hfagp_raymarch_rays_bwd_rows_bytes
    assert bwd(None, None, None) == -1 and rays(None, 256, 256, None) == -1 and nbytes(None) == 0
    a = _filled_list(lib, lib.RayListBwdArgs)
    assert bwd(C.byref(a), None, None) == -2 and rays(C.byref(a), 256, 256, None) == -2
    for field in ("ray_origins", "ray_directions"):
        a = _filled_list(lib, lib.RayListBwdArgs)
        setattr(a, field, None)
        assert bwd(C.byref(a), None, None) == -1 and rays(C.byref(a), 256, 256, None) == -1, field
    a = _filled_list(lib, lib.RayListBwdArgs)
    a.R = 0
    assert bwd(C.byref(a), None, None) == -1 and rays(C.byref(a), 256, 256, None) == -1
    a = _filled_list(lib, lib.RayListBwdArgs)
    assert rays(C.byref(a), None, 256, None) == -1 and rays(C.byref(a), 256, None, None) == -1
    a.bwd.g_feat = None
    assert bwd(C.byref(a), None, None) == -1 and b"no upstream gradient" in h.hfagp_last_error()
    g = lib.RaymarchGeomGrads()
    g.g_depth = 256
    assert bwd(C.byref(a), C.byref(g), None) == -1 and b"depth_range" in h.hfagp_last_error()
    # the scratch size: a pure function of the shapes, sized by R (not by res), 0 for R <= 0
    f = _filled_list(lib, lib.RayListArgs)
    f.base.Sc = f.base.Sf = 16
    n101 = nbytes(C.byref(f))
    f.R = 202
    n202 = nbytes(C.byref(f))
    f.base.res = 77
    assert n101 > 0 and n202 > n101 and nbytes(C.byref(f)) == n202
    f.R = 0
    assert nbytes(C.byref(f)) == 0
    # the grid's own scratch size is what it was: res * res rays per frame
    grid = lib.RaymarchArgs()
    grid.B, grid.H, grid.W, grid.res, grid.Sc, grid.Sf = 2, 20, 20, 10, 16, 16
    f.R = 100
    assert h.hfagp_raymarch_bwd_rows_bytes(C.byref(grid)) == nbytes(C.byref(f)) > 0


def test_render_rays_refuses_cpu_tensors_and_bad_shapes():
    from hfa_gp_amd.config import tiny64
    from hfa_gp_amd.generator import TriPlaneGenerator
    g = TriPlaneGenerator(tiny64())
    ws = torch.zeros(2, g.cfg.num_ws, 512)
    rays = torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.render_rays(ws, rays, rays)
    with pytest.raises(ValueError, match=r"\[B, R, 3\]"):
        g.render_rays(ws, torch.zeros(3, 5, 3), torch.zeros(3, 5, 3))            # rays.shape[0] must equal ws.shape[0]
    with pytest.raises(ValueError, match="must match"):
        g.render_rays(ws, rays, torch.zeros(2, 6, 3))
    with pytest.raises(TypeError, match="floating-point"):
        g.render_rays(ws, rays.long(), rays)
    with pytest.raises(NotImplementedError, match="noise_mode"):
        g.render_rays(ws, rays, rays, noise_mode="random")
