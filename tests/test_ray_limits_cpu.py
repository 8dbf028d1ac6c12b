"""Per-ray depth limits, the parts that need no GPU: cam_utils.ray_limits_box (the reference of hfagp_ray_limits_box) against a
float64 slab computation and closed-form cases, cam_utils.ray_grid_ortho's geometry, the reference renderer with limits
(tests/ray_limits_ref.py) against the untouched oracle where the two must agree, its empty-ray semantics, and the argument checks
of the new entry points through ctypes (nothing is launched)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import ray_limits_ref as RL
from tests.test_gpu_render_rays import B, R
from tests.util import ROOT

NAN, INF = float("nan"), float("inf")


def slab64(o, d, side):
    """The slab method in float64, axis by axis in Python floats: IEEE division, NaN makes the ray empty."""
    h = side / 2
    near, far, nan = -INF, INF, False
    for k in range(3):
        ok, dk = float(o[k]), float(d[k])
        inv = math.copysign(INF, dk) if dk == 0.0 else 1.0 / dk
        lo, hi = -h - ok, h - ok
        t0 = NAN if (lo == 0.0 and math.isinf(inv)) else lo * inv
        t1 = NAN if (hi == 0.0 and math.isinf(inv)) else hi * inv
        if math.isnan(t0) or math.isnan(t1):
            nan = True
            continue
        near, far = max(near, min(t0, t1)), min(far, max(t0, t1))
    return (NAN, NAN) if nan else (max(near, 0.0), far)


@pytest.mark.parametrize("side", [1.0, 2.0])
@pytest.mark.parametrize("name", ["mixed", "miss"])
def test_ray_limits_box_vs_float64_slabs(name, side):
    from hfa_gp_amd.cam_utils import ray_limits_box, ray_limits_valid
    o, d = RL.LISTS[name]()
    tn, tf = ray_limits_box(o, d, side)
    assert tn.shape == tf.shape == (B, R) and tn.dtype == torch.float32
    ref = torch.tensor([[slab64(o[b, i].double(), d[b, i].double(), side) for i in range(R)] for b in range(B)], dtype=torch.float64)
    valid = ray_limits_valid(tn, tf)
    assert torch.equal(valid, ref[..., 1] > ref[..., 0])
    torch.testing.assert_close(tn.double(), ref[..., 0], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(tf.double(), ref[..., 1], rtol=1e-6, atol=1e-6)
    if name == "mixed":
        assert bool(valid.all()) and float((tf - tn).min()) > 0.3
        assert bool((tn == 0).any()) == (side == 2.0)           # origins inside the larger box start at the origin
    elif side == 1.0:
        assert torch.equal(valid, ~RL.MISS) and int((~valid).sum()) == 40


def test_ray_limits_box_closed_forms():
    from hfa_gp_amd.cam_utils import ray_limits_box, ray_limits_valid
    o = torch.tensor([[0.0, 0.0, 2.7],      # axis-parallel through the centre: [2.2, 3.2]
                      [0.1, -0.2, 0.3],     # origin inside: near clamped at 0, far = the exit
                      [0.5, 0.0, 2.0],      # axis-parallel ON the face x = 0.5: 0 * inf -> NaN -> empty
                      [0.5001, 0.0, 2.0],   # just outside that face, parallel to it: a miss
                      [0.0, 0.0, 2.7],      # pointing away
                      [0.0, 0.0, 2.0]])     # direction of length 2: the limits halve
    d = torch.tensor([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -2.0]])
    tn, tf = ray_limits_box(o, d, 1.0)
    valid = ray_limits_valid(tn, tf)
    assert valid.tolist() == [True, True, False, False, False, True]
    torch.testing.assert_close(tn[[0, 1, 5]], torch.tensor([2.2, 0.0, 0.75]), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(tf[[0, 1, 5]], torch.tensor([3.2, 0.4, 1.25]), rtol=1e-6, atol=1e-6)
    assert math.isnan(float(tn[2])) and math.isnan(float(tf[2]))
    assert float(tf[3]) < float(tn[3]) and float(tf[4]) < float(tn[4])
    assert not tn.requires_grad
    tn2, _ = ray_limits_box(o.clone().requires_grad_(True), d, 1.0)
    assert not tn2.requires_grad                  # the limits carry no gradient


def test_ray_grid_ortho_geometry():
    from hfa_gp_amd.cam_utils import create_cam2world_matrix, ray_grid_ortho
    pos = torch.tensor([[0.0, 0.0, 4.0], [2.0, 1.0, 3.0]])
    c2w = create_cam2world_matrix(pos, pos, device="cpu")         # (columns (-left, up, -forward): +z towards the centre)
    res, extent = 5, 1.2
    o, d = ray_grid_ortho(c2w, res, extent)
    assert o.shape == d.shape == (2, res * res, 3) and o.is_contiguous() and d.is_contiguous()
    for b in range(2):
        x, y, z, p = c2w[b, :3, 0], c2w[b, :3, 1], c2w[b, :3, 2], c2w[b, :3, 3]
        assert torch.equal(d[b], z.expand(res * res, 3))                 # parallel: the camera's +z ...
        torch.testing.assert_close(z, -pos[b] / pos[b].norm())           # ... which looks at the centre
        rel = o[b] - p
        torch.testing.assert_close(rel @ z, torch.zeros(res * res), atol=1e-6, rtol=0)        # origins in the camera's z = 0 plane
        px = ((torch.arange(res) + 0.5) / res - 0.5) * extent
        torch.testing.assert_close((rel @ x).reshape(res, res), px[None].expand(res, res), atol=1e-6, rtol=0)     # x along a row
        torch.testing.assert_close((rel @ y).reshape(res, res), px[:, None].expand(res, res), atol=1e-6, rtol=0)  # y down the rows
        torch.testing.assert_close(o[b].mean(0), p, atol=1e-6, rtol=0)
    # (16-float labels are taken as well, and the grid is differentiable w.r.t. the pose)
    c = c2w.reshape(2, 16).clone().requires_grad_(True)
    o2, d2 = ray_grid_ortho(c, res, extent)
    assert torch.equal(o2.detach(), o) and torch.equal(d2.detach(), d)
    (o2.sum() + d2.sum()).backward()
    assert c.grad is not None and bool(c.grad.abs().sum() > 0)


@pytest.mark.parametrize("rays", ["r27", "mixed"])
def test_reference_with_constant_limits_is_the_oracle(rays):
    """Limits filled with cfg.ray_start / ray_end: the restated coarse depths differ from torch.linspace + u * delta in the last
    bit only.  Measured: feat <= 6.0e-7, depth <= 9.6e-7; bar 5e-6."""
    from oracle import eg3d_oracle as O
    cs = RL.case("small128", rays=rays, limits="config")
    o, d = cs["od"]
    with torch.no_grad():
        feat, depth, wsum = O.importance_renderer(cs["P"], cs["cfg"], cs["planes"], o, d, cs["us"], cs["ui"])
    assert bool(cs["valid"].all())
    for got, want, name in zip(cs["out"], (feat, depth[..., 0], wsum[..., 0]), ("feat", "depth", "wsum")):
        err = float((got.detach() - want).abs().max())
        print(f"{rays}/{name}: max err {err:.3e}")
        assert err <= 5e-6, (rays, name, err)


def test_reference_empty_ray_semantics():
    cs = RL.case("tiny64", rays="miss")
    valid = cs["valid"]
    assert torch.equal(valid, ~RL.MISS)
    feat, depth, wsum = (t.detach() for t in cs["out"])
    assert bool((feat[~valid] == -1).all()) and bool((wsum[~valid] == 0).all())
    assert torch.isfinite(depth).all() and bool((depth[~valid] == depth.max()).all())
    # the valid rays are what the mixed list gives them (per-ray arithmetic; the depth is left out: its clamp range differs)
    mixed = RL.case("tiny64", rays="mixed")
    assert torch.equal(feat[valid], mixed["out"][0].detach()[valid]) and torch.equal(wsum[valid], mixed["out"][2].detach()[valid])
    # exactly zero gradient from and to an empty ray
    _, _, d_rays = RL.reference(cs, "all")
    assert bool((d_rays[~valid] == 0).all()) and bool((d_rays[valid] != 0).any())
    # white_back: the background is +1
    wb = RL.case("tiny64", rays="miss", white_back=True)
    assert bool((wb["out"][0].detach()[~valid] == 1).all())


def test_reference_all_empty_call():
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    from tests.util import perturb_state, state_cpu
    cfg = PRESETS["tiny64"]()
    P = state_cpu(perturb_state(TriPlaneGenerator(cfg, seed=0)))
    o, d = (t[:, :5] for t in RL.mixed_list())
    g = torch.Generator().manual_seed(1)
    planes = torch.randn(B, 3, 32, 20, 20, generator=g)
    us, ui = torch.rand(B, 5, cfg.depth_resolution, 1, generator=g), torch.rand(B * 5, cfg.depth_resolution_importance, generator=g)
    tn = torch.tensor([[1.0, NAN, 2.0, INF, 0.5]] * B)
    tf = torch.tensor([[1.0, 3.0, 1.0, INF, NAN]] * B)           # far == near, NaN, far < near, inf, NaN
    feat, depth, wsum, valid = RL.importance_renderer_limits(P, cfg, planes, o, d, us, ui, tn, tf)
    assert not bool(valid.any())
    assert bool((feat == -1).all()) and bool((wsum == 0).all()) and bool((depth == 0).all())


# ----------------------------------------------------------------------------- the C ABI's argument checks (nothing is launched)
@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _list_args(lib, a):
    f = a.base if isinstance(a, lib.RayListArgs) else a.bwd.fwd
    for name in ("planes", "u_strat", "u_imp", "dec_w0", "dec_b0", "dec_w1", "dec_b1", "feat", "depth", "wsum", "tminmax"):
        setattr(f, name, 1)               # non-null, never dereferenced: a check fails first
    f.B, f.H, f.W, f.Sc, f.Sf = 1, 64, 64, 24, 24
    f.box_warp = 1.0
    f.ray_start, f.ray_end = 3.0, 2.0     # NOT checked by the limits entry points
    a.ray_origins, a.ray_directions, a.R = 1, 1, 7
    return a


def test_limits_entry_points_check_their_arguments(lib):
    h = lib.lib()
    EBADARG, EUNSUPPORTED = -1, -2
    lim, bad = lib.RayLimits(), lib.RayLimits()
    lim.t_near, lim.t_far = 1, 1
    bad.t_near = 1
    assert h.hfagp_ray_limits_box(None, 1, 1, 1, 4, 1.0, None) == EBADARG and b"null pointer" in h.hfagp_last_error()
    assert h.hfagp_ray_limits_box(1, 1, 1, 1, 0, 1.0, None) == EBADARG and b"n_rays" in h.hfagp_last_error()
    assert h.hfagp_ray_limits_box(1, 1, 1, 1, 4, 0.0, None) == EBADARG and b"box_side" in h.hfagp_last_error()
    fa, ba = _list_args(lib, lib.RayListArgs()), _list_args(lib, lib.RayListBwdArgs())
    ba.bwd.d_planes = ba.bwd.rec = ba.bwd.g_feat = 1
    calls = {"fwd": lambda l: h.hfagp_raymarch_rays_limits_fwd(C.byref(fa), l, None),
             "bwd": lambda l: h.hfagp_raymarch_rays_limits_bwd(C.byref(ba), l, None, None),
             "bwd_rays": lambda l: h.hfagp_raymarch_rays_limits_bwd_rays(C.byref(ba), l, 1, 1, None)}
    for name, call in calls.items():
        assert call(None) == EBADARG and b"limits" in h.hfagp_last_error(), name
        assert call(C.byref(bad)) == EBADARG and b"limits" in h.hfagp_last_error(), name
        # ray_end < ray_start passes; the next check that fails is the sample count's
        assert call(C.byref(lim)) == EUNSUPPORTED and b"unsupported sample counts" in h.hfagp_last_error(), name
    # ... while the entry point without limits still refuses that range
    assert h.hfagp_raymarch_rays_fwd(C.byref(fa), None) == EBADARG and b"bad ray range" in h.hfagp_last_error()
    fa.R = 0
    assert calls["fwd"](C.byref(lim)) == EBADARG and b"R = 0" in h.hfagp_last_error()
    # the struct is two pointers
    assert C.sizeof(lib.RayLimits) == 16


# ----------------------------------------------------------------------------- compiled code
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _resources(unit, tmp_path):
    """{kernel: {figure: value}} and the ISA text of a unit compiled with build.sh's flags."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    asm = tmp_path / f"{unit}.s"
    out = subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", os.path.join(ROOT, "hfa-gp_amd", "csrc", f"{unit}.hip"),
                          "-o", str(asm), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|VGPRs|AGPRs|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return res, asm.read_text()


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_ray_limits_unit_resources(tmp_path):
    """ray_limits.hip is in build.sh's list and, compiled with its flags: one kernel without scratch, spill or LDS and none of the
    packed fp32 arithmetic build.sh keeps out of the library."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(.*\bray_limits\b", build, re.M), "ray_limits.hip is not in build.sh's unit list"
    res, text = _resources("ray_limits", tmp_path)
    assert len(res) == 1 and "ray_limits_box_kernel" in next(iter(res)), res
    r = next(iter(res.values()))
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["LDS Size [bytes/block]"] == 0, r
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_list_instantiations_of_the_ray_marcher_have_no_scratch(tmp_path):
    """The 15 list instantiations of raymarch_body — the only code that reads the limits — keep no scratch, spill no vector register
    and stay within 256 VGPRs (two workgroups per CU), as the grid instantiations do."""
    res, _ = _resources("raymarch", tmp_path)
    lists = {k: v for k, v in res.items() if "raymarch_rays_kernel" in k}
    grids = {k: v for k, v in res.items() if "raymarch_kernel" in k}
    assert len(lists) == 15 and len(grids) == 27, (len(lists), len(grids))
    for k, r in {**lists, **grids}.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 256, (k, r)
