"""The camera gradient of the ray marcher without a GPU: the closed forms of tests/camera_ref.py (what
csrc/raymarch_camera.hip computes) against autograd through the oracle in float64, and the build / binding of
hfagp_raymarch_bwd_camera (header, symbol table, kernel resources, argument validation)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import camera_ref as R
from tests.util import ROOT, look_at_label

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F64 = torch.float64


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("box_warp", [0.45, 0.6, 1.0])
@pytest.mark.parametrize("hw", [(20, 36), (24, 24), (36, 20)])
@pytest.mark.parametrize("axes", ["eg3d_original", "eg3d_fixed"])
def test_position_grad_matches_oracle_autograd(axes, hw, box_warp):
    """d <g, mean_planes grid_sample(planes, proj(2 p / box_warp))> / dp; about a third of the points lie outside the box
    (every coordinate uniform in +-1.145 half boxes: (1 / 1.145)^3 = 2 / 3 inside), where taps fall off the planes."""
    from oracle import eg3d_oracle as O
    gen = torch.Generator().manual_seed(7)
    n, m, c = 2, 400, 8
    h, w = hw
    planes = torch.randn(n, 3, c, h, w, generator=gen, dtype=F64)
    coords = ((torch.rand(n, m, 3, generator=gen, dtype=F64) * 2 - 1) * 1.145 * box_warp / 2).requires_grad_(True)
    g = torch.randn(n, m, c, generator=gen, dtype=F64)
    outside = ((2 / box_warp) * coords.detach()).abs().amax(-1) > 1
    assert 0.2 < float(outside.double().mean()) < 0.45
    feats = O.sample_from_planes(O.plane_axes(axes), planes, coords, box_warp).mean(1)
    ref, = torch.autograd.grad((feats * g).sum(), coords)
    got = R.gather_position_grad(planes, coords.detach(), g, axes, box_warp)
    assert bool(ref[outside].any()) and bool(ref[~outside].any())
    assert rel(got, ref) <= 1e-10, rel(got, ref)


def skewed_label(dtype=F64):
    c = look_at_label(torch.tensor([1.3, 1.8]), torch.tensor([1.5, 1.7])).to(dtype)
    c[:, 17] = torch.tensor([0.07, -0.11], dtype=dtype)       # skew
    c[:, 18] = torch.tensor([0.47, 0.52], dtype=dtype)        # cx
    c[:, 21] = torch.tensor([0.55, 0.44], dtype=dtype)        # cy
    c[:, 16] = torch.tensor([4.1, 4.4], dtype=dtype)          # fx != fy
    return c


@pytest.mark.parametrize("res", [10, 7])
def test_ray_setup_adjoint_matches_oracle_autograd(res):
    from oracle import eg3d_oracle as O
    c = skewed_label().requires_grad_(True)
    o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:].reshape(-1, 3, 3), res)
    rg = torch.randn(2, res * res, 6, generator=torch.Generator().manual_seed(3), dtype=F64)
    ref, = torch.autograd.grad((o * rg[..., :3]).sum() + (d * rg[..., 3:]).sum(), c)
    got = R.ray_setup_adjoint(c.detach(), res, rg)
    assert rel(got, ref) <= 1e-10, rel(got, ref)
    zero = [k for k in range(25) if k not in R.NONZERO_COLUMNS]
    assert not bool(got[:, zero].any()) and not bool(ref[:, zero].any())
    assert bool((ref[:, R.NONZERO_COLUMNS] != 0).all())


def test_composed_reference_matches_oracle_autograd(monkeypatch):
    """Positional derivative per sample -> sums along the ray -> ray_setup adjoint, on the inputs of
    test_gpu_geometry_grad.case("small128") with all three upstream gradients, against c.grad of the oracle's renderer (float64).
    The per-sample points and dL/dF are taken from the oracle's own graph at its two sample_from_planes calls."""
    from oracle import eg3d_oracle as O
    from tests.test_gpu_geometry_grad import case
    cs = case("small128")
    cfg = cs["cfg"]
    P = {k: (v.detach().double() if v.is_floating_point() else v) for k, v in cs["P"].items()}
    planes = cs["planes"].detach().double()
    c = cs["c"].double().requires_grad_(True)
    res = cfg.neural_rendering_resolution
    o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:].reshape(-1, 3, 3), res)
    calls = []
    inner = O.sample_from_planes

    def recording(axes, pl, xyz, box_warp):
        out = inner(axes, pl, xyz, box_warp)
        out.retain_grad()
        calls.append((xyz, out))
        return out

    monkeypatch.setattr(O, "sample_from_planes", recording)
    feat, depth, wsum = O.importance_renderer(P, cfg, planes, o, d, cs["us"].double(), cs["ui"].double())
    ups = cs["ups"]
    loss = (feat * ups["g_feat"].double()).sum() + (depth[..., 0] * ups["g_depth"].double()).sum() + \
        (wsum[..., 0] * ups["g_wsum"].double()).sum()
    loss.backward()
    assert len(calls) == 2
    b, r = cs["b"], cs["r"]
    ray_grad = torch.zeros(b, r, 6, dtype=F64)
    for xyz, feats in calls:
        g = feats.grad.sum(1)                    # the mean hands each plane g / 3
        dp = R.gather_position_grad(planes, xyz.detach(), g, cfg.plane_axes, cfg.box_warp).reshape(b, r, -1, 3)
        pts = xyz.detach().reshape(b, r, -1, 3)
        t = ((pts - o.detach()[:, :, None]) * d.detach()[:, :, None]).sum(-1)        # |d| = 1
        ray_grad += R.ray_sums(dp, t)
    got = R.ray_setup_adjoint(c.detach(), res, ray_grad)
    assert rel(got, c.grad) <= 1e-9, rel(got, c.grad)


# ----------------------------------------------------------------------------- build and binding
@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_camera_entry_binding_matches_header(lib):
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int hfagp_raymarch_bwd_camera\(([^)]*)\);", text)
    assert m, "include/hfagp.h does not declare hfagp_raymarch_bwd_camera"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["a", "ray_grad", "d_cam2world", "d_intrinsics", "stream"]
    res, args = lib.SYMBOLS["hfagp_raymarch_bwd_camera"]
    assert res is C.c_int and len(args) == 5 and args[0] == C.POINTER(lib.RaymarchBwdArgs)
    assert lib.ABI_VERSION == 15, "the export is additive: no struct changes layout"
    assert hasattr(lib.lib(), "hfagp_raymarch_bwd_camera")


def test_camera_entry_argument_validation(lib):
    h = lib.lib()
    assert h.hfagp_raymarch_bwd_camera(None, 8, None, None, None) == -1
    assert b"raymarch_bwd_camera: null pointer" in h.hfagp_last_error()
    a = lib.RaymarchBwdArgs()
    assert h.hfagp_raymarch_bwd_camera(C.byref(a), 8, None, None, None) == -1          # rec
    assert b"raymarch_bwd_camera: null pointer" in h.hfagp_last_error()
    a.rec = 8                                  # non-null, never dereferenced: the arguments are checked first
    assert h.hfagp_raymarch_bwd_camera(C.byref(a), None, None, None, None) == -1       # ray_grad
    assert b"raymarch_bwd_camera: null pointer" in h.hfagp_last_error()
    for c2w, intr in ((8, None), (None, 8)):
        assert h.hfagp_raymarch_bwd_camera(C.byref(a), 8, c2w, intr, None) == -1
        assert b"d_cam2world and d_intrinsics go together" in h.hfagp_last_error()
    assert h.hfagp_raymarch_bwd_camera(C.byref(a), 8, None, None, None) == -1          # the forward arguments are checked next
    assert b"raymarch_bwd_camera: null pointer" in h.hfagp_last_error()


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_camera_unit_resources(tmp_path):
    """Compiled with build.sh's flags: every kernel of the unit without scratch and without spilled vector registers, all six
    ray instantiations present, and no packed fp32 arithmetic (build.sh's note) in its ISA."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(.*\braymarch_camera\b", build, re.M), "raymarch_camera.hip is not in build.sh's unit list"
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    src = os.path.join(ROOT, "hfa-gp_amd", "csrc", "raymarch_camera.hip")
    asm = tmp_path / "unit.s"
    out = subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", src, "-o", str(asm), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            seen.setdefault(name, {})[m.group(1)] = int(m.group(2))
    rays = [n for n in seen if "raymarch_bwd_camera_kernel" in n]
    assert len(rays) == 6, rays                  # S = 32 / 64 / 96 x {split fp16, fp32 decoder}
    assert any("camera_reduce_kernel" in n for n in seen)
    for n, v in seen.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0}, (n, v)
    text = asm.read_text()
    assert "raymarch_bwd_camera_kernel" in text and "camera_reduce_kernel" in text
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)
