"""The per-ray surface normals without a GPU: the reference of tests/normals_ref.py against central differences and against the
point-query reference, its invariants, `render.normal_map`, and the build / binding of hfagp_raymarch_normals (header, symbol
table, kernel resources, argument validation)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

from tests import normals_ref as N
from tests import query_ref as Q
from tests.util import ROOT, look_at_label

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F64 = torch.float64


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _query_cfg(axes):
    return types.SimpleNamespace(plane_axes=axes, box_warp=Q.BOX_WARP, decoder_lr_mul=Q.LR_MUL)


@pytest.mark.parametrize("axes", Q.AXES)
def test_sample_gradient_matches_central_differences(axes):
    """g = d sigma / d x of the reference at points kept off the texel edges (sigma is smooth inside a texel cell) against central
    differences of the oracle's sigma in float64; about a third of the points lie outside the box."""
    cs = Q.base_case()
    P = {k: v.double() for k, v in cs["P"].items()}
    planes, pts = cs["pn"].double(), cs["coords"].double()
    _, g, n = N.sample_normals(P, _query_cfg(axes), planes, pts)
    h = 1e-6                                      # 3.5e-5 pixels: far inside the 1e-3 margin of make_points
    fd = torch.zeros_like(g)
    for k in range(3):
        e = torch.zeros(3, dtype=F64)
        e[k] = h
        fd[..., k] = (Q.query_fp64(P, planes, pts + e, Q.BOX_WARP, axes, Q.LR_MUL)[1] -
                      Q.query_fp64(P, planes, pts - e, Q.BOX_WARP, axes, Q.LR_MUL)[1])[..., 0] / (2 * h)
    assert rel(g, fd) <= 1e-7, rel(g, fd)
    outside = g.abs().amax(-1) == 0
    assert bool(outside[:, :2].all()) and 0.05 < float(outside.double().mean()) < 0.6      # SPECIAL[0:2] lie outside every plane
    assert bool((n[outside] == 0).all())
    assert float(((n[~outside] ** 2).sum(-1) - 1).abs().max()) <= 1e-9                      # |g| >> 1e-6 there: unit length


@pytest.mark.parametrize("axes", Q.AXES)
def test_sample_gradient_matches_query_reference(axes):
    cs = Q.base_case()
    P = {k: v.double() for k, v in cs["P"].items()}
    _, g, _ = N.sample_normals(P, _query_cfg(axes), cs["pn"].double(), cs["coords"].double())
    ref = Q.reference(cs["P"], cs["pn"], cs["coords"], torch.ones(Q.B, Q.M, 1), None, Q.BOX_WARP, axes, Q.LR_MUL)["coords"]
    assert rel(g, ref) <= 1e-12, rel(g, ref)


@pytest.mark.parametrize("preset,axes,hw,box_warp", [N.CASES[0], N.CASES[3], N.CASES[6]], ids=["tiny64", "fixed-36x20", "40x72-0.45"])
def test_normal_norm_bounded_by_opacity(preset, axes, hw, box_warp):
    ref = N.case_reference(preset, axes, hw, box_warp)
    nrm = ref["normal"].norm(dim=-1)
    assert ref["normal"].shape == (2, 100, 3) and bool((nrm <= ref["wsum"] + 1e-12).all())
    assert float(nrm.max()) > 0.05, "the case renders no surface"


def test_camera_looking_away_gives_exact_zeros():
    cs = N.case("tiny64")
    c = cs["c"].clone()
    m = c[:, :16].view(-1, 4, 4)
    m[:, :3, 0] *= -1                             # half a turn about the camera's up axis: every ray leaves the box behind
    m[:, :3, 2] *= -1
    for dtype in (F64, torch.float32):
        out = N.reference(cs["P"], cs["cfg"], cs["planes"], c, cs["us"], cs["ui"], dtype=dtype)
        assert bool((out["g"] == 0).all()) and bool((out["normal"] == 0).all())


def test_normal_map_colours():
    from hfa_gp_amd import render
    n = torch.zeros(1, 3, 2, 2)
    n[0, :, 0, 0] = torch.tensor([0.0, 0.0, 0.3])          # +z, not unit length
    n[0, :, 0, 1] = torch.tensor([-2.0, 0.0, 0.0])         # -x
    n[0, :, 1, 0] = torch.tensor([0.0, 0.5, 0.0])          # +y; pixel (1, 1) stays 0
    img = render.normal_map(n)
    assert img.dtype == torch.uint8 and img.shape == (1, 3, 2, 2)
    assert img[0, :, 0, 0].tolist() == [128, 128, 255]
    assert img[0, :, 0, 1].tolist() == [0, 128, 128]
    assert img[0, :, 1, 0].tolist() == [128, 255, 128]
    assert img[0, :, 1, 1].tolist() == [128, 128, 128]
    mask = torch.tensor([1.0, 0.5, 0.0, 1.0]).view(1, 1, 2, 2)
    img = render.normal_map(n, mask=mask)
    assert img[0, :, 0, 0].tolist() == [128, 128, 255]
    assert img[0, :, 0, 1].tolist() == [64, 128, 128]      # -0.5 * 127.5 + 128 = 64.25
    assert img[0, :, 1, 0].tolist() == [128, 128, 128]


def test_normal_map_camera_rotation():
    """A normal along the camera's own axes (columns of the label's cam2world rotation) maps to the unit axes in camera space."""
    from hfa_gp_amd import render
    c = look_at_label(torch.tensor([1.3, 1.8]), torch.tensor([1.5, 1.7]))
    rot = c[:, :16].view(-1, 4, 4)[:, :3, :3]
    n = torch.zeros(2, 3, 1, 3)
    for k in range(3):
        n[:, :, 0, k] = 0.7 * rot[:, :, k]                 # world-space direction of camera axis k
    img = render.normal_map(n, c=c)
    for k in range(3):
        want = [128, 128, 128]
        want[k] = 255
        assert img[0, :, 0, k].tolist() == want and img[1, :, 0, k].tolist() == want
    world = render.normal_map(n)
    assert not torch.equal(world, img)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 4, 4, generator=g)
    unit = x / x.norm(dim=1, keepdim=True)
    want = render.to_uint8(torch.einsum("bji,bjhw->bihw", rot, unit))
    assert int((render.normal_map(x, c=c).int() - want.int()).abs().max()) <= 1


# ----------------------------------------------------------------------------- the fp32 oracle's own error on the GPU cases
@pytest.mark.parametrize("preset,axes,hw,box_warp", N.CASES, ids=N.CASE_IDS)
def test_fp32_oracle_edge_rays(preset, axes, hw, box_warp):
    """Edge-ray condition of tests/test_gpu_normals.py: the fp32 oracle against the float64 reference, each drawing its own fine
    depths, has at most 1 ray of 200 beyond the bar."""
    cs = N.case(preset, axes, hw, box_warp)
    ref = N.case_reference(preset, axes, hw, box_warp)
    got = N.reference(cs["P"], cs["cfg"], cs["planes"], cs["c"], cs["us"], cs["ui"], dtype=torch.float32)
    bad = N.rays_beyond(got["normal"], ref["normal"], f"{preset}/{axes}/{hw}/{box_warp}: fp32 oracle")
    assert bad <= N.MAX_EDGE_RAYS_ORACLE, bad


# ----------------------------------------------------------------------------- build and binding
@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_normals_entry_binding_matches_header(lib):
    raw = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    assert re.search(r"^ \*   hfagp_raymarch_normals\s+<-", raw, re.M), "hfagp_raymarch_normals is not in the header's entry list"
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int hfagp_raymarch_normals\(([^)]*)\);", text)
    assert m, "include/hfagp.h does not declare hfagp_raymarch_normals"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["fwd", "normal", "stream"]
    res, args = lib.SYMBOLS["hfagp_raymarch_normals"]
    assert res is C.c_int and len(args) == 3 and args[0] == C.POINTER(lib.RaymarchArgs)
    assert lib.ABI_VERSION == 15, "the export is additive: no struct changes layout"
    assert hasattr(lib.lib(), "hfagp_raymarch_normals")
    from hfa_gp_amd import ops
    assert callable(ops.raymarch_normals)


def test_normals_entry_argument_validation(lib):
    h = lib.lib()
    assert h.hfagp_raymarch_normals(None, 8, None) == -1
    assert b"raymarch_normals: null pointer" in h.hfagp_last_error()
    a = lib.RaymarchArgs()
    a.state, a.planes = 8, 8                   # non-null, never dereferenced: the arguments are checked first
    assert h.hfagp_raymarch_normals(C.byref(a), None, None) == -1          # normal
    assert b"raymarch_normals: null pointer" in h.hfagp_last_error()
    a.state = None
    assert h.hfagp_raymarch_normals(C.byref(a), 8, None) == -1             # state
    a.state, a.planes = 8, None
    assert h.hfagp_raymarch_normals(C.byref(a), 8, None) == -1             # planes
    assert b"raymarch_normals: null pointer" in h.hfagp_last_error()
    for f, _ in lib.RaymarchArgs._fields_[:9]:                             # every input pointer set: the sample counts are checked
        setattr(a, f, 8)
    a.B, a.H, a.W, a.res, a.box_warp, a.ray_start, a.ray_end = 1, 8, 8, 4, 1.0, 2.25, 3.3
    for sc, sf in ((48, 32), (24, 24), (64, 64)):
        a.Sc, a.Sf = sc, sf
        assert h.hfagp_raymarch_normals(C.byref(a), 8, None) == -2
        assert b"raymarch_normals: unsupported sample counts" in h.hfagp_last_error()


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_normals_unit_resources(tmp_path):
    """On its own `units+=` line of build.sh; compiled with build.sh's flags: every kernel of the unit without scratch and without
    spilled vector registers, all six instantiations present, and no packed fp32 arithmetic (build.sh's note) in its ISA."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(raymarch_normals\)$", build, re.M), "raymarch_normals.hip is not on its own units+= line of build.sh"
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    src = os.path.join(ROOT, "hfa-gp_amd", "csrc", "raymarch_normals.hip")
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
    rays = [n for n in seen if "raymarch_normals_kernel" in n]
    assert len(rays) == 6 and len(seen) == 6, seen       # S = 32 / 64 / 96 x {split 16-bit, fp32 decoder}
    for n, v in seen.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0}, (n, v)
    text = asm.read_text()
    assert "raymarch_normals_kernel" in text
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)
