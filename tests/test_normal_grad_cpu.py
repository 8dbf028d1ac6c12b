"""The gradient of the per-ray surface normals without a GPU: the reference of tests/normal_grad_ref.py pinned against the forward
reference (tests/normals_ref.py), the closed-form adjoint the kernel implements against autograd, the fp32 reference's own error
(rho: the figure the GPU tolerances scale with), and the build / binding of hfagp_raymarch_normals_bwd."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import normal_grad_ref as G
from tests import normals_ref as N
from tests.util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ONE_PER_S = [N.CASES[0], N.CASES[5], N.CASES[2]]          # 16+16, 32+32 (not square, box_warp 0.6), 48+48 samples
ONE_PER_S_IDS = [N.CASE_IDS[0], N.CASE_IDS[5], N.CASE_IDS[2]]
KEPT_MEASURED = (199, 193, 191, 189, 194, 191, 185)       # of 200, with the oracle's own importance depths


@pytest.mark.parametrize("preset,axes,hw,box_warp", N.CASES, ids=N.CASE_IDS)
def test_index_gather_reproduces_forward_reference(preset, axes, hw, box_warp):
    """The hand-written gather gives the N and g of normals_ref (grid_sample) to 1e-12 in float64 (measured: 2e-16 and 7e-14)."""
    cs, depths, g_hat, mask = G.masked_case(preset, axes, hw, box_warp)
    ref = N.case_reference(preset, axes, hw, box_warp)
    with torch.no_grad():
        feats = G.gather_from_planes(axes, cs["planes"].double(), torch.randn(2, 50, 3, dtype=torch.float64,
                                                                             generator=torch.Generator().manual_seed(1)) * 0.4,
                                     cs["cfg"].box_warp)
    assert feats.shape == (2, 3, 50, 32)
    got = G.reference(cs["P"], cs["cfg"], cs["planes"], cs["c"], depths, g_hat)
    d_n, d_g = float((got["normal"] - ref["normal"]).abs().max()), float((got["g"] - ref["g"]).abs().max())
    print(f"normal {d_n:.1e}, g {d_g:.1e}; {int(mask.sum())} of {mask.numel()} rays kept")
    assert d_n <= 1e-12 and d_g <= 1e-12
    assert int(mask.sum()) == KEPT_MEASURED[N.CASES.index((preset, axes, hw, box_warp))]


def test_index_gather_equals_grid_sample():
    from oracle import eg3d_oracle as O
    g = torch.Generator().manual_seed(3)
    planes = torch.randn(2, 3, 32, 9, 13, generator=g, dtype=torch.float64)
    pts = (torch.rand(2, 400, 3, generator=g, dtype=torch.float64) - 0.5) * 1.4          # some outside the box
    for axes in ("eg3d_original", "eg3d_fixed"):
        want = O.sample_from_planes(O.plane_axes(axes), planes, pts, 1.0)
        assert float((G.gather_from_planes(axes, planes, pts, 1.0) - want).abs().max()) <= 1e-13


@pytest.mark.parametrize("preset,axes,hw,box_warp", ONE_PER_S, ids=ONE_PER_S_IDS)
def test_closed_form_adjoint_equals_autograd(preset, axes, hw, box_warp):
    """The formulas of include/hfagp.h (what the kernel computes), written out in float64, against autograd: 1e-10 relative on the
    planes and on all four decoder tensors."""
    cs, depths, g_hat, _ = G.masked_case(preset, axes, hw, box_warp)
    ref = G.reference(cs["P"], cs["cfg"], cs["planes"], cs["c"], depths, g_hat)
    got = G.closed_form(cs["P"], cs["cfg"], cs["planes"], cs["c"], depths, g_hat)
    assert float((got["normal"] - ref["normal"]).abs().max()) <= 1e-12
    for k, a, b in zip(("planes",) + G.DEC_KEYS, (got["planes"],) + got["dec"], (ref["planes"],) + ref["dec"]):
        rel = float((a - b).abs().max() / b.abs().max())
        print(f"{k}: {rel:.2e} relative, max |ref| {float(b.abs().max()):.3e}")
        assert float(b.abs().max()) > 1e-3 and rel <= 1e-10, (k, rel)
    assert bool((ref["dec"][2][1:] == 0).all()) and bool((ref["dec"][3][1:] == 0).all()), "the colour rows get nothing"


def test_closed_form_camera_looking_away_gives_exact_zeros():
    cs, depths, g_hat, _ = G.masked_case(*N.CASES[0])
    c = cs["c"].clone()
    m = c[:, :16].view(-1, 4, 4)
    m[:, :3, 0] *= -1                             # half a turn about the camera's up axis: every ray leaves the box behind
    m[:, :3, 2] *= -1
    for fn in (G.reference, G.closed_form):
        out = fn(cs["P"], cs["cfg"], cs["planes"], c, depths, G.upstream(cs))
        assert bool((out["planes"] == 0).all()) and all(bool((t == 0).all()) for t in out["dec"])


@pytest.mark.parametrize("preset,axes,hw,box_warp", N.CASES, ids=N.CASE_IDS)
def test_fp32_reference_rho(preset, axes, hw, box_warp):
    """rho: the fp32 reference against the float64 one under the edge mask, the worst err / bar over d_planes and the decoder
    gradients.  Printed; the GPU tests recompute it and scale their tolerance by max(1, 4 rho).  Measured with G^ of
    normal_grad_ref.upstream: 0.39, 0.38, 0.25, 0.14, 0.22, 4.50, 1.10 in the order of CASES (the two box_warp cases lead, from
    the decoder.net.2.weight gradient; d_planes alone: at most 1.25)."""
    rho = G.oracle_rho(preset, axes, hw, box_warp)
    assert 0.0 < rho < float("inf")


# ----------------------------------------------------------------------------- build and binding
@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_entry_binding_matches_header(lib):
    raw = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    assert re.search(r"^ \*   hfagp_raymarch_normals_bwd\s+<-", raw, re.M), "hfagp_raymarch_normals_bwd is not in the header's entry list"
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int hfagp_raymarch_normals_bwd\(([^)]*)\);", text)
    assert m, "include/hfagp.h does not declare hfagp_raymarch_normals_bwd"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["fwd", "g_normal", "d_planes", "d_dec_w0", "d_dec_b0", "d_dec_w1", "d_dec_b1",
                                                           "stream"]
    res, args = lib.SYMBOLS["hfagp_raymarch_normals_bwd"]
    assert res is C.c_int and len(args) == 8 and args[0] == C.POINTER(lib.RaymarchArgs) and all(a is C.c_void_p for a in args[1:])
    assert lib.ABI_VERSION == 15 and lib.lib().hfagp_abi_version() == 15, "the export is additive: no struct changes layout"
    assert hasattr(lib.lib(), "hfagp_raymarch_normals_bwd")
    from hfa_gp_amd import ops
    assert callable(ops.raymarch_normals_bwd)


def test_entry_argument_validation(lib):
    h = lib.lib()
    fn = h.hfagp_raymarch_normals_bwd
    assert fn(None, 8, 8, None, None, None, None, None) == -1
    assert b"raymarch_normals_bwd: null pointer" in h.hfagp_last_error()
    a = lib.RaymarchArgs()
    a.state, a.planes = 8, 8                   # non-null, never dereferenced: the arguments are checked first
    assert fn(C.byref(a), None, 8, None, None, None, None, None) == -1           # g_normal
    assert fn(C.byref(a), 8, None, None, None, None, None, None) == -1           # d_planes
    assert b"raymarch_normals_bwd: null pointer" in h.hfagp_last_error()
    a.state = None
    assert fn(C.byref(a), 8, 8, None, None, None, None, None) == -1              # state
    a.state, a.planes = 8, None
    assert fn(C.byref(a), 8, 8, None, None, None, None, None) == -1              # planes
    assert b"raymarch_normals_bwd: null pointer" in h.hfagp_last_error()
    a.planes = 8
    for some in ((8, None, None, None), (8, 8, 8, None), (None, None, None, 8)):   # only some of the four decoder outputs
        assert fn(C.byref(a), 8, 8, *some, None) == -1
        assert b"the four decoder gradients go together" in h.hfagp_last_error()
    for f, _ in lib.RaymarchArgs._fields_[:9]:                             # every input pointer set: the sample counts are checked
        setattr(a, f, 8)
    a.B, a.H, a.W, a.res, a.box_warp, a.ray_start, a.ray_end = 1, 8, 8, 4, 1.0, 2.25, 3.3
    for sc, sf in ((48, 32), (24, 24), (64, 64)):
        a.Sc, a.Sf = sc, sf
        assert fn(C.byref(a), 8, 8, None, None, None, None, None) == -2
        assert b"raymarch_normals_bwd: unsupported sample counts" in h.hfagp_last_error()
        assert fn(C.byref(a), 8, 8, 8, 8, 8, 8, None) == -2


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_unit_resources(tmp_path):
    """On its own `units+=` line of build.sh; compiled with build.sh's flags: every kernel of the unit without scratch and without
    spilled vector registers, all twelve instantiations present, and no packed fp32 arithmetic (build.sh's note) in its ISA."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(raymarch_normals_bwd\)$", build, re.M), "raymarch_normals_bwd.hip is not on its own units+= line"
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    src = os.path.join(ROOT, "hfa-gp_amd", "csrc", "raymarch_normals_bwd.hip")
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
    rays = [n for n in seen if "raymarch_normals_bwd_kernel" in n]
    assert len(rays) == 12 and len(seen) == 12, seen     # S = 32 / 64 / 96 x {split 16-bit, fp32 decoder} x {with, without PG}
    for n, v in seen.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0}, (n, v)
    text = asm.read_text()
    assert "raymarch_normals_bwd_kernel" in text
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)
