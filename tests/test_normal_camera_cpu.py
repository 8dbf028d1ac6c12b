"""The camera gradient of the per-ray surface normals without a GPU: the closed form the kernel implements (tests/normal_camera_ref.py,
include/hfagp.h) against float64 autograd on all seven cases, and the build / binding of hfagp_raymarch_normals_bwd_camera."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import camera_ref as CR
from tests import normal_camera_ref as NC
from tests import normal_grad_ref as G
from tests import normals_ref as N
from tests.util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("preset,axes,hw,box_warp", N.CASES, ids=N.CASE_IDS)
def test_closed_form_equals_autograd(preset, axes, hw, box_warp):
    """dL/dx and dL/dc of the formulas within 1e-9 of max |ref| of float64 autograd (measured: at most 5e-14); the label slots that
    carry no gradient exactly 0; every other slot well away from 0 somewhere in the batch."""
    cs, depths, g_hat, mask = G.masked_case(preset, axes, hw, box_warp)
    dc, dx = NC.reference(cs["P"], cs["cfg"], cs["planes"], cs["c"], depths, g_hat)
    dc2, dx2, ray_grad = NC.closed_form(cs["P"], cs["cfg"], cs["planes"], cs["c"], depths, g_hat, parts=True)
    rel_x = float((dx2 - dx).abs().max() / dx.abs().max())
    rel_c = float((dc2 - dc).abs().max() / dc.abs().max())
    print(f"d x {rel_x:.2e}, d c {rel_c:.2e} relative; max |d c| {float(dc.abs().max()):.3e}; {int(mask.sum())} of {mask.numel()} rays kept")
    assert rel_x <= 1e-9 and rel_c <= 1e-9
    assert bool((dc[:, NC.ZERO_COLUMNS] == 0).all()) and bool((dc2[:, NC.ZERO_COLUMNS] == 0).all())
    assert float(dc[:, CR.NONZERO_COLUMNS].abs().max(0).values.min()) > 1e-3
    assert float((ray_grad - NC.ray_records(dx, depths)).abs().max()) <= 1e-9 * float(ray_grad.abs().max())


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
    assert re.search(r"^ \*   hfagp_raymarch_normals_bwd_camera\s+<-", raw, re.M), "not in the header's entry list"
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int hfagp_raymarch_normals_bwd_camera\(([^)]*)\);", text)
    assert m, "include/hfagp.h does not declare hfagp_raymarch_normals_bwd_camera"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["fwd", "g_normal", "ray_grad", "accumulate", "d_cam2world", "d_intrinsics",
                                                           "stream"]
    assert "hfagp_raymarch_normals_bwd_camera" in lib.SYMBOLS
    res, args = lib.SYMBOLS["hfagp_raymarch_normals_bwd_camera"]
    assert res is C.c_int and len(args) == 7 and args[0] == C.POINTER(lib.RaymarchArgs) and args[3] is C.c_int
    assert lib.ABI_VERSION == 15 and lib.lib().hfagp_abi_version() == 15, "the export is additive: no struct changes layout"
    assert hasattr(lib.lib(), "hfagp_raymarch_normals_bwd_camera")
    from hfa_gp_amd import ops
    assert callable(ops.raymarch_normals_bwd_camera)
    assert "not implemented" not in re.search(r"/\* Camera gradient of hfagp_raymarch_normals.*?\*/", raw, re.S).group(0)


def test_entry_argument_validation(lib):
    """NULL arguments and a lone d_cam2world / d_intrinsics return -1 before anything is launched (no GPU is touched)."""
    h = lib.lib()
    fn = h.hfagp_raymarch_normals_bwd_camera
    assert fn(None, 8, 8, 0, None, None, None) == -1
    assert b"raymarch_normals_bwd_camera: null pointer" in h.hfagp_last_error()
    a = lib.RaymarchArgs()
    a.state, a.planes = 8, 8                   # non-null, never dereferenced: the arguments are checked first
    assert fn(C.byref(a), None, 8, 0, None, None, None) == -1                    # g_normal
    assert b"raymarch_normals_bwd_camera: null pointer" in h.hfagp_last_error()
    assert fn(C.byref(a), 8, None, 1, None, None, None) == -1                    # ray_grad
    a.state = None
    assert fn(C.byref(a), 8, 8, 0, None, None, None) == -1                       # state
    a.state, a.planes = 8, None
    assert fn(C.byref(a), 8, 8, 0, None, None, None) == -1                       # planes
    assert b"raymarch_normals_bwd_camera: null pointer" in h.hfagp_last_error()
    a.planes = 8
    for pair in ((8, None), (None, 8)):
        assert fn(C.byref(a), 8, 8, 0, *pair, None) == -1
        assert b"d_cam2world and d_intrinsics go together" in h.hfagp_last_error()
    assert fn(C.byref(a), 8, 8, 0, None, None, None) == -1                       # the forward's own checks: its inputs are NULL
    assert b"raymarch_normals_bwd_camera: null pointer" in h.hfagp_last_error()
    for f, _ in lib.RaymarchArgs._fields_[:9]:                             # every input pointer set: the sample counts are checked
        setattr(a, f, 8)
    a.B, a.H, a.W, a.res, a.box_warp, a.ray_start, a.ray_end = 1, 8, 8, 4, 1.0, 2.25, 3.3
    for sc, sf in ((48, 32), (24, 24), (64, 64)):
        a.Sc, a.Sf = sc, sf
        assert fn(C.byref(a), 8, 8, 0, None, None, None) == -2
        assert b"raymarch_normals_bwd_camera: unsupported sample counts" in h.hfagp_last_error()
        assert fn(C.byref(a), 8, 8, 1, 8, 8, None) == -2


def test_shared_code_is_in_one_header():
    """The compositing of the two normal backward kernels is defined once (raymarch_normals_common.h), and the cross term sits
    next to gather_position_grad (fused with it: one read of the texels); the sibling names the twin of every block it keeps inline."""
    csrc = os.path.join(ROOT, "hfa-gp_amd", "csrc")
    for unit in ("raymarch_normals_bwd.hip", "raymarch_normals_camera.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "raymarch_normals_common.h"' in text and "struct Composite" not in text, unit
    assert open(os.path.join(csrc, "raymarch_normals_common.h")).read().count("struct Composite") == 1
    sib = open(os.path.join(csrc, "raymarch_normals_bwd.hip")).read()
    for twin in ("normals_load_ray", "normals_pass_a", "normals_weight_adjoint", "normals_gamma_q", "normals_second_taps"):
        assert f"twin: {twin}" in sib, twin
    adj = open(os.path.join(csrc, "decoder_adjoint.h")).read()
    assert adj.index("void gather_position_grad(") < adj.index("void gather_position_cross_grad(")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_unit_resources(tmp_path):
    """On its own `units+=` line of build.sh; compiled with build.sh's flags: every kernel of the unit without scratch and without
    spilled vector registers, all six instantiations present, and no packed fp32 arithmetic (build.sh's note) in its ISA."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(raymarch_normals_camera\)$", build, re.M), "raymarch_normals_camera.hip is not on its own units+= line"
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    src = os.path.join(ROOT, "hfa-gp_amd", "csrc", "raymarch_normals_camera.hip")
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
    assert len(seen) == 6 and all("raymarch_normals_camera_kernel" in n for n in seen), seen     # S = 32 / 64 / 96 x two decoders
    for n, v in seen.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0}, (n, v)
    text = asm.read_text()
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)
