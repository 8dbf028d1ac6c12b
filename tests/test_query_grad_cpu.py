"""Backward of the tri-plane point query without a GPU: the float64 reference the GPU tests compare against (tests/query_ref.py)
agrees with central differences; the C ABI addition (struct image, export, argument checks); the build-time resources of
csrc/planes_query_bwd.hip (no scratch, no spills, no packed fp32 arithmetic); the Python surface that must not change."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import query_ref as Q
from tests.util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "hfa-gp_amd", "csrc")


# ----------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("axes", Q.AXES)
def test_reference_matches_central_differences(axes):
    """6 x 10 planes, B = 2, 9 points (inside, straddling the border, outside): every coordinate gradient and a sample of the
    plane and decoder gradients against  (L(x + e) - L(x - e)) / 2e  in float64."""
    g = torch.Generator().manual_seed(3)
    b, h, w, m, box_warp, lr_mul = 2, 6, 10, 9, 0.8, 0.5
    P = {k: v.double() for k, v in Q.decoder(g, lr_mul).items()}
    pn = torch.randn(b, 3, 32, h, w, generator=g).double()
    coords = Q.make_points(g, b, m, box_warp, h, w, special=False, spread=2.2).double()
    coords[:, 0] = torch.tensor([0.39, -0.395, 0.1], dtype=torch.float64)    # last texel row / first column: one tap row outside
    assert not Q.near_edge(coords, box_warp, h, w).any()
    gs, gr = torch.randn(b, m, 1, generator=g).double(), torch.randn(b, m, 32, generator=g).double()
    ref = Q.reference(P, pn, coords, gs, gr, box_warp, axes, lr_mul)

    def loss(P_, pn_, co_):
        rgb, sigma = Q.query_fp64(P_, pn_, co_, box_warp, axes, lr_mul)
        return float((sigma * gs).sum() + (rgb * gr).sum())

    def central(t, idx, eps):
        keep = t[idx].item()
        t[idx] = keep + eps
        up = loss(P, pn, coords)
        t[idx] = keep - eps
        dn = loss(P, pn, coords)
        t[idx] = keep
        return (up - dn) / (2 * eps)

    # a step of 1e-6 in world units is 1e-5 of a texel: every point stays inside its bilinear cell (EDGE = 1e-3)
    for bi in range(b):
        for mi in range(m):
            for k in range(3):
                want = central(coords, (bi, mi, k), 1e-6)
                got = ref["coords"][bi, mi, k].item()
                assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (bi, mi, k, got, want)
    assert ref["coords"].abs().max() > 0
    nz = ref["planes"].nonzero()
    for idx in nz[torch.randperm(len(nz), generator=g)[:12]].tolist():
        want = central(pn, tuple(idx), 1e-5)
        assert abs(ref["planes"][tuple(idx)].item() - want) <= 1e-7 * max(1.0, abs(want)), idx
    for key, dref in zip(Q.DEC_KEYS, ref["dec"]):
        flat = torch.randperm(dref.numel(), generator=g)[:4].tolist() + ([0] if key.startswith("decoder.net.2") else [])
        for f in flat:
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(f), dref.shape))
            want = central(P[key], idx, 1e-6)
            assert abs(dref[idx].item() - want) <= 1e-6 * max(1.0, abs(want)), (key, idx)


def test_broadcast_reference_is_the_sum_over_identities():
    full = Q.base_case()
    one = Q.reference(full["P"], full["pn"], full["coords"][:1], full["ups"]["g_sigma"], None, Q.BOX_WARP, "eg3d_original", Q.LR_MUL)
    both = Q.reference(full["P"], full["pn"], full["coords"][:1].expand(Q.B, -1, -1).contiguous(), full["ups"]["g_sigma"], None,
                       Q.BOX_WARP, "eg3d_original", Q.LR_MUL)
    assert one["coords"].shape == (1, Q.M, 3)
    assert torch.allclose(one["coords"], both["coords"].sum(0, keepdim=True), rtol=1e-12, atol=1e-12)


def test_points_keep_clear_of_texel_edges():
    coords = Q.base_case()["coords"]
    assert coords.shape == (Q.B, Q.M, 3) and coords.dtype == torch.float32
    assert not Q.near_edge(coords, Q.BOX_WARP, Q.H, Q.W).any()
    assert torch.equal(coords[0, :7], torch.tensor(Q.SPECIAL) * Q.BOX_WARP)
    px = Q.pixel_coords(coords, Q.BOX_WARP, "eg3d_original", Q.H, Q.W)
    inside = ((px[..., 0] > -1) & (px[..., 0] < Q.W) & (px[..., 1] > -1) & (px[..., 1] < Q.H)).all(-1)
    assert 0.2 < 1.0 - inside.float().mean() < 0.8          # both populations are there


# ----------------------------------------------------------------------------- C ABI
def test_planes_query_bwd_binding_matches_header():
    """The ctypes image of HfagpPlanesQueryBwdArgs has the header's field order (a reordering would not fail to load)."""
    from hfa_gp_amd import _lib
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} HfagpPlanesQueryBwdArgs;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\w+", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.PlanesQueryBwdArgs._fields_]
    kinds = {"float": C.c_float, "double": C.c_double, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for decl in body.split(";"):
        if decl.strip():
            want = C.c_void_p if "*" in decl else kinds[re.findall(r"\w+", decl)[0]]
            for part in decl.split(","):
                assert dict(_lib.PlanesQueryBwdArgs._fields_)[re.findall(r"\w+", part)[-1]] is want, decl
    assert _lib.ABI_VERSION == 15
    assert "#define HFAGP_ABI_VERSION 15" in text
    assert re.search(r"backward \(.*hfagp_planes_query_bwd", text, re.S), "not in the header's list under 'backward'"


def test_planes_query_bwd_is_exported_and_checks_its_arguments():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.lib()
    assert h.hfagp_abi_version() == 15
    assert h.hfagp_planes_query_bwd(None, None) == -1
    assert b"null pointer" in h.hfagp_last_error()
    a = _lib.PlanesQueryBwdArgs()
    for f in ("planes", "dec_w0", "dec_b0", "dec_w1", "dec_b1"):
        setattr(a, f, 1)                      # non-null, never dereferenced: the checks reject the call first
    a.g_sigma, a.d_planes = 1, 1
    a.B, a.H, a.W, a.Bc, a.M, a.box_warp = 2, 8, 8, 2, 5, 1.0
    assert h.hfagp_planes_query_bwd(C.byref(a), None) == -2             # no coords = grid mode: no backward
    assert b"grid mode" in h.hfagp_last_error()
    a.coords = 1
    a.g_sigma = None
    assert h.hfagp_planes_query_bwd(C.byref(a), None) == -1             # no upstream gradient
    a.g_rgb, a.d_planes = 1, None
    assert h.hfagp_planes_query_bwd(C.byref(a), None) == -1             # no output
    a.d_coords, a.d_dec_w0 = 1, 1
    assert h.hfagp_planes_query_bwd(C.byref(a), None) == -1             # the decoder gradients go together
    assert b"together" in h.hfagp_last_error()
    a.d_dec_w0 = None
    a.Bc = 3
    assert h.hfagp_planes_query_bwd(C.byref(a), None) == -1 and b"Bc=3" in h.hfagp_last_error()
    a.Bc, a.H, a.W = 1, 8192, 8192
    assert h.hfagp_planes_query_bwd(C.byref(a), None) == -2 and b"2^25" in h.hfagp_last_error()
    a.H, a.W, a.M = 8, 8, 0
    assert h.hfagp_planes_query_bwd(C.byref(a), None) == -1
    a.M, a.box_warp = 5, 0.0
    assert h.hfagp_planes_query_bwd(C.byref(a), None) == -1 and b"box_warp" in h.hfagp_last_error()


# ----------------------------------------------------------------------------- build-time resources
def _flags_and_units():
    build = open(os.path.join(CSRC, "build.sh")).read()
    return re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split(), re.findall(r"^units\+=\((\w+)\)", build, re.M)


def test_unit_is_appended_to_the_build():
    _, units = _flags_and_units()
    assert "planes_query_bwd" in units and "planes_query" in units
    both = open(os.path.join(CSRC, "planes_query_common.h")).read()
    assert "scale_rn" in both
    for unit in ("planes_query", "planes_query_bwd"):          # one definition of the point normalisation, used by both units
        src = open(os.path.join(CSRC, unit + ".hip")).read()
        assert '#include "planes_query_common.h"' in src and not re.search(r"float\s+scale_rn\s*\(", src), unit


def test_decoder_adjoint_has_a_single_source():
    """The pieces of the decoder adjoint that the ray-march backward, camera, point-query and normals kernels share are each
    defined once, in decoder_adjoint.h; no unit carries its own fp32 adjoint loop or its own operand-image struct."""
    pieces = ("decoder_images_lds", "build_grad_lds", "build_grad16_lds", "gather8_mfma", "colour_logit_grad", "decoder_bwd_lds",
              "decoder_bwd16_lds", "dec_grad_zero", "dec_grad_tile", "dec_grad_flush", "publish_taps", "scatter_tile_runs",
              "gather_position_grad")
    structs = ("GradLds", "DecGrads", "DecGradAcc", "TileLds")
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hip")))
    text = {f: open(os.path.join(CSRC, f)).read() for f in files}
    for name in pieces:          # a definition: `void name(` at the start of a declarator (calls have no return type before them)
        where = [f for f in files for _ in re.finditer(r"\bvoid\s+%s\s*\(" % name, text[f])]
        assert where == ["decoder_adjoint.h"], (name, where)
    for name in structs:
        where = [f for f in files for _ in re.finditer(r"\bstruct\s+%s\b\s*\{" % name, text[f])]
        assert where == ["decoder_adjoint.h"], (name, where)
    for f in files:
        if f.endswith(".hip"):
            assert not re.search(r"\bstruct\s+\w*GradLds\b", text[f]), f
            assert "mfma_f32_16x16x4f32(wA" not in text[f], f
    for unit in ("raymarch_bwd", "raymarch_camera", "planes_query_bwd", "raymarch_normals"):
        assert '#include "decoder_adjoint.h"' in text[unit + ".hip"], unit


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_every_instance_compiles_without_scratch_spills_or_packed_fp32(tmp_path):
    flags, _ = _flags_and_units()
    asm = tmp_path / "unit.s"
    out = subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "planes_query_bwd.hip"), "-o", str(asm),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name and "planes_query_bwd_kernel" in name:
            seen.setdefault(name, {})[m.group(1)] = int(m.group(2))
    assert len(seen) == 8, sorted(seen)          # {split 16-bit, fp32 decoder} x {decoder gradients or not} x {point gradient or not}
    for name, res in seen.items():
        assert res["ScratchSize [bytes/lane]"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
        assert res["Occupancy [waves/SIMD]"] >= 1, (name, res)
    text = asm.read_text()
    assert "planes_query_bwd_kernel" in text
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)


# ----------------------------------------------------------------------------- Python surface
def test_sample_mixed_still_refuses_a_gradient_without_the_keyword():
    import inspect
    from hfa_gp_amd.config import tiny64
    from hfa_gp_amd.generator import TriPlaneGenerator
    gen = TriPlaneGenerator(tiny64())
    sig = inspect.signature(gen.sample_mixed)
    assert sig.parameters["differentiable"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["differentiable"].default is False
    assert "query" in inspect.signature(gen.synthesis).parameters
    ws = torch.zeros(1, gen.cfg.num_ws, gen.cfg.w_dim, requires_grad=True)
    with pytest.raises(RuntimeError, match="no_grad") as e:
        gen._no_backward("sample_mixed", ws)
    assert "differentiable=True" in str(e.value)
    # the ops wrapper refuses grid mode and a call with nothing to compute before it reaches the library
    from hfa_gp_amd import ops
    assert {"d_planes", "coords_grad", "decoder_grads", "dec_out"} <= set(inspect.signature(ops.planes_query_bwd).parameters)
