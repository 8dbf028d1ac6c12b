"""The antialiased resample without a GPU: the host-built tap tables of ops.resize_aa against torch's F.interpolate(antialias=True)
in float64, their invariants, the argument validation of the two C entry points, and the composed reference of
tests/resample_ref.py against the oracle at the native resolution."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import resample_ref
from tests.util import ROOT, perturb_state, state_cpu

SQUARES = [(8, 16), (24, 16), (32, 16), (64, 16), (63, 16), (10, 16), (40, 10), (4, 16), (64, 128), (256, 128)]
SHAPES = [((n, n), (m, m)) for n, m in SQUARES] + [((7, 12), (5, 16))]


@pytest.mark.parametrize("in_hw,out_hw", SHAPES, ids=[f"{i[0]}x{i[1]}-{o[0]}x{o[1]}" for i, o in SHAPES])
def test_dense_tables_match_interpolate(in_hw, out_hw):
    from hfa_gp_amd import ops
    wy, wx = ops._aa_tables(in_hw[0], out_hw[0])[2], ops._aa_tables(in_hw[1], out_hw[1])[2]
    assert wy.dtype == torch.float64 and wy.shape == (out_hw[0], in_hw[0]) and wx.shape == (out_hw[1], in_hw[1])
    x = torch.randn(2, 3, *in_hw, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ref = F.interpolate(x, out_hw, mode="bilinear", align_corners=False, antialias=True)
    err = (wy @ x @ wx.T - ref).abs().max().item()
    print(f"{in_hw} -> {out_hw}: max err {err:.3e}")
    assert err <= 1e-12


def test_known_taps():
    from hfa_gp_amd import ops
    down = ops._aa_tables(256, 128)[2]
    assert torch.equal(down[5, 8:14], torch.tensor([0, 1, 3, 3, 1, 0], dtype=torch.float64) / 8)
    start, count, w = ops._aa_unpack(ops._aa_tables(64, 128)[0])
    assert int(count.max()) == 2                                   # up-sampling: plain two-tap bilinear
    assert torch.equal(w[5, :2], torch.tensor([0.75, 0.25])) and int(start[5]) == 2


def _densify(table, n_src):
    from hfa_gp_amd import ops
    start, count, w = ops._aa_unpack(table)
    out = torch.zeros(table.shape[0], n_src)
    for d in range(table.shape[0]):
        assert 0 <= int(start[d]) and int(start[d]) + int(count[d]) <= n_src
        assert bool((w[d, int(count[d]):] == 0).all())
        out[d, int(start[d]):int(start[d]) + int(count[d])] = w[d, :int(count[d])]
    return out


@pytest.mark.parametrize("n_in,n_out", SQUARES + [(7, 5), (12, 16)], ids=lambda v: str(v))
def test_table_invariants(n_in, n_out):
    from hfa_gp_amd import ops
    forward, transposed, dense = ops._aa_tables(n_in, n_out)
    assert forward.dtype == transposed.dtype == torch.int32
    assert forward.shape == (n_out, 2 + ops.AA_KMAX) and transposed.shape == (n_in, 2 + ops.AA_KMAX)
    fw = _densify(forward, n_in)
    assert torch.equal(fw, dense.float())
    assert bool(((fw.double().sum(1) - 1).abs() <= 1e-6).all())
    assert torch.equal(_densify(transposed, n_out), dense.float().T)        # the same fp32 entries, transposed


@pytest.mark.parametrize("n_out", [10, 16, 128])
def test_table_caps_over_the_supported_range(n_out):
    from hfa_gp_amd import _lib, ops
    assert ops.AA_KMAX == 9
    header = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    assert f"#define HFAGP_RESIZE_AA_KMAX {ops.AA_KMAX}\n" in header
    for n_in in range(-(-n_out // 4), 4 * n_out + 1):
        forward, transposed, _ = ops._aa_tables(n_in, n_out)
        assert int(forward[:, 1].max()) <= ops.AA_KMAX and int(forward[:, 1].min()) >= 1, n_in
        assert int(transposed[:, 1].max()) <= ops.AA_KMAX and int(transposed[:, 1].min()) >= 1, n_in
    for n_in in (-(-n_out // 4) - 1, 4 * n_out + 1, 0):
        with pytest.raises(ValueError, match="outside the supported ratios"):
            ops._aa_tables(n_in, n_out)


def test_argument_validation_returns_codes():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.lib()
    for fn in (h.hfagp_resize_aa_fwd, h.hfagp_resize_aa_bwd):
        assert fn(None, None) == -1
        assert b"null pointer" in h.hfagp_last_error()
        a = _lib.ResizeAaArgs()
        a.B, a.Hi, a.Wi, a.Ho, a.Wo, a.C, a.kmax = 1, 8, 8, 16, 16, 32, 9
        assert fn(C.byref(a), None) == -1                    # every pointer null
        a.src = a.dst = a.table_h = 1                        # non-null, never dereferenced: the checks come first
        assert fn(C.byref(a), None) == -1                    # one table missing
        a.table_w = 1
        a.C = 6
        assert fn(C.byref(a), None) == -2
        assert b"multiple of 4" in h.hfagp_last_error()
        a.C, a.kmax = 32, 10
        assert fn(C.byref(a), None) == -2
        assert b"kmax=10" in h.hfagp_last_error() and b"compiled for" in h.hfagp_last_error()
        a.kmax, a.Wo = 9, 0
        assert fn(C.byref(a), None) == -2
        assert b"empty extent" in h.hfagp_last_error()
        a.Wo, a.Hi = 16, 65
        assert fn(C.byref(a), None) == -2
        assert b"supported ratios" in h.hfagp_last_error()
        a.Hi, a.Wi = 8, 3
        assert fn(C.byref(a), None) == -2
        assert b"supported ratios" in h.hfagp_last_error()


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_unit_resources(tmp_path):
    """resample_aa.hip is in build.sh's list and, compiled with its flags: both kernels without scratch, spill or LDS, 16-byte
    loads and stores, and none of the packed fp32 arithmetic build.sh keeps out of the library."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(.*\bresample_aa\b", build, re.M), "resample_aa.hip is not in build.sh's unit list"
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    asm = tmp_path / "unit.s"
    out = subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", os.path.join(ROOT, "hfa-gp_amd", "csrc", "resample_aa.hip"),
                          "-o", str(asm), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, set()
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            seen.add(name)
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert len(seen) == 2 and any("resize_aa_kernel" in n for n in seen) and any("resize_aa_bwd_kernel" in n for n in seen), seen
    text = asm.read_text()
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)


def test_binding_matches_header():
    """The ctypes image of HfagpResizeAaArgs has the header's field order."""
    from hfa_gp_amd import _lib
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} HfagpResizeAaArgs;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\w+", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.ResizeAaArgs._fields_]


def test_entry_checks_need_no_gpu():
    """The refusals of synthesis(neural_rendering_resolution=) that come before the device check's successors: a bad N on CPU tensors
    still reports the missing device first (no CPU fallback), and the attribute starts at the configured value."""
    from hfa_gp_amd.config import tiny64
    from hfa_gp_amd.generator import TriPlaneGenerator
    g = TriPlaneGenerator(tiny64())
    assert g.neural_rendering_resolution == g.cfg.neural_rendering_resolution == 16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.synthesis(torch.zeros(1, g.cfg.num_ws, 512), torch.zeros(1, 25), neural_rendering_resolution=8)
    for bad in (3, 65, 8.5, True):
        with pytest.raises(ValueError, match="neural_rendering_resolution"):
            g._set_resolution(1, bad, None, None)
    assert g.neural_rendering_resolution == 16
    g._set_resolution(1, 8, None, None)
    assert g.neural_rendering_resolution == 8
    with pytest.raises(ValueError, match="u_strat"):
        g._set_resolution(2, None, torch.zeros(2, 256, g.cfg.depth_resolution, 1), None)      # sized for 16^2 rays, not 8^2
    g._set_resolution(2, None, torch.zeros(2, 64, g.cfg.depth_resolution, 1), torch.zeros(128, g.cfg.depth_resolution_importance))


def test_reference_at_native_resolution_is_the_oracle():
    from hfa_gp_amd.config import tiny64
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = tiny64()
    P = state_cpu(perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False))
    ws, c, us, ui = resample_ref.inputs(cfg, 2, cfg.neural_rendering_resolution)
    with torch.no_grad():
        want = O.synthesis(P, cfg, ws, c, us, ui, return_planes=True)
        for n in (None, cfg.neural_rendering_resolution):
            got = resample_ref.synthesis(P, cfg, ws, c, us, ui, n)
            for k in ("image", "image_raw", "image_depth", "feature_image"):
                assert torch.equal(got[k], want[k]), k
        # and off it the shapes are EG3D's: the ray images at n, the image at the configured size
        ws, c, us, ui = resample_ref.inputs(cfg, 1, 8)
        got = resample_ref.synthesis(P, cfg, ws, c, us, ui, 8)
    assert got["image"].shape == (1, 3, 64, 64) and got["image_raw"].shape == (1, 3, 8, 8)
    assert got["image_depth"].shape == got["image_mask"].shape == (1, 1, 8, 8)
