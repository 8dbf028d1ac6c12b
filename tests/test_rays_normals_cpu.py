"""Surface normals along ray lists without a GPU: the float64 references of tests/rays_normals_ref.py against the grid's
(normals_ref, normal_grad_ref, normal_camera_ref) on the rays of a label, the two conditions the GPU tests rest on (the fp32 oracle's
edge rays, the edge mask's kept fraction) on the lists those tests use, the C entry points' argument checks through ctypes
(nothing is launched) and the host-side guards of `TriPlaneGenerator.render_rays(normals=, normal_grad=, normal_ray_grad=)`."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import normal_camera_ref as NC
from tests import normal_grad_ref as G
from tests import normals_ref as N
from tests import rays_normals_ref as RN
from tests.util import ROOT

# (preset, axes, plane (H, W), list, limits): the lists of tests/test_gpu_rays_normals.py
LIST_CASES = [("tiny64", "eg3d_original", (20, 20), "r27", None), ("small128", "eg3d_original", (20, 20), "r27", None),
              ("ffhq512_128", "eg3d_original", (20, 20), "r27", None), ("small128", "eg3d_fixed", (36, 20), "r27", None),
              ("small128", "eg3d_original", (20, 20), "miss", "box"), ("small128", "eg3d_original", (20, 20), "mixed", "box"),
              ("tiny64", "eg3d_original", (20, 20), "miss", "box")]
LIST_IDS = [f"{p}-{a}-{h[0]}x{h[1]}-{r}-{lim}" for p, a, h, r, lim in LIST_CASES]


# ----------------------------------------------------------------------------- the restatement is the same function
@pytest.mark.parametrize("case", [N.CASES[0], N.CASES[3]], ids=[N.CASE_IDS[0], N.CASE_IDS[3]])
def test_references_equal_the_grids_on_ray_grid(case):
    """On ray_grid(c, 10) in float64 the list references are normals_ref.case_reference, normal_grad_ref.reference and
    normal_camera_ref.reference (its dL/dx summed into the per-ray records) to 1e-12."""
    from hfa_gp_amd.cam_utils import ray_grid
    cs, ref = N.case(*case), N.case_reference(*case)
    cfg = cs["cfg"]
    o, d = ray_grid(cs["c"].double(), cfg.neural_rendering_resolution)
    got = RN.reference(cs["P"], cfg, cs["planes"], o, d, cs["us"], cs["ui"])
    for k in ("normal", "wsum", "fine_depths", "g"):
        err = float((got[k] - ref[k]).abs().max())
        print(f"{k}: max |list - grid| {err:.3e}")
        assert err <= 1e-12, k
    depths = G.oracle_depths(*case)
    assert float((got["depths"] - depths).abs().max()) <= 1e-12
    hw = case[2]
    mask = RN.edge_mask(cfg, hw, o, d, depths)
    assert torch.equal(mask, G.edge_mask(cfg, hw, cs["c"], depths))
    g_hat = G.upstream(cs) * mask[..., None]
    want = G.reference(cs["P"], cfg, cs["planes"], cs["c"], depths, g_hat)
    mine = RN.grad_reference(cs["P"], cfg, cs["planes"], o, d, depths, g_hat)
    for a, b, k in zip((mine["planes"],) + mine["dec"], (want["planes"],) + want["dec"], ("planes",) + G.DEC_KEYS):
        scale = max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        print(f"d {k}: max |list - grid| {err:.3e} (max |ref| {scale:.3e})")
        assert err <= 1e-12 * scale, k
    _, dx = NC.reference(cs["P"], cfg, cs["planes"], cs["c"], depths, g_hat)
    records = NC.ray_records(dx, depths)
    err = float((mine["rays"] - records).abs().max())
    print(f"rays: max |autograd w.r.t. (o, d) - ray sums of dL/dx| {err:.3e} (max |ref| {float(records.abs().max()):.3e})")
    assert err <= 1e-12 * max(1.0, float(records.abs().max()))


# ----------------------------------------------------------------------------- the conditions of the GPU tests
@pytest.mark.parametrize("key", LIST_CASES, ids=LIST_IDS)
def test_fp32_oracle_edge_rays_and_kept_fraction(key):
    """The fp32 oracle against float64, each drawing its own fine depths: at most N.MAX_EDGE_RAYS_ORACLE rays beyond the bar; the
    edge mask at the float64 depths keeps at least G.MIN_KEPT of the valid rays; the list renders a surface."""
    cs, ref = RN.case(*key), RN.case_reference(*key)
    got = RN.case_reference(*key, dtype=torch.float32)
    assert torch.equal(got["valid"], ref["valid"])
    bad = N.rays_beyond(got["normal"], ref["normal"], f"{key}: fp32 oracle")
    assert bad <= N.MAX_EDGE_RAYS_ORACLE, bad
    nrm = ref["normal"].norm(dim=-1)
    assert bool((nrm <= ref["wsum"] + 1e-12).all()) and float(nrm.max()) > 0.05, "the list renders no surface"
    valid = ref["valid"] if cs["lim"] is not None else None
    mask = RN.edge_mask(cs["cfg"], cs["hw"], cs["o"], cs["d"], ref["depths"], valid)
    frac = RN.kept(mask, valid)
    print(f"{key}: {int(ref['valid'].sum())} of {ref['valid'].numel()} rays valid, edge mask keeps {frac:.3f} of them")
    assert frac >= G.MIN_KEPT
    if key[3] == "miss":
        assert torch.equal(ref["valid"], ~RN.RL.MISS) and bool((ref["normal"][RN.RL.MISS] == 0).all())


def test_empty_rays_take_no_part_in_the_gradient_reference():
    """With the depths of the empty rays replaced by NaN (an unwritten state) the gradient reference is finite, equals the one of
    the list with those rays removed, and gives them a zero ray gradient."""
    key = ("tiny64", "eg3d_original", (20, 20), "miss", "box")
    cs, ref = RN.case(*key), RN.case_reference(*key)
    valid = ref["valid"]
    depths = torch.where(valid[..., None, None], ref["depths"], torch.full_like(ref["depths"], float("nan")))
    g_hat, _ = RN.masked_upstream(cs, depths, valid)
    g_hat = torch.where(valid[..., None], g_hat, torch.ones_like(g_hat))           # (dropped by the reference)
    full = RN.grad_reference(cs["P"], cs["cfg"], cs["planes"], cs["o"], cs["d"], depths, g_hat, valid=valid)
    keep = ~RN.RL.MISS[0]
    cut = lambda t: t[:, keep]                                                      # noqa: E731
    part = RN.grad_reference(cs["P"], cs["cfg"], cs["planes"], cut(cs["o"]), cut(cs["d"]), cut(ref["depths"]), cut(g_hat))
    assert all(bool(torch.isfinite(t).all()) for t in (full["planes"], full["rays"]) + full["dec"])
    assert float((full["planes"] - part["planes"]).abs().max()) <= 1e-12 * max(1.0, float(part["planes"].abs().max()))
    assert bool((full["rays"][~valid] == 0).all()) and float(full["rays"][valid].abs().max()) > 0


# ----------------------------------------------------------------------------- the C ABI, nothing launched
@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    _lib.lib()
    return _lib


def _filled_list(lib):
    """A RayListArgs whose pointers are non-null and never dereferenced: every call below is refused before a launch."""
    a = lib.RayListArgs()
    for k in ("planes", "u_strat", "u_imp", "dec_w0", "dec_b0", "dec_w1", "dec_b1", "state"):
        setattr(a.base, k, 256)
    a.base.B, a.base.H, a.base.W, a.base.Sc, a.base.Sf = 2, 20, 20, 24, 24       # 24 + 24 samples: unsupported, so a call that passes the other checks is -2
    a.base.ray_start, a.base.ray_end, a.base.box_warp, a.base.decoder_lr_mul = 2.25, 3.3, 1.0, 1.0
    a.ray_origins, a.ray_directions, a.R = 256, 256, 101
    return a


def test_entries_are_declared_bound_and_additive(lib):
    raw = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    assert re.search(r"#define HFAGP_ABI_VERSION 15\b", raw) and lib.lib().hfagp_abi_version() == 15
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("hfagp_raymarch_rays_normals", "hfagp_raymarch_rays_normals_bwd", "hfagp_raymarch_rays_normals_bwd_rays"):
        assert re.search(r"\b%s\(const HfagpRayListArgs\* list, const HfagpRayLimits\* lim," % name, text), name
        assert name in lib.SYMBOLS and hasattr(lib.lib(), name), name
    assert len(lib.SYMBOLS["hfagp_raymarch_rays_normals"][1]) == 4 and len(lib.SYMBOLS["hfagp_raymarch_rays_normals_bwd"][1]) == 9
    assert len(lib.SYMBOLS["hfagp_raymarch_rays_normals_bwd_rays"][1]) == 7
    from hfa_gp_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("raymarch_rays_normals", "raymarch_rays_normals_bwd", "raymarch_rays_normals_bwd_rays"))


def test_entries_check_their_arguments(lib):
    h = lib.lib()
    fwd, bwd, rays = h.hfagp_raymarch_rays_normals, h.hfagp_raymarch_rays_normals_bwd, h.hfagp_raymarch_rays_normals_bwd_rays
    calls = {"raymarch_rays_normals": lambda a, lim: fwd(a, lim, 256, None),
             "raymarch_rays_normals_bwd": lambda a, lim: bwd(a, lim, 256, 256, None, None, None, None, None),
             "raymarch_rays_normals_bwd_rays": lambda a, lim: rays(a, lim, 256, 256, 256, 0, None)}
    for who, call in calls.items():
        assert call(None, None) == -1 and (who + ": null pointer").encode() in h.hfagp_last_error()
        a = _filled_list(lib)
        assert call(C.byref(a), None) == -2 and b"unsupported sample counts" in h.hfagp_last_error(), who
        a.base.state = None
        assert call(C.byref(a), None) == -1 and (who + ": null pointer").encode() in h.hfagp_last_error()
        for field in ("ray_origins", "ray_directions"):
            a = _filled_list(lib)
            setattr(a, field, None)
            assert call(C.byref(a), None) == -1 and b"null pointer" in h.hfagp_last_error(), (who, field)
        a = _filled_list(lib)
        a.R = 0
        assert call(C.byref(a), None) == -1 and b"rays per frame" in h.hfagp_last_error(), who
        # the config's interval is checked without limits and ignored with them; limits with a NULL member are refused
        a = _filled_list(lib)
        a.base.ray_end = a.base.ray_start
        assert call(C.byref(a), None) == -1 and b"bad ray range" in h.hfagp_last_error(), who
        lim = lib.RayLimits()
        lim.t_near = 256
        assert call(C.byref(a), C.byref(lim)) == -1 and b"null pointer (limits)" in h.hfagp_last_error(), who
        lim.t_far = 256
        assert call(C.byref(a), C.byref(lim)) == -2 and b"unsupported sample counts" in h.hfagp_last_error(), who
    a = _filled_list(lib)
    assert fwd(C.byref(a), None, None, None) == -1
    assert bwd(C.byref(a), None, None, 256, None, None, None, None, None) == -1
    assert bwd(C.byref(a), None, 256, None, None, None, None, None, None) == -1
    assert bwd(C.byref(a), None, 256, 256, 256, None, None, None, None) == -1 and b"go together" in h.hfagp_last_error()
    assert rays(C.byref(a), None, 256, None, 256, 0, None) == -1 and rays(C.byref(a), None, 256, 256, None, 1, None) == -1
    assert rays(C.byref(a), None, None, 256, 256, 0, None) == -1


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_list_unit_resources(tmp_path):
    """raymarch_rays_normals.hip, on its own `units+=` line of build.sh and compiled with build.sh's flags: the 24 list instantiations
    (6 forward, 12 plane / decoder backward, 6 rays' kernels) and no grid kernel, every one without scratch and without spilled
    vector registers, and no packed fp32 arithmetic (build.sh's note) in its ISA; build.sh hashes the three included sources."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(raymarch_rays_normals\)$", build, re.M), "raymarch_rays_normals.hip is not on its own units+= line"
    assert re.search(r'includes=\(\[raymarch_rays_normals\]="raymarch_normals raymarch_normals_bwd raymarch_normals_camera"\)', build)
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    src = os.path.join(ROOT, "hfa-gp_amd", "csrc", "raymarch_rays_normals.hip")
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
    # (Itanium mangling: the trailing template argument Lb1E is LIST = true)
    fwd = [n for n in seen if re.search(r"raymarch_normals_kernelILi\d+ELb[01]ELb1EE", n)]
    bwd = [n for n in seen if re.search(r"raymarch_normals_bwd_kernelILi\d+ELb[01]ELb[01]ELb1EE", n)]
    rays = [n for n in seen if "raymarch_normals_camera_rays_kernel" in n]
    assert (len(fwd), len(bwd), len(rays), len(seen)) == (6, 12, 6, 24), sorted(seen)
    for n, v in seen.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0}, (n, v)
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", asm.read_text())


# ----------------------------------------------------------------------------- host-side guards
def _gen():
    from hfa_gp_amd.config import tiny64
    from hfa_gp_amd.generator import TriPlaneGenerator
    return TriPlaneGenerator(tiny64()).requires_grad_(False)


def test_render_rays_keywords_and_refusals_need_no_device():
    import inspect
    g = _gen()
    sig = inspect.signature(g.render_rays)
    for k in ("normals", "normal_grad", "normal_ray_grad"):
        assert sig.parameters[k].default is False, k
    ws = torch.zeros(2, g.cfg.num_ws, 512)
    rays = torch.zeros(2, 5, 3)
    # the rays' gradient of the normal term is opt-in: refused before the device is looked at
    for kw in (dict(normal_grad=True), dict(normals=True, normal_grad=True)):
        with pytest.raises(NotImplementedError, match="rays' gradient of the normal term is opt-in.*normal_ray_grad=True"):
            g.render_rays(ws, rays.clone().requires_grad_(True), rays, **kw)
        with pytest.raises(NotImplementedError, match="normal_ray_grad=True"):
            g.render_rays(ws, rays, rays.clone().requires_grad_(True), **kw)
    # ... not under no_grad, not for a detached map, not with the opt-in: those reach the device check
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        g.render_rays(ws, rays.clone().requires_grad_(True), rays, normal_grad=True)
    for kw in (dict(normals=True), dict(normal_ray_grad=True), dict(normal_grad=True, normal_ray_grad=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            g.render_rays(ws, rays.clone().requires_grad_(True), rays, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.render_rays(ws, rays, rays, normal_grad=True)


@pytest.mark.parametrize("b,r", [(0, 5), (2, 0), (0, 0)])
def test_empty_call_shapes_and_edges(b, r):
    """`ray_list._empty` is what `render_rays` returns for B = 0 or R = 0: 'normal' [B,R,3] only when asked for, detached unless
    normal_grad, with the autograd edge of the call's inputs under grad."""
    from hfa_gp_amd import ray_list
    plain = ray_list._empty(b, r, "cpu", 0.0, False, False, False)
    assert set(plain) == {"feature", "rgb", "depth", "mask"}
    src = torch.zeros(3, requires_grad=True)
    zero = 0.0 * src.sum()
    out = ray_list._empty(b, r, "cpu", zero, True, True, False)
    assert set(out) == {"feature", "rgb", "depth", "mask", "valid", "normal"}
    assert out["normal"].shape == (b, r, 3) and not out["normal"].requires_grad and out["feature"].requires_grad
    out = ray_list._empty(b, r, "cpu", zero, False, True, True)
    assert out["normal"].shape == (b, r, 3) and out["normal"].requires_grad and out["normal"].dtype == torch.float32
    out["normal"].sum().backward()
    assert src.grad is not None and bool((src.grad == 0).all())


def test_ops_refuse_a_missing_state_before_anything_else():
    from hfa_gp_amd import ops
    t = torch.zeros(1)
    for name in ("raymarch_rays_normals", "raymarch_rays_normals_bwd", "raymarch_rays_normals_bwd_rays"):
        args = (t, t, None) if name != "raymarch_rays_normals" else (t, None)
        with pytest.raises(RuntimeError, match=f"{name}: state must be the `raymarch_state` buffer the forward call filled, got None"):
            getattr(ops, name)(*args, ray_origins=t, ray_directions=t, u_strat=t, u_imp=t, dec_w0=t, dec_b0=t, dec_w1=t, dec_b1=t,
                               ray_start=2.25, ray_end=3.3, box_warp=1.0, decoder_lr_mul=1.0, plane_axes=0, white_back=False,
                               decoder_precision="fp32")
