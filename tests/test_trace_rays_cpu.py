"""Surface tracing without a GPU: the torch restatement of hfagp_trace_rays (tests/trace_ref.py) on an analytic field, the implicit
gradient of the traced depth (`ray_losses.implicit_depth`) against a closed form and against central differences on the oracle's
density, `cam_utils.pixel_rays` against `ray_grid`, the C surface, and the kernel's build-time resources."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import query_ref as Q
from tests import trace_ref as T
from tests.util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F64 = torch.float64

# ----------------------------------------------------------------------------- 1. the analytic field sigma = a - b |x|
A, Bc, LEVEL = 5.0, 4.0, 3.0                       # the surface is the sphere of radius (A - LEVEL) / Bc = 0.5


def _rays(n, seed, dtype=F64):
    """n rays from the sphere of radius 2 aimed at points within 0.3 of the centre (all cross the surface), |d| in [0.5, 2]."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(1, n, 3, generator=g, dtype=F64)
    o = 2.0 * u / u.norm(dim=-1, keepdim=True)
    aim = (torch.rand(1, n, 3, generator=g, dtype=F64) - 0.5) * 0.6 / 3 ** 0.5
    d = aim - o
    d = d / d.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * torch.rand(1, n, 1, generator=g, dtype=F64))
    return o.to(dtype), d.to(dtype)


@pytest.mark.parametrize("steps,refine", [(1, 0), (1, 12), (7, 5), (64, 8), (33, 0), (16, 30)])
def test_analytic_field_root(steps, refine):
    o, d = _rays(37, 1)
    t_mid = -(o * d).sum(-1) / (d * d).sum(-1)                    # closest approach to the centre: inside the sphere
    tn, tf = torch.zeros_like(t_mid), t_mid                        # so that the last node t_steps = t_far hits even at steps = 1
    out = T.trace(T.sphere_sigma(A, Bc), o, d, tn, tf, LEVEL, steps, refine)
    exact = T.sphere_root(A, Bc, LEVEL, o, d)
    dt = (tf - tn) / steps
    assert bool(out["hit"].all())
    want_cell = torch.ceil(exact / dt).clamp(max=steps).to(torch.int32)          # first node at or past the root
    assert torch.equal(out["cell"], want_cell)
    w = T.bracket_width(tn, tf, steps, refine)
    err = (out["t"] - exact).abs()
    print(f"steps {steps} refine {refine}: max |t - exact| / bracket width = {float((err / w).max()):.3e}")
    assert bool((err <= w).all())
    # the final bracket: `refine` halvings of a coarse interval (each midpoint rounded once: a few ulp of t), t inside it
    assert bool((out["hi"] - out["lo"] <= w + 8 * torch.finfo(F64).eps * out["hi"]).all())
    assert bool((out["lo"] <= out["t"]).all()) and bool((out["t"] <= out["hi"]).all())


def test_analytic_field_special_rays():
    o, d = _rays(8, 2)
    t_mid = -(o * d).sum(-1) / (d * d).sum(-1)
    tn, tf = torch.zeros_like(t_mid), t_mid.clone()
    exact = T.sphere_root(A, Bc, LEVEL, o, d)
    o[0, 0] = torch.tensor([0.1, -0.2, 0.05], dtype=F64)           # starts inside: cell 0, t = t_near
    tn[0, 0], tf[0, 0] = 0.25, 0.5
    o[0, 1], d[0, 1] = torch.tensor([2.0, 0.0, 0.0], dtype=F64), torch.tensor([0.0, 1.0, 0.0], dtype=F64)      # passes at distance 2
    tn[0, 1], tf[0, 1] = 0.0, 3.0
    tf[0, 2] = tn[0, 2]                                            # empty: t_far <= t_near
    tn[0, 3] = float("nan")                                        # empty: a NaN limit
    tf[0, 4] = float("inf")                                        # empty: a limit that is not finite
    tf[0, 5] = 0.5 * exact[0, 5]                                   # stops short of the surface: a miss
    out = T.trace(T.sphere_sigma(A, Bc), o, d, tn, tf, LEVEL, 16, 6)
    assert out["cell"][0].tolist()[:6] == [0, -1, -1, -1, -1, -1]
    assert out["hit"][0].tolist() == [True] + [False] * 5 + [True, True]
    assert float(out["t"][0, 0]) == 0.25 and bool((out["t"][0, 1:6] == 0).all())
    assert bool(torch.isfinite(out["t"]).all())
    assert bool(((out["t"][0, 6:] - exact[0, 6:]).abs() <= T.bracket_width(tn, tf, 16, 6)[0, 6:]).all())


def test_nan_density_never_hits():
    o, d = _rays(6, 3)
    t_mid = -(o * d).sum(-1) / (d * d).sum(-1)
    tn, tf = torch.zeros_like(t_mid), t_mid
    base = T.sphere_sigma(A, Bc)
    exact = T.sphere_root(A, Bc, LEVEL, o, d)

    def all_nan(x):
        return torch.full(x.shape[:-1], float("nan"), dtype=x.dtype)

    out = T.trace(all_nan, o, d, tn, tf, LEVEL, 8, 4)
    assert not bool(out["hit"].any()) and bool((out["cell"] == -1).all()) and bool((out["t"] == 0).all())

    def nan_shell(x):                                               # NaN in a shell just outside the surface, on ray 0 only
        s = base(x)
        r = x.norm(dim=-1)
        bad = (r > 0.5) & (r < 0.8)
        bad[:, 1:] = False
        return torch.where(bad, torch.full_like(s, float("nan")), s)

    out = T.trace(nan_shell, o, d, tn, tf, LEVEL, 8, 10)
    assert bool(out["hit"].all()) and bool(torch.isfinite(out["t"]).all())
    # a NaN at a bisection point goes to the low side, so ray 0 still closes in on the surface from outside; and with a NaN
    # density at the low end the secant step is refused: t = hi
    assert float(out["t"][0, 0]) == float(out["hi"][0, 0])
    assert bool(((out["t"] - exact).abs() <= T.bracket_width(tn, tf, 8, 10)).all())


def test_restatement_runs_in_fp32():
    o, d = _rays(21, 4, torch.float32)
    t_mid = -(o * d).sum(-1) / (d * d).sum(-1)
    tn, tf = torch.zeros_like(t_mid), t_mid
    out = T.trace(T.sphere_sigma(A, Bc), o, d, tn, tf, LEVEL, 24, 8)
    exact = T.sphere_root(A, Bc, LEVEL, o.double(), d.double())
    assert out["t"].dtype == torch.float32 and bool(out["hit"].all())
    # fp32: the bracket width (~5e-4) plus the rounding of x and sigma (~1e-6 in sigma) over the slope along the ray,
    # |d sigma / dt| = b |d| cos >= 4 * 0.5 * 0.8: below 1e-5 in t
    assert bool(((out["t"].double() - exact).abs() <= T.bracket_width(tn, tf, 24, 8).double() + 1e-5).all())


# ----------------------------------------------------------------------------- 2. implicit_depth against the closed form
def test_implicit_depth_matches_closed_form_autograd():
    """d/d(a, b, o, d) of sum_r c_r t_r: autograd of the closed-form root against `implicit_depth` on the traced root (refine = 40:
    the root to float64 rounding).  Equal to float64 rounding — 1e-12 relative to the largest entry leaves four digits for the
    cancellation in the closed form's square root (found: 2e-15).  Grazing, inside and missed rays: exact zeros."""
    from hfa_gp_amd.ray_losses import implicit_depth, transversal
    o, d = _rays(24, 5)
    t_mid = -(o * d).sum(-1) / (d * d).sum(-1)
    tn, tf = torch.zeros_like(t_mid), t_mid.clone()
    # ray 0: a grazing crossing — impact parameter 0.5 (1 - 1e-5), the cosine of the crossing is ~4.5e-3 < 0.01
    o[0, 0] = torch.tensor([-2.0, 0.5 * (1 - 1e-5), 0.0], dtype=F64)
    d[0, 0] = torch.tensor([1.0, 0.0, 0.0], dtype=F64)
    tn[0, 0], tf[0, 0] = 0.0, 2.0
    # ray 1 starts inside, ray 2 stops short of the surface
    o[0, 1] = torch.tensor([0.1, 0.1, -0.1], dtype=F64)
    d[0, 1] = torch.tensor([-0.3, -0.3, 0.3], dtype=F64)             # towards the centre: the density rises along it
    tn[0, 1], tf[0, 1] = 0.0, 0.1
    tf[0, 2] = 0.1
    c = torch.randn(1, 24, generator=torch.Generator().manual_seed(6), dtype=F64)
    a = torch.tensor(A, dtype=F64, requires_grad=True)
    b = torch.tensor(Bc, dtype=F64, requires_grad=True)
    o.requires_grad_(True)
    d.requires_grad_(True)
    with torch.no_grad():
        tr = T.trace(T.sphere_sigma(a, b), o, d, tn, tf, LEVEL, 16, 40)
    assert tr["cell"][0, :3].tolist()[1:] == [0, -1] and int(tr["cell"][0, 0]) > 0 and bool((tr["cell"][0, 3:] > 0).all())
    mask = tr["hit"] & (tr["cell"] > 0)
    x = o + tr["t"][..., None] * d
    sig = a - b * x.norm(dim=-1)
    g = (-b * x / x.norm(dim=-1, keepdim=True)).detach()
    ok = transversal(g, d.detach())
    assert ok[0].tolist() == [False] + [True] * 23                   # only the grazing ray fails the slope floor
    t = implicit_depth(tr["t"], sig, g, d, mask=mask)
    assert torch.equal(t.detach(), tr["t"])
    got = torch.autograd.grad((c * t).sum(), [a, b, o, d], retain_graph=True)
    keep = mask & ok
    exact = T.sphere_root(a, b, LEVEL, o, d)
    assert float((exact.detach() - tr["t"])[keep].abs().max()) <= 1e-13
    want = torch.autograd.grad((c * torch.where(keep, exact, torch.zeros_like(exact))).sum(), [a, b, o, d])
    for name, gv, wv in zip("abod", got, want):
        err = float((gv - wv).abs().max()) / float(wv.abs().max())
        print(f"d/d{name}: max err / max |ref| = {err:.3e}")
        assert err <= 1e-12
    for gv in got[2:]:
        assert bool((gv[0, :3] == 0).all())                          # grazing, inside, missed: exact zeros
    # without the mask the inside ray (a crossing slope of its own) would move: the mask is what makes it a constant
    t2 = implicit_depth(tr["t"], sig, g, d)
    assert bool((torch.autograd.grad(t2.sum(), o)[0][0, 1] != 0).any())


# ----------------------------------------------------------------------------- 3. the formula against differences, oracle density
FD_RAYS, FD_STEPS, FD_REFINE, FD_SEED = 48, 24, 40, 71
FD_EPS = (1e-4, 1e-5, 1e-6)
FD_TOL = 9.2e-6       # ten times the spread of the difference quotients over FD_EPS (the test's docstring has the figures)


@pytest.fixture(scope="module")
def fd_case():
    P, pn = T.planes_case()
    pn = pn.double()
    o, d, tn, tf = T.sphere_rays(torch.Generator().manual_seed(FD_SEED), Q.B, FD_RAYS, dtype=F64)
    sig = T.oracle_sigma(P, pn, "eg3d_original")
    with torch.no_grad():
        nodes = T.node_sigmas(sig, o, d, tn, tf, FD_STEPS)
        level = float(torch.quantile(nodes[torch.isfinite(nodes)], 0.9))
        base = T.trace(sig, o, d, tn, tf, level, FD_STEPS, FD_REFINE)
    return dict(P=P, pn=pn, rays=(o, d, tn, tf), level=level, base=base)


def test_implicit_formula_against_central_differences(fd_case):
    """sum_r c_r t_r on the planes of query_ref.base_case() in float64 (refine = 40): its derivative along three random plane
    directions by the implicit formula against central differences of the re-traced roots, over the rays on the formula (hit,
    cell > 0, slope above the floor) whose cell is the same at +eps and -eps.
    Measured here (seed 71, 2 x 48 rays, steps 24, level = the 0.9 quantile of the node densities): 81 of the 96 rays are on the
    formula, and none of the 96 (0 %) changes its cell at any eps; the difference quotients at eps = 1e-4, 1e-5, 1e-6 spread by at
    most 9.2e-7 of the derivative (the truncation error at 1e-4 leads): tolerance 9.2e-6 for the quotient at 1e-5, which is found
    9.2e-9 from the formula."""
    P, pn, (o, d, tn, tf), level, base = (fd_case[k] for k in ("P", "pn", "rays", "level", "base"))
    mask = base["hit"] & (base["cell"] > 0)
    g = torch.Generator().manual_seed(FD_SEED + 1)
    c = torch.randn(Q.B, FD_RAYS, generator=g, dtype=F64)
    assert int(mask.sum()) >= FD_RAYS                                        # at least half of the rays march to a crossing
    worst_changed, worst_spread, worst_err = 0.0, 0.0, 0.0
    for k in range(3):
        D = torch.randn(pn.shape, generator=g, dtype=F64)
        roots, same = {}, mask.clone()
        for eps in FD_EPS:
            with torch.no_grad():
                tp = T.trace(T.oracle_sigma(P, pn + eps * D, "eg3d_original"), o, d, tn, tf, level, FD_STEPS, FD_REFINE)
                tm = T.trace(T.oracle_sigma(P, pn - eps * D, "eg3d_original"), o, d, tn, tf, level, FD_STEPS, FD_REFINE)
            stable = (tp["cell"] == base["cell"]) & (tm["cell"] == base["cell"])
            worst_changed = max(worst_changed, 1.0 - float(stable.double().mean()))
            same &= stable
            roots[eps] = (tp["t"], tm["t"])
        pl = pn.clone().requires_grad_(True)
        (d_pl,), _, _, carries, _ = T.implicit_grads(lambda x: T.oracle_sigma(P, pl, "eg3d_original")(x), [pl], o, d, base["t"],
                                                      same, c, torch.zeros(Q.B, FD_RAYS, 3, dtype=F64))
        formula = float((d_pl * D).sum())
        quot = [float((c * (roots[e][0] - roots[e][1]))[carries].sum()) / (2 * e) for e in FD_EPS]
        spread = (max(quot) - min(quot)) / abs(formula)
        err = abs(quot[1] - formula) / abs(formula)
        print(f"direction {k}: formula {formula:.9e}, quotients {quot}, spread {spread:.3e}, err {err:.3e}, "
              f"{int(carries.sum())} rays on the formula")
        worst_spread, worst_err = max(worst_spread, spread), max(worst_err, err)
    print(f"worst share of rays changing cell {worst_changed:.4f}, worst spread {worst_spread:.3e}, worst err {worst_err:.3e}")
    assert worst_changed <= 0.05
    assert worst_err <= FD_TOL



# ----------------------------------------------------------------------------- 4. pixel_rays against ray_grid
def test_pixel_rays_equals_ray_grid_at_pixel_centres():
    from hfa_gp_amd.cam_utils import cam_sampler, pixel_rays, ray_grid
    torch.manual_seed(3)
    c = cam_sampler(3, "cpu")
    c[:, 17] = 0.013                                               # a skew, so that every term of the formula is live
    res = 13
    ar = torch.arange(res, dtype=c.dtype)
    centre = ar * (1.0 / res) + (0.5 / res)
    v, u = torch.meshgrid(centre, centre, indexing="ij")           # row i (v) major, column j (u) fastest: ray_grid's order
    uv = torch.stack((u.reshape(-1), v.reshape(-1)), -1)[None].repeat(3, 1, 1)
    o, d = pixel_rays(c, uv)
    og, dg = ray_grid(c, res)
    assert o.shape == (3, res * res, 3) and torch.equal(o, og) and torch.equal(d, dg)
    u0, v0, u1, v1 = 0.25, 0.1, 0.8, 0.55
    uvw = torch.stack((u0 + uv[..., 0] * (u1 - u0), v0 + uv[..., 1] * (v1 - v0)), -1)
    o, d = pixel_rays(c, uvw)
    og, dg = ray_grid(c, res, window=(u0, v0, u1, v1))
    assert torch.equal(o, og) and torch.equal(d, dg)
    # any subset of the points, in any order
    pick = torch.tensor([5, 0, 77, 168])
    o, d = pixel_rays(c, uvw[:, pick])
    assert torch.equal(o, og[:, pick]) and torch.equal(d, dg[:, pick])
    # differentiable in c and uv
    cg, ug = c.clone().requires_grad_(True), uvw[:, pick].clone().requires_grad_(True)
    o, d = pixel_rays(cg, ug)
    (o.sum() + (d * torch.tensor([1.0, 2.0, 3.0])).sum()).backward()
    assert bool((cg.grad.abs().sum(1) > 0).all()) and bool((ug.grad.abs().sum(-1) > 0).all())
    with pytest.raises(ValueError, match="uv must be"):
        pixel_rays(c, uvw[0])


# ----------------------------------------------------------------------------- 5. the C surface
@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_trace_rays_binding_matches_header(lib):
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} HfagpTraceRaysArgs;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\w+", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in lib.TraceRaysArgs._fields_]
    assert "hfagp_trace_rays" in lib.SYMBOLS


def test_trace_rays_argument_validation_returns_codes(lib):
    h = lib.lib()
    assert h.hfagp_trace_rays(None, None) == -1
    assert b"null pointer" in h.hfagp_last_error()
    a = lib.TraceRaysArgs()
    assert h.hfagp_trace_rays(C.byref(a), None) == -1
    for f in ("planes", "ray_origins", "ray_directions", "t_near", "t_far", "dec_w0", "dec_b0", "dec_w1", "dec_b1", "t"):
        setattr(a, f, 1)                                             # non-null, never dereferenced: the scalars are rejected first
    a.B, a.H, a.W, a.R, a.box_warp, a.steps, a.refine = 1, 8, 8, 5, 1.0, 0, 8
    assert h.hfagp_trace_rays(C.byref(a), None) == -1 and b"steps" in h.hfagp_last_error()
    a.steps = 4097
    assert h.hfagp_trace_rays(C.byref(a), None) == -1 and b"steps" in h.hfagp_last_error()
    a.steps, a.refine = 128, 31
    assert h.hfagp_trace_rays(C.byref(a), None) == -1 and b"refine" in h.hfagp_last_error()
    a.refine = -1
    assert h.hfagp_trace_rays(C.byref(a), None) == -1 and b"refine" in h.hfagp_last_error()
    a.refine, a.t = 8, None
    assert h.hfagp_trace_rays(C.byref(a), None) == -1 and b"output" in h.hfagp_last_error()
    a.t, a.H, a.W = 1, 8192, 8192
    assert h.hfagp_trace_rays(C.byref(a), None) == -2 and b"2^25" in h.hfagp_last_error()


def test_generator_and_ops_refuse_before_any_launch():
    from hfa_gp_amd import ops
    from hfa_gp_amd.config import tiny64
    from hfa_gp_amd.generator import TriPlaneGenerator
    gen = TriPlaneGenerator(tiny64())
    ws = torch.zeros(1, gen.cfg.num_ws, 512)
    o = torch.zeros(1, 4, 3)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gen.trace_rays(ws, o, o)
        with pytest.raises(ValueError, match="ray_limits must be"):
            gen.trace_rays(ws, o, o, ray_limits="sphere")
        with pytest.raises(ValueError, match="go together"):
            gen.trace_rays(ws, o, o, t_near=0.1)
        with pytest.raises(ValueError, match="mutually exclusive"):
            gen.trace_rays(ws, o, o, t_near=0.1, t_far=1.0, ray_limits="box")
        with pytest.raises(ValueError, match="steps"):
            gen.trace_rays(ws, o, o, steps=0)
        with pytest.raises(ValueError, match="refine"):
            gen.trace_rays(ws, o, o, refine=31)
        with pytest.raises(ValueError, match=r"\[B, R, 3\]"):
            gen.trace_rays(ws, o[0], o[0])
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.trace_rays(torch.zeros(1, 3, 8, 8, 32), o, o, o[..., 0], o[..., 0], 10.0, dec_w0=None, dec_b0=None, dec_w1=None,
                       dec_b1=None, box_warp=1.0, plane_axes=0, decoder_lr_mul=1.0, decoder_precision="fp32")


# ----------------------------------------------------------------------------- 6. the kernel's build-time resources
def _build_flags():
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(.*\bsurface_trace\b", build, re.M), "surface_trace.hip is not in build.sh's unit list"
    return re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_trace_rays_kernel_has_no_scratch_and_no_spills(tmp_path):
    """Compiled with build.sh's flags: every trace_rays_kernel instance — {split fp16, fp32 decoder} x {plain, normals} — without
    scratch and without VGPR or SGPR spills; the plain instances without LDS (the normals ones hold the 8 KB image of W0'^T)."""
    out = subprocess.run([HIPCC, *_build_flags(), "-c", os.path.join(ROOT, "hfa-gp_amd", "csrc", "surface_trace.hip"), "-o",
                          str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen, lds = None, set(), {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not (name and "trace_rays_kernel" in name):
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m:
            seen.add(name)
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m:
            lds[name] = int(m.group(1))
    assert len(seen) == 4 and set(lds) == seen, seen
    # the template arguments <DEC16, NORMALS> are mangled as ILb.ELb.E: NORMALS = 0 is the plain instance
    plain = [n for n in lds if re.search(r"ILb[01]ELb0E", n)]
    assert len(plain) == 2 and all(lds[n] == 0 for n in plain), lds
    assert all(lds[n] == 8192 for n in lds if n not in plain), lds


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_trace_rays_unit_has_no_packed_fp32_arithmetic(tmp_path):
    """test_kernel_resources.py's rule for every unit (build.sh's note on packed fp32 ops), as test_shape_cpu.py holds its units to it."""
    asm = tmp_path / "unit.s"
    out = subprocess.run([HIPCC, *_build_flags(), "-S", "--cuda-device-only", os.path.join(ROOT, "hfa-gp_amd", "csrc", "surface_trace.hip"),
                          "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = asm.read_text()
    assert "trace_rays_kernel" in text
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)
