"""Query-point normals without a GPU: the float64 reference of tests/query_normals_ref.py against central differences, the fp32
oracle against it, the two C entries (header, binding, argument validation), the build-time resources of the two HIP units,
the PLY writer with normals and the CLI flag."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import normal_grad_ref as NG
from tests import query_normals_ref as R
from tests import query_ref as Q
from tests.util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = [("planes_query_normals", "planes_query_normals_kernel", 4), ("planes_query_normals_bwd", "planes_query_normals_bwd_kernel", 4)]


# ----------------------------------------------------------------------------- the reference
def test_forward_reference_vs_central_differences_of_sigma():
    cs = Q.base_case()
    P = {k: cs["P"][k].double() for k in Q.DEC_KEYS}
    eps = 1e-6
    for axes in Q.AXES:
        ref = R.base_forward(axes)
        for k in range(3):
            d = torch.zeros(3, dtype=torch.float64)
            d[k] = eps
            sp = Q.query_fp64(P, cs["pn"].double(), cs["coords"].double() + d, Q.BOX_WARP, axes, Q.LR_MUL)[1]
            sm = Q.query_fp64(P, cs["pn"].double(), cs["coords"].double() - d, Q.BOX_WARP, axes, Q.LR_MUL)[1]
            fd = ((sp - sm) / (2 * eps))[..., 0]
            err = float((fd - ref["g"][..., k]).abs().max())
            print(f"{axes} axis {k}: max |fd - g| {err:.3e}, max |g| {float(ref['g'].abs().max()):.3e}")
            assert err <= 1e-6 * max(1.0, float(ref["g"].abs().max()))
        # outside every plane: exact zeros; elsewhere the normalisation is well conditioned and n has unit length
        assert bool((ref["g"][:, :2] == 0).all()) and bool((ref["n"][:, :2] == 0).all())
        norm = ref["g"].norm(dim=-1)
        assert float(norm[norm > 0].min()) > 0.1
        assert float((ref["n"].norm(dim=-1)[norm > 0] - 1).abs().max()) < 1e-9


def _first_order_loss(P, pn, axes, gg, gn):
    f = R.forward(P, pn, Q.base_case()["coords"], axes)
    return float((f["g"] * gg.double()).sum() + (f["n"] * gn.double()).sum())


@pytest.mark.parametrize("axes", Q.AXES)
def test_backward_reference_vs_central_differences(axes):
    """Second order: central differences of the first-order loss <g, G_g> + <n, G_n> w.r.t. a handful of plane texels and decoder
    entries against the double-backward reference."""
    cs = Q.base_case()
    gg, gn = R.upstream()
    ref = R.base_backward(axes, "both")
    eps = 1e-5
    g = torch.Generator().manual_seed(3)
    nz = ref["planes"].abs().flatten().topk(200).indices
    picks = [("planes", int(nz[int(i)])) for i in torch.randint(0, 200, (6,), generator=g)]
    picks += [(k, int(torch.randint(0, cs["P"][k].numel(), (1,), generator=g))) for k in Q.DEC_KEYS[:3] for _ in range(2)]
    picks.append((Q.DEC_KEYS[2], 5))                     # an entry of the sigma row
    for name, idx in picks:
        vals = []
        for sgn in (1.0, -1.0):
            P = {k: cs["P"][k].double().clone() for k in Q.DEC_KEYS}
            pn = cs["pn"].double().clone()
            (pn if name == "planes" else P[name]).view(-1)[idx] += sgn * eps
            vals.append(_first_order_loss(P, pn, axes, gg, gn))
        fd = (vals[0] - vals[1]) / (2 * eps)
        want = float((ref["planes"] if name == "planes" else ref["dec"][Q.DEC_KEYS.index(name)]).flatten()[idx])
        print(f"{axes} {name}[{idx}]: fd {fd:.6e} reference {want:.6e}")
        assert abs(fd - want) <= 1e-5 * max(1.0, abs(want)), (name, idx)
    # the colour rows of the second layer and all of its bias receive nothing
    assert bool((ref["dec"][2][1:] == 0).all()) and bool((ref["dec"][3] == 0).all())


@pytest.mark.parametrize("axes", Q.AXES)
def test_fp32_oracle_is_within_the_bar(axes):
    f64, f32 = R.base_forward(axes), R.base_forward(axes, dtype=torch.float32)
    assert R.worst(f32["g"], f64["g"], f"{axes} fp32 oracle g") <= 1.0
    assert R.worst(f32["n"], f64["n"], f"{axes} fp32 oracle n") <= 1.0
    b64, b32 = R.base_backward(axes, "both"), R.base_backward(axes, "both", dtype=torch.float32)
    assert R.rho(b32["planes"], b32["dec"], b64, f"{axes} fp32 oracle backward") <= 1.0


# ----------------------------------------------------------------------------- the C entries
def test_header_and_binding_agree_on_the_two_entries():
    from hfa_gp_amd import _lib
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    assert re.search(r"#define HFAGP_ABI_VERSION 15\b", text) and _lib.ABI_VERSION == 15
    nocomment = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, struct, cls in (("hfagp_planes_query_normals", "HfagpPlanesQueryArgs", _lib.PlanesQueryArgs),
                              ("hfagp_planes_query_normals_bwd", "HfagpPlanesQueryBwdArgs", _lib.PlanesQueryBwdArgs)):
        m = re.search(r"int %s\(([^)]*)\);" % name, nocomment)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == len(argtypes) == 4
        assert args[0].startswith(f"const {struct}*") and argtypes[0]._type_ is cls
        assert all(t is C.c_void_p for t in argtypes[1:]) and args[3].startswith("void*")


def _filled(cls):
    from hfa_gp_amd import _lib
    a = cls()
    for k in ("planes", "coords", "dec_w0", "dec_b0", "dec_w1", "dec_b1"):
        setattr(a, k, 256)                       # never dereferenced: every call below is refused before a launch
    a.B, a.H, a.W, a.Bc, a.M, a.box_warp, a.decoder_lr_mul = 1, 8, 8, 1, 4, 1.0, 1.0
    return a, _lib.lib()


def test_forward_entry_validates_its_arguments():
    from hfa_gp_amd import _lib
    a, lib = _filled(_lib.PlanesQueryArgs)
    fn = lib.hfagp_planes_query_normals
    assert fn(None, 256, 256, None) == -1
    assert fn(C.byref(a), None, None, None) == -1 and b"at least one output" in lib.hfagp_last_error()
    a.planes = None
    assert fn(C.byref(a), 256, None, None) == -1
    a.planes, a.coords = 256, None
    assert fn(C.byref(a), 256, None, None) == -2 and b"grid" in lib.hfagp_last_error()
    a.coords, a.M = 256, 0
    assert fn(C.byref(a), 256, None, None) == -1
    a.M, a.Bc, a.B = 4, 3, 2
    assert fn(C.byref(a), 256, None, None) == -1
    a.Bc, a.out_stride = 1, 3
    assert fn(C.byref(a), 256, None, None) == -1 and b"out_stride" in lib.hfagp_last_error()


def test_backward_entry_validates_its_arguments():
    from hfa_gp_amd import _lib
    a, lib = _filled(_lib.PlanesQueryBwdArgs)
    fn = lib.hfagp_planes_query_normals_bwd
    a.d_planes = 256
    assert fn(None, 256, 256, None) == -1
    assert fn(C.byref(a), None, None, None) == -1 and b"g_grad" in lib.hfagp_last_error()
    a.g_sigma = 256
    assert fn(C.byref(a), 256, None, None) == -1 and b"g_sigma" in lib.hfagp_last_error()
    a.g_sigma, a.g_rgb = None, 256
    assert fn(C.byref(a), 256, None, None) == -1
    a.g_rgb, a.d_coords = None, 256
    assert fn(C.byref(a), 256, None, None) == -1 and b"d_coords" in lib.hfagp_last_error()
    a.d_coords, a.d_dec_w0 = None, 256
    assert fn(C.byref(a), 256, None, None) == -1 and b"all or none" in lib.hfagp_last_error()
    a.d_dec_w0, a.d_planes = None, None
    assert fn(C.byref(a), 256, None, None) == -1 and b"at least one output" in lib.hfagp_last_error()
    a.d_planes, a.coords = 256, None
    assert fn(C.byref(a), None, 256, None) == -2 and b"grid" in lib.hfagp_last_error()
    a.coords, a.dec_w1 = 256, None
    assert fn(C.byref(a), None, 256, None) == -1


# ----------------------------------------------------------------------------- the two HIP units
@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.parametrize("unit,kernel,instances", UNITS, ids=[u for u, _, _ in UNITS])
def test_unit_resources(tmp_path, unit, kernel, instances):
    """Each unit on its own `units+=` line of build.sh; compiled with build.sh's flags, every kernel instance has no scratch and
    no spills, its LDS fits one workgroup per CU, and the unit holds no packed fp32 arithmetic."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(%s\)$" % unit, build, re.M), f"{unit}.hip is not on a units+= line of its own"
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    asm = tmp_path / "unit.s"
    out = subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", os.path.join(ROOT, "hfa-gp_amd", "csrc", unit + ".hip"), "-o", str(asm),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, set()
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and name and kernel in name:
            seen.add(name)
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name and kernel in name:
            assert int(m.group(1)) <= 160 * 1024, f"{name}: LDS {m.group(1)}"
    assert len(seen) == instances, seen
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", asm.read_text())


# ----------------------------------------------------------------------------- PLY and the CLI
def _mesh():
    rng = np.random.default_rng(1)
    v = rng.standard_normal((5, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)
    c = rng.integers(0, 256, (5, 3)).astype(np.uint8)
    n = rng.standard_normal((5, 3)).astype(np.float32)
    return v, f, c, n


def test_save_ply_round_trip_with_normals(tmp_path):
    from hfa_gp_amd.render import save_ply
    v, f, c, n = _mesh()
    for colors in (None, c):
        path = tmp_path / "m.ply"
        save_ply(path, torch.from_numpy(v), f, colors, torch.from_numpy(n))
        raw = path.read_bytes()
        head, body = raw.split(b"end_header\n", 1)
        props = [ln.split()[-1] for ln in head.decode().splitlines() if ln.startswith("property float") or ln.startswith("property uchar")]
        assert props == ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue"] if colors is not None else [])
        dt = [(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")] + ([(k, "u1") for k in "rgb"] if colors is not None else [])
        vert = np.frombuffer(body[:5 * np.dtype(dt).itemsize], dtype=dt)
        assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), v)
        assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), n)
        if colors is not None:
            assert np.array_equal(np.stack([vert["r"], vert["g"], vert["b"]], 1), c)
        face = np.frombuffer(body[5 * np.dtype(dt).itemsize:], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
        assert np.all(face["n"] == 3) and np.array_equal(face["idx"], f)
    with pytest.raises(ValueError):
        save_ply(tmp_path / "bad.ply", v, f, None, n[:4])


def test_save_ply_without_normals_is_byte_identical(tmp_path):
    """The file the writer produced before the keyword existed, built here by hand."""
    from hfa_gp_amd.render import save_ply
    v, f, c, _ = _mesh()
    for colors in (None, c):
        props = ["property float x", "property float y", "property float z"]
        dt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
        if colors is not None:
            props += ["property uchar red", "property uchar green", "property uchar blue"]
            dt += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        vert = np.empty(5, dtype=dt)
        for i, k in enumerate("xyz"):
            vert[k] = v[:, i]
        if colors is not None:
            for i, k in enumerate(("red", "green", "blue")):
                vert[k] = c[:, i]
        face = np.empty(2, dtype=[("n", "u1"), ("idx", "<i4", (3,))])
        face["n"], face["idx"] = 3, f
        header = ["ply", "format binary_little_endian 1.0", "element vertex 5", *props, "element face 2",
                  "property list uchar int vertex_indices", "end_header"]
        want = ("\n".join(header) + "\n").encode("ascii") + vert.tobytes() + face.tobytes()
        for kw in ({}, {"normals": None}):
            path = tmp_path / "m.ply"
            save_ply(path, v, f, colors, **kw)
            assert path.read_bytes() == want


def test_extract_shapes_cli_normals_flag():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import extract_shapes as X
    finally:
        sys.path.pop(0)
    a = X.build_parser().parse_args(["--seeds", "0", "--outdir", "o", "--format", "ply"])
    assert a.normals is False
    a = X.build_parser().parse_args(["--seeds", "0", "--outdir", "o", "--format", "both", "--normals", "--colors"])
    assert a.normals is True and a.colors is True
    assert "--normals" in X.build_parser().format_help() and "frame" in X.build_parser().format_help()
    # the vertex re-basing and the direction map agree: a world displacement maps to the same lattice direction
    n, cube = 9, 0.8
    verts = torch.tensor([[1.0, 2.0, 3.0], [4.0, 2.5, 0.5]])
    d = X.eg3d_to_world(verts[1:], n, cube) - X.eg3d_to_world(verts[:1], n, cube)
    back = X.world_to_eg3d_dir(d) / (cube / (n - 1))
    assert torch.allclose(back, verts[1:] - verts[:1], atol=1e-5)
