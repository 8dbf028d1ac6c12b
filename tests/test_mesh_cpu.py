"""Mesh export without a GPU: the marching-cubes case table (generated, closed and oriented on random volumes through the numpy
reference), the C ABI of hfagp_marching_cubes_* (binding, argument validation), the unit's build-time resources, the PLY
writer and the CLI's arguments."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.mesh_ref import MC_SRC, closed_manifold, mc_faces, mc_table, mc_vertices
from tests.util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HAVE_HIPCC = os.path.exists(HIPCC) or bool(shutil.which("hipcc"))


def _gen_module():
    sys.path.insert(0, os.path.join(ROOT, "tools", "dev"))
    try:
        import gen_mc_table
    finally:
        sys.path.pop(0)
    return gen_mc_table


def test_table_is_the_generated_one():
    src = open(MC_SRC).read()
    block = re.search(r"// mc-table begin.*?// mc-table end\n", src, re.S).group(0)
    assert block == _gen_module().c_block()


def test_table_single_corner_cases():
    counts, edges = mc_table()
    assert counts[0] == 0 and counts[255] == 0
    assert counts[1] == 1 and list(edges[1, :3]) == [0, 4, 8]         # corner 0 inside: normal toward +(1, 1, 1)
    assert counts[254] == 1 and list(edges[254, :3]) == [0, 8, 4]     # its complement: reversed
    assert counts.max() <= edges.shape[1] // 3


@pytest.mark.parametrize("shape", [(9, 10, 11), (4, 17, 6), (12, 3, 30)])
def test_reference_noise_meshes_closed_and_oriented(shape):
    """Random noise with an outside boundary layer visits the ambiguous cases: the table's mesh is closed, each edge bounds two
    faces in opposite directions, every vertex is used, no face repeats a vertex."""
    rng = np.random.default_rng(sum(shape))
    for _ in range(4):
        v = rng.standard_normal(shape).astype(np.float32)
        v[[0, -1]] = -1
        v[:, [0, -1]] = -1
        v[:, :, [0, -1]] = -1
        verts, faces = mc_vertices(v, 0.1), mc_faces(v, 0.1)
        assert faces.shape[0] > 0
        closed_manifold(faces, verts.shape[0])
        assert (np.bincount(faces.reshape(-1), minlength=verts.shape[0]) > 0).all()
        assert ((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])).all()


def test_every_case_closes_in_isolation():
    """Each of the 256 cases alone inside an outside shell (a 4^3 volume, one cube of interior) gives a closed, oriented mesh
    with positive signed volume."""
    from tests.mesh_ref import signed_volume_and_area
    for case in range(1, 256):
        v = np.full((4, 4, 4), -1.0, dtype=np.float32)
        for c in range(8):
            if case >> c & 1:
                v[1 + (c >> 2 & 1), 1 + (c >> 1 & 1), 1 + (c & 1)] = 1.0
        verts, faces = mc_vertices(v, 0.0), mc_faces(v, 0.0)
        closed_manifold(faces, verts.shape[0])
        assert signed_volume_and_area(verts, faces)[0] > 0, case


@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_marching_cubes_binding_matches_header(lib):
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} HfagpMarchingCubesArgs;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"\[\d+\]", "", body)
    names = [re.findall(r"\w+", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in lib.MarchingCubesArgs._fields_]
    assert lib.ABI_VERSION == 15
    for name in ("hfagp_marching_cubes_count", "hfagp_marching_cubes_emit", "hfagp_marching_cubes_workspace_bytes"):
        assert name in lib.SYMBOLS


def test_marching_cubes_argument_validation(lib):
    h = lib.lib()
    assert h.hfagp_marching_cubes_workspace_bytes(512, 512, 512) == 2 * 8 * 512 * 512        # 4 MB at 512^3
    assert h.hfagp_marching_cubes_count(None, None) == -1
    assert b"null pointer" in h.hfagp_last_error()
    a = lib.MarchingCubesArgs()
    assert h.hfagp_marching_cubes_count(C.byref(a), None) == -1
    assert h.hfagp_marching_cubes_emit(C.byref(a), None) == -1
    a.volume, a.workspace, a.counts = 8, 8, 8       # non-null, never dereferenced: extents are rejected first
    a.n0, a.n1, a.n2 = 2, 1, 5
    assert h.hfagp_marching_cubes_count(C.byref(a), None) == -1
    assert b"bad extents" in h.hfagp_last_error()
    a.n0, a.n1, a.n2 = 4, 4, 4
    a.workspace_bytes = h.hfagp_marching_cubes_workspace_bytes(4, 4, 4) - 8
    assert h.hfagp_marching_cubes_emit(C.byref(a), None) == -1
    assert b"workspace" in h.hfagp_last_error()
    a.workspace_bytes += 8
    a.workspace = 12
    assert h.hfagp_marching_cubes_count(C.byref(a), None) == -1                              # misaligned workspace
    assert b"aligned" in h.hfagp_last_error()


def _build_flags():
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    return build, re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_marching_cubes_kernel_resources(tmp_path):
    """In build.sh's unit list; compiled with build.sh's flags: no scratch, no spills, no packed fp32 arithmetic."""
    build, flags = _build_flags()
    assert re.search(r"^units\+=\(.*\bmarching_cubes\b", build, re.M), "marching_cubes.hip is not in build.sh's unit list"
    src = os.path.join(ROOT, "hfa-gp_amd", "csrc", "marching_cubes.hip")
    out = subprocess.run([HIPCC, *flags, "-c", src, "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, set()
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and name and "mc_" in name:
            seen.add(name)
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert len(seen) == 3, seen          # count, scan, emit
    asm = tmp_path / "mc.s"
    out = subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", src, "-o", str(asm)], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = asm.read_text()
    assert "mc_emit_kernel" in text
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)


def _read_ply(path):
    """tiny binary little-endian PLY reader: header lines, vertex record array, faces [F, 3]"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    nv = int(next(h for h in header if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in header if h.startswith("element face")).split()[-1])
    props = [h.split()[-1] for h in header if h.startswith("property") and "list" not in h]
    types = {"float": "<f4", "uchar": "u1"}
    dt = np.dtype([(h.split()[-1], types[h.split()[1]]) for h in header if h.startswith("property") and "list" not in h])
    assert dt.names == tuple(props)
    vert = np.frombuffer(raw, dtype=dt, count=nv, offset=end)
    fdt = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
    face = np.frombuffer(raw, dtype=fdt, count=nf, offset=end + nv * dt.itemsize)
    assert end + nv * dt.itemsize + nf * fdt.itemsize == len(raw)
    assert (face["n"] == 3).all()
    return header, vert, face["idx"]


def test_save_ply_header_and_round_trip(tmp_path):
    from hfa_gp_amd.render import save_ply
    rng = np.random.default_rng(1)
    verts = rng.standard_normal((7, 3)).astype(np.float32)
    faces = rng.integers(0, 7, (5, 3)).astype(np.int32)
    save_ply(tmp_path / "m.ply", verts, faces)
    header, v, f = _read_ply(tmp_path / "m.ply")
    assert header == ["ply", "format binary_little_endian 1.0", "element vertex 7", "property float x", "property float y",
                      "property float z", "element face 5", "property list uchar int vertex_indices", "end_header"]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), verts) and np.array_equal(f, faces)
    colors = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    import torch
    save_ply(tmp_path / "c.ply", torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(colors))
    header, v, f = _read_ply(tmp_path / "c.ply")
    assert header[3:9] == ["property float x", "property float y", "property float z", "property uchar red",
                           "property uchar green", "property uchar blue"]
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), colors) and np.array_equal(f, faces)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), verts)
    save_ply(tmp_path / "e.ply", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    header, v, f = _read_ply(tmp_path / "e.ply")
    assert len(v) == 0 and len(f) == 0 and "element face 0" in header
    with pytest.raises(ValueError):
        save_ply(tmp_path / "x.ply", verts, faces, colors.astype(np.float32))


def test_extract_shapes_cli_mesh_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import extract_shapes as X
    finally:
        sys.path.pop(0)
    a = X.build_parser().parse_args(["--seeds", "0", "--outdir", "o"])
    assert a.format == "mrc" and a.level == 10.0 and a.colors is False
    a = X.build_parser().parse_args(["--seeds", "0", "--outdir", "o", "--format", "ply", "--level", "5", "--colors"])
    assert a.format == "ply" and a.level == 5.0 and a.colors is True
    with pytest.raises(SystemExit):
        X.build_parser().parse_args(["--seeds", "0", "--outdir", "o", "--format", "obj"])
    import torch
    n, cube = 5, 1.0
    w = X.eg3d_to_world(torch.tensor([[0.0, 1.0, 4.0]]), n, cube)
    assert torch.allclose(w, torch.tensor([[0.0 * 0.25 - 0.5, 0.25 - 0.5, 0.0 - 0.5]]))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_shapes.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--format", "--level", "--colors"):
        assert flag in out.stdout
