"""Marching cubes on the GPU (csrc/marching_cubes.hip, ops.marching_cubes, render.shape_mesh_eg3d, TriPlaneGenerator.extract_mesh,
HeadNeRF get_mesh, tools/extract_shapes.py --format ply) against the numpy reference of the contract (tests/mesh_ref.py).
Needs an MI355X:  python -m pytest tests -m gpu"""
import dataclasses
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests.mesh_ref import closed_manifold, mc_faces, mc_vertices, signed_volume_and_area
from tests.util import ROOT, perturb_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _mc(dev, vol, level, **kw):
    from hfa_gp_amd import ops
    with torch.no_grad():
        v, f = ops.marching_cubes(torch.as_tensor(vol).to(dev).contiguous(), level, **kw)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.device == dev and f.device == dev
    return v.cpu().numpy(), f.cpu().numpy()


def _smooth(rng, shape):
    g = np.meshgrid(*[np.linspace(0, 1, n) for n in shape], indexing="ij")
    v = np.zeros(shape)
    for _ in range(4):
        w = rng.uniform(2, 9, 3)
        ph = rng.uniform(0, 6.3, 3)
        v += np.sin(w[0] * g[0] + ph[0]) * np.cos(w[1] * g[1] + ph[1]) * np.sin(w[2] * g[2] + ph[2])
    return v.astype(np.float32)


def _shell(v, value=-5.0):
    v = v.copy()
    v[[0, -1]] = value
    v[:, [0, -1]] = value
    v[:, :, [0, -1]] = value
    return v


@pytest.mark.parametrize("shape", [(33, 47, 70), (2, 5, 64), (3, 66, 129)])
def test_vertices_and_faces_exact(dev, shape):
    """Vertices equal the numpy rebuild (crossed edges in contract order, the interpolation formula) and the faces equal the
    table's faces in contract order, for smooth and noise fields, with a non-trivial spacing and origin."""
    rng = np.random.default_rng(shape[2])
    spacing, origin = (0.5, 2.0, 0.25), (-3.0, 1.0, 7.0)
    for vol, level in ((_smooth(rng, shape), 0.1), (rng.standard_normal(shape).astype(np.float32), -0.2)):
        verts, faces = _mc(dev, vol, level, spacing=spacing, origin=origin)
        want = mc_vertices(vol, level, spacing, origin)
        extent = max(abs(o) + abs(s) * n for o, s, n in zip(origin, spacing, shape))
        assert verts.shape == want.shape
        assert np.abs(verts - want).max() <= 1e-6 * extent
        assert np.array_equal(faces, mc_faces(vol, level))


def test_nan_is_outside(dev):
    rng = np.random.default_rng(3)
    vol = rng.standard_normal((9, 8, 70)).astype(np.float32)
    vol[rng.random(vol.shape) < 0.1] = np.nan
    verts, faces = _mc(dev, vol, 0.0)
    want = mc_vertices(np.nan_to_num(vol, nan=-np.inf), 0.0)
    assert verts.shape == want.shape
    assert np.array_equal(faces, mc_faces(np.nan_to_num(vol, nan=-1.0), 0.0))


@pytest.mark.parametrize("shape", [(20, 30, 65), (6, 7, 130)])
def test_noise_faces_closed_manifold(dev, shape):
    """Random noise inside an outside boundary layer (every ambiguous case): indices in range, no repeated index, every vertex
    used, each face on the edges of one cube, each edge shared by two faces in opposite directions."""
    rng = np.random.default_rng(shape[0])
    vol = _shell(rng.standard_normal(shape).astype(np.float32))
    level = 0.05
    verts, faces = _mc(dev, vol, level)
    nv = verts.shape[0]
    assert faces.shape[0] > 1000 and faces.min() >= 0 and faces.max() < nv
    assert ((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])).all()
    assert (np.bincount(faces.reshape(-1), minlength=nv) > 0).all()
    # vertex -> owning point and axis, from the contract order
    n0, n1, n2 = shape
    inside = vol > level
    f = np.zeros(shape + (3,), bool)
    f[:-1, :, :, 0] = inside[:-1] != inside[1:]
    f[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    f[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    sel = np.nonzero(f.reshape(-1))[0]
    assert sel.size == nv                                              # counts[0] = number of crossed edges
    pt = sel // 3
    own = np.stack([pt // (n1 * n2), (pt // n2) % n1, pt % n2], 1)
    far = own + np.eye(3, dtype=np.int64)[sel % 3]
    lo = own[faces].min(1)                                             # the cube of each face
    for ends in (own[faces], far[faces]):
        d = ends - lo[:, None, :]
        assert ((d >= 0) & (d <= 1)).all()
    closed_manifold(faces, nv)


def _ball(c, r, n=64):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"))
    return r - np.sqrt(((g - np.asarray(c, np.float64)[:, None, None, None]) ** 2).sum(0))


def test_analytic_shapes(dev):
    n, r = 64, 20.0
    cases = [("sphere", _ball((31.3, 32.2, 30.6), r), 2),
             ("two spheres", np.maximum(_ball((16.5, 32, 31), 12), _ball((47.2, 32, 33), 12)), 4)]
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) - 31.7] * 3, indexing="ij"))
    torus = 7.0 - np.sqrt((np.sqrt(g[0] ** 2 + g[1] ** 2) - 18.0) ** 2 + g[2] ** 2)
    cases.append(("torus", torus, 0))
    for name, field, chi in cases:
        verts, faces = _mc(dev, field.astype(np.float32), 0.0)
        e = closed_manifold(faces, verts.shape[0])
        assert verts.shape[0] - e + faces.shape[0] == chi, name
        if name == "sphere":
            vol, area = signed_volume_and_area(verts, faces)
            assert abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01 and abs(area / (4 * np.pi * r ** 2) - 1) < 0.02, (vol, area)


def test_deterministic_and_empty(dev):
    from hfa_gp_amd import ops
    rng = np.random.default_rng(9)
    vol = torch.from_numpy(rng.standard_normal((40, 50, 200)).astype(np.float32)).to(dev)
    with torch.no_grad():
        a = ops.marching_cubes(vol, 0.3)
        b = ops.marching_cubes(vol, 0.3)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for v in (torch.ones(5, 6, 7, device=dev), -torch.ones(5, 6, 7, device=dev)):
            verts, faces = ops.marching_cubes(v, 0.0)
            assert verts.shape == (0, 3) and faces.shape == (0, 3)
        with pytest.raises(RuntimeError, match="CUDA"):
            ops.marching_cubes(torch.zeros(4, 4, 4), 0.0)
        with pytest.raises(RuntimeError, match="float32"):
            ops.marching_cubes(torch.zeros(4, 4, 4, device=dev, dtype=torch.float64), 0.0)
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.marching_cubes(torch.zeros(4, 4, 8, device=dev)[:, :, ::2], 0.0)
        with pytest.raises(RuntimeError, match="extent"):
            ops.marching_cubes(torch.zeros(4, 1, 8, device=dev), 0.0)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.marching_cubes(vol.clone().requires_grad_(True), 0.0)


def _gen(dev, preset):
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = dataclasses.replace(PRESETS[preset](), conv_precision="fp32")
    return cfg, perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)


def _trim(v):
    from hfa_gp_amd.render import _border_eg3d
    return _border_eg3d(v)


def _level(vol):
    n = vol.shape[-1]
    p = int(30 * n / 256)
    return float(vol[..., p:n - p, p:n - p, p:n - p].median())


def _crossed(inside):
    f = np.zeros(inside.shape + (3,), bool)
    f[:-1, :, :, 0] = inside[:-1] != inside[1:]
    f[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    f[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    return np.nonzero(f.reshape(-1))[0]


def _eg3d_vertex_of(inside):
    """index into EG3D's vertex list (volume E[a, b, c] = V[N-1-c, b, a]) of each vertex of V, by the edge both lie on"""
    n = inside.shape[0]
    sel = _crossed(inside)
    pt, axis = sel // 3, sel % 3
    i, j, k = pt // (n * n), (pt // n) % n, pt % n
    # V edge (i, j, k) + axis 0 is E's axis-2 edge owned by (k, j, N-2-i); axis 1 -> E axis 1 at (k, j, N-1-i); axis 2 -> E axis 0
    c = np.where(axis == 0, n - 2 - i, n - 1 - i)
    e_axis = 2 - axis
    slot = ((k * n + j) * n + c) * 3 + e_axis
    e_sel = _crossed(np.ascontiguousarray(np.flip(inside, 0).transpose(2, 1, 0)))
    idx = np.searchsorted(e_sel, slot)
    assert np.array_equal(e_sel[idx], slot)
    return idx


@pytest.mark.parametrize("preset,n", [("tiny64", 48), ("ffhq512_128", 64)])
def test_generator_extract_mesh(dev, preset, n):
    from hfa_gp_amd import ops
    from hfa_gp_amd.headnerf import _LatentBasis
    from hfa_gp_amd.render import shape_mesh_eg3d, to_uint8
    cfg, gen = _gen(dev, preset)
    ws = torch.randn(2, cfg.num_ws, cfg.w_dim, generator=torch.Generator().manual_seed(21)).to(dev)
    with torch.no_grad():
        vol = gen.density_grid(ws, resolution=n)
        level = _level(vol)
        meshes = gen.extract_mesh(ws, resolution=n, level=level, colors=True)
        cube = cfg.box_warp
        voxel = cube / (n - 1)
        planes, pam = gen._query_planes(ws)
        for b, m in enumerate(meshes):
            assert set(m) == {"vertices", "faces", "colors"}
            verts, faces = ops.marching_cubes(_trim(vol[b]), level, spacing=(voxel,) * 3, origin=(-cube / 2,) * 3)
            assert verts.shape[0] > 100
            assert torch.equal(m["vertices"], verts) and torch.equal(m["faces"], faces)
            rgb = ops.planes_query(planes[b:b + 1], verts[None], planes_absmax=pam, **gen._query_kwargs())[1][0]
            assert m["colors"].dtype == torch.uint8 and torch.equal(m["colors"], to_uint8(rgb[:, :3]))
            # EG3D's .ply geometry: the same vertex set under (a, b, c) <-> ((N-1-c) voxel - cube/2, b voxel - cube/2, a voxel - cube/2)
            ev, ef = shape_mesh_eg3d(vol[b], level=level)
            assert ev.shape == verts.shape and ef.shape == faces.shape
            a_, b_, c_ = ev.double().cpu().unbind(1)
            world = torch.stack([(n - 1 - c_) * voxel, b_ * voxel, a_ * voxel], 1) - cube / 2
            perm = _eg3d_vertex_of(_trim(vol[b]).cpu().numpy() > level)
            assert np.abs(world.numpy()[perm] - verts.double().cpu().numpy()).max() <= 1e-5 * cube
        basis = _LatentBasis()
        basis.generator = gen
        again = basis.get_mesh(ws, resolution=n, level=level)
        assert torch.equal(again[1]["vertices"], meshes[1]["vertices"]) and "colors" not in again[1]
    with pytest.raises(RuntimeError, match="no_grad"):
        gen.extract_mesh(ws.clone().requires_grad_(True), resolution=8)


def test_extract_shapes_cli_ply(dev, tmp_path):
    from hfa_gp_amd.config import tiny64
    from hfa_gp_amd.generator import load_G_official
    from hfa_gp_amd.render import shape_mesh_eg3d
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import extract_shapes as X
    finally:
        sys.path.pop(0)
    n = 40
    cfg = tiny64()
    gen = load_G_official(cfg=cfg, seed=0, weights=None, device=dev)
    with torch.no_grad():
        z = torch.from_numpy(np.random.RandomState(3).randn(1, cfg.z_dim)).float().to(dev)
        grid = gen.density_grid(gen.mapping(z, X.frontal_label(dev)), resolution=n)[0]
        level = _level(grid)
        verts, faces = shape_mesh_eg3d(grid, level=level)
    assert verts.shape[0] > 0
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_shapes.py"), "--preset", "tiny64", "--seeds", "3",
                          "--resolution", str(n), "--format", "ply", "--level", repr(level), "--colors", "--outdir",
                          str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    raw = (tmp_path / "seed0003.ply").read_bytes()
    header = raw[:raw.index(b"end_header\n")].decode().splitlines()
    assert f"element vertex {verts.shape[0]}" in header and f"element face {faces.shape[0]}" in header
    assert "property uchar red" in header
    assert not (tmp_path / "seed0003.mrc").exists()


def test_mesh_512_closed_manifold(dev):
    """A 512^3 ffhq512_128 head: the mesh is closed and edge-manifold (torch sorts on the GPU); prints the extraction time."""
    from hfa_gp_amd import ops
    cfg, gen = _gen(dev, "ffhq512_128")
    ws = torch.randn(1, cfg.num_ws, cfg.w_dim, generator=torch.Generator().manual_seed(5)).to(dev)
    n = 512
    with torch.no_grad():
        vol = _trim(gen.density_grid(ws, resolution=n)[0])
        level = _level(vol)
        ops.marching_cubes(vol, level)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verts, faces = ops.marching_cubes(vol, level)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    nv = verts.shape[0]
    print(f"\n512^3 marching cubes: {ms:.2f} ms, {nv} vertices, {faces.shape[0]} faces")
    assert nv > 10000
    f = faces.long()
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    d = torch.sort(a * nv + b).values
    assert not bool((d[1:] == d[:-1]).any())
    r = torch.sort(b * nv + a).values
    assert torch.equal(d, r)
    assert int(torch.bincount(f.reshape(-1), minlength=nv).min()) > 0
