"""Mesh tracing on the GPU (csrc/mesh_trace.hip, ops.trace_mesh, mesh.trace_mesh / mesh_maps) against `mesh.trace_mesh_reference`
in float32 on the CPU, whose bits both kernels must give.  Needs an MI355X:  python -m pytest tests -m gpu

1. the brute-force kernel is the reference: hit, face, front equal and t, bary, point, normal equal to the bit on every ray, random
   and adversarial (tests/mesh_trace_ref.adversarial_rays), for F around the LDS tile and B = 2 with shared and per-frame vertices;
2. the grid kernel is the brute-force kernel: every output equal at G = 1, 4, 7; two calls give the same bits;
3. `trace_mesh(differentiable=True)`: the kernel's forward values, the CPU float64 gradients under the project's gradient bar;
4. one generator case: extract_mesh -> TriangleMesh.from_dict -> mesh_maps on tiny64."""
import dataclasses
import os
import re

import pytest
import torch

from tests import mesh_trace_ref as M
from tests.normal_grad_ref import bar_ratio
from tests.util import ROOT, perturb_state

pytestmark = pytest.mark.gpu

TILE = int(re.search(r"constexpr int kMeshTile = (\d+);",
                     open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "mesh_trace.hip")).read()).group(1))
FLOATS, FLAGS = ("t", "bary", "point", "normal"), ("hit", "face", "front")
GRIDS = (1, 4, 7)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _assert_same(got, want, what):
    """every output equal; the float ones to the bit (−0 and +0 differ here)"""
    for k in FLAGS:
        assert torch.equal(got[k].cpu().to(want[k].dtype), want[k].cpu()), f"{what}: {k}"
    for k in FLOATS:
        g, w = _bits(got[k]), _bits(want[k])
        assert torch.equal(g, w), f"{what}: {k} differs on {int((g != w).sum())} of {g.numel()} entries"


def _topology(nf):
    """nf faces: the icosahedron's subdivisions where they have nf faces, otherwise the first nf of the 320 (an open surface)."""
    levels = {20: 0, 320: 2, 1280: 3}.get(nf)
    if levels is not None:
        return M.icosphere(levels)
    v, f = M.icosphere(0 if nf == 1 else 2)
    return v, f[:nf].contiguous()


def _run_case(dev, nf, per_frame, n_rays):
    from hfa_gp_amd import mesh
    v, f = _topology(nf)
    assert f.shape[0] == nf
    verts = M.second_frame(v) if per_frame else v[None]
    m = mesh.TriangleMesh(verts.to(dev), f.to(dev))
    assert m.tri.shape == (verts.shape[0], nf, 9)
    hits = 0
    for g in GRIDS:
        grid = m.build_grid(g)
        box = grid[2].cpu()
        rays = [M.adversarial_rays(verts[b if per_frame else 0], f, (box[b if per_frame else 0, :3], box[b if per_frame else 0, 3:]),
                                   g, seed=100 * g + b) for b in range(2)]
        n = rays[0][0].shape[0]
        # the eight special rays first, then an even pick of the rest; one ray: an ordinary one
        pick = torch.tensor([n - 1]) if n_rays == 1 else \
            torch.cat((torch.arange(8), 8 + torch.linspace(0, n - 9, n_rays - 8).round().long()))
        o, d, tn, tf = (torch.stack([r[k][pick] for r in rays]).contiguous() for k in range(4))
        assert o.shape == (2, n_rays, 3)
        want = mesh.trace_mesh_reference(verts, f, o, d, tn, tf)
        args = [t.to(dev) for t in (o, d, tn, tf)]
        m.grid = None
        brute = mesh.trace_mesh(m, *args)
        _assert_same(brute, want, f"brute force against the reference (G = {g} rays)")
        for k in FLOATS:                                                           # a miss: exact +0
            assert not bool(_bits(brute[k]).reshape(2, n_rays, -1)[~want["hit"]].any()), k
        m.grid = grid
        through = mesh.trace_mesh(m, *args)
        _assert_same(through, brute, f"grid G = {g} against brute force")
        _assert_same(mesh.trace_mesh(m, *args), through, f"grid G = {g}, second call")
        hits += int(want["hit"].sum())
        if n_rays > 8:
            assert not bool(want["hit"][:, :8].any())                              # the specials are misses whatever the mesh
    return hits


@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per-frame"])
@pytest.mark.parametrize("nf", [1, 20, 320, 1280, TILE - 1, TILE, TILE + 1])
def test_kernels_are_the_reference(dev, nf, per_frame):
    hits = _run_case(dev, nf, per_frame, 257)
    print(f"F = {nf}: {hits} hits over {len(GRIDS)} x 2 x 257 rays")
    assert hits >= (60 if nf >= 20 else 1)


@pytest.mark.parametrize("n_rays", [1, 64])
def test_kernels_are_the_reference_ray_counts(dev, n_rays):
    assert _run_case(dev, 320, True, n_rays) >= 1


def test_empty_inputs_launch_nothing(dev):
    from hfa_gp_amd import mesh, ops
    v, f = M.icosphere(0)
    m = mesh.TriangleMesh(v.to(dev), f.to(dev))
    m.build_grid(2)
    none = mesh.trace_mesh(m, torch.zeros(1, 0, 3, device=dev), torch.zeros(1, 0, 3, device=dev))
    assert none["t"].shape == (1, 0) and none["bary"].shape == (1, 0, 3)
    none = mesh.trace_mesh(m, torch.zeros(0, 5, 3, device=dev), torch.zeros(0, 5, 3, device=dev))
    assert none["face"].shape == (0, 5)
    o = torch.tensor([[[0.0, 0.0, 2.0]] * 3], device=dev)
    d = torch.tensor([[[0.0, 0.0, -1.0]] * 3], device=dev)
    empty = mesh.trace_mesh(mesh.TriangleMesh(v.to(dev), f[:0].to(dev)), o, d)
    assert not bool(empty["hit"].any()) and bool((empty["face"] == -1).all()) and not bool(empty["point"].any())
    only_t = ops.trace_mesh(m.tri, o, d, torch.zeros(1, 3, device=dev), torch.full((1, 3), 9.0, device=dev), grid=m.grid, want=("t",))
    assert set(only_t) == {"t"} and bool((only_t["t"] > 1.0).all())


def test_differentiable_forward_is_the_kernels_and_gradients_meet_float64(dev):
    """The case of tests/test_mesh_trace_cpu.py's gradient test: the float64 gradients are the CPU autograd of the closed form
    (held there to central differences); the device's float32 gradients must meet them under normal_grad_ref.bar_ratio <= 1."""
    from hfa_gp_amd import mesh
    v, f, o, d, coef = M.grad_case(torch.float64)
    v, o, d = (x.requires_grad_(True) for x in (v, o, d))
    ref = mesh.trace_mesh(mesh.TriangleMesh(v, f), o, d, differentiable=True, reference=True)
    want = torch.autograd.grad(M.grad_loss(ref, coef), [v, o, d])
    v32, f, o32, d32, _ = M.grad_case(torch.float32)
    vd, od, dd = (x.to(dev).requires_grad_(True) for x in (v32, o32, d32))
    for g in (None, 4):
        m = mesh.TriangleMesh(vd, f.to(dev))
        if g:
            m.build_grid(g)
        out = mesh.trace_mesh(m, od, dd, differentiable=True)
        plain = mesh.trace_mesh(m, od.detach(), dd.detach())
        _assert_same(out, plain, "differentiable forward")
        assert torch.equal(plain["face"].cpu(), ref["face"])
        loss = sum((out[k].reshape(2, 32, -1).double() * coef[k].to(dev)).sum() for k in coef)
        got = torch.autograd.grad(loss, [vd, od, dd])
        for name, a, b in zip(("vertices", "origins", "directions"), got, want):
            ratio = bar_ratio(a, b)
            print(f"grid {g}: d/d{name} bar ratio {ratio:.3e}")
            assert ratio <= 1.0
        assert bool((got[1][:, 30:] == 0).all()) and bool((got[2][:, 30:] == 0).all())        # a miss: exactly zero


def test_generator_mesh_maps_on_tiny64(dev):
    """extract_mesh(resolution=32) -> from_dict -> mesh_maps at a synthesis label: the mask is non-empty, and every hit's point is
    Σ bary·vertices of its face to 1e-5 of the cube side.  (How close the depth is to `trace_rays` is measured, not asserted:
    profiles/mesh_trace/README.md.)"""
    from hfa_gp_amd import mesh
    from hfa_gp_amd.cam_utils import cam_sampler, ray_grid
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    from hfa_gp_amd.headnerf import flip_label_
    cfg = dataclasses.replace(PRESETS["tiny64"](), conv_precision="fp32")
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    ws = torch.randn(1, cfg.num_ws, cfg.w_dim, generator=torch.Generator().manual_seed(21)).to(dev)
    torch.manual_seed(5)
    c = flip_label_(cam_sampler(1, "cpu")).to(dev)
    n, res = 32, cfg.neural_rendering_resolution
    with torch.no_grad():
        vol = gen.density_grid(ws, resolution=n)
        p = int(30 * n / 256)
        level = float(vol[..., p:n - p, p:n - p, p:n - p].median())
        m = mesh.TriangleMesh.from_dict(gen.extract_mesh(ws, resolution=n, level=level)[0])
    assert m.num_faces > 0
    m.build_grid()
    maps = mesh.mesh_maps(m, c, res)
    assert maps["depth"].shape == (1, 1, res, res) and maps["normal"].shape == (1, 3, res, res) and maps["face"].shape == (1, res, res)
    mask = maps["mask"][0, 0] > 0
    print(f"{m.num_faces} faces, G = {m.grid[3]}: {int(mask.sum())} of {res * res} pixels hit")
    assert int(mask.sum()) > 0
    o, d = ray_grid(c, res)
    out = mesh.trace_mesh(m, o, d)
    assert torch.equal(out["t"].reshape(1, 1, res, res), maps["depth"])
    again = m.interpolate(m.vertices, out)
    err = float((again - out["point"])[out["hit"]].abs().max())
    print(f"max |point - sum bary vertices| = {err:.3e} (cube side {cfg.box_warp})")
    assert err <= 1e-5 * cfg.box_warp
