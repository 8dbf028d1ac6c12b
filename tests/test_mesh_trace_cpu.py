"""Mesh tracing without a GPU: `mesh.trace_mesh_reference` (the definition) on analytic cases, the no-cracks property, float32
against float64, the grid builder, the gradient of `trace_mesh(differentiable=True)`, `interpolate` / `mesh_maps`, the C surface of
hfagp_trace_mesh and the unit's build-time resources."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import mesh_trace_ref as M
from tests.normal_grad_ref import bar_ratio
from tests.util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F32, F64 = torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")


def _mesh_mod():
    from hfa_gp_amd import mesh
    return mesh


# ----------------------------------------------------------------------------- 1. analytic cases
TRI_V = [[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]          # N = (0, 0, 1)


def _one(dtype, verts, faces, o, d, tn=0.0, tf=INF):
    mesh = _mesh_mod()
    out = mesh.trace_mesh_reference(torch.tensor(verts, dtype=dtype), torch.tensor(faces), torch.tensor([[o]], dtype=dtype),
                                    torch.tensor([[d]], dtype=dtype), tn, tf)
    return {k: v[0, 0] for k, v in out.items()}


def _assert_miss(out):
    assert not bool(out["hit"]) and int(out["face"]) == -1 and not bool(out["front"])
    for k in ("t", "bary", "point", "normal"):
        assert bool((out[k] == 0).all()) and not bool(torch.signbit(out[k]).any()), k


@pytest.mark.parametrize("dtype", [F32, F64])
def test_single_triangle_by_hand(dtype):
    """o = (1/4, 1/4, 2), d = (0, 0, −2): dn = −2, dot(A, N) = −1, t = 1/2; the point (1/4, 1/4, 1) has weights (1/2, 1/4, 1/4);
    every number is a dyadic fraction, so the results are exact in both dtypes."""
    out = _one(dtype, TRI_V, [[0, 1, 2]], [0.25, 0.25, 2.0], [0.0, 0.0, -2.0])
    assert bool(out["hit"]) and int(out["face"]) == 0 and bool(out["front"])
    assert out["face"].dtype == torch.int32 and out["t"].dtype == dtype
    assert float(out["t"]) == 0.5
    assert out["bary"].tolist() == [0.5, 0.25, 0.25]
    assert out["point"].tolist() == [0.25, 0.25, 1.0]
    assert out["normal"].tolist() == [0.0, 0.0, 1.0]


@pytest.mark.parametrize("dtype", [F32, F64])
def test_back_face_parallel_degenerate_and_limits(dtype):
    # from below: the same hit, two-sided, the normal still the winding's
    out = _one(dtype, TRI_V, [[0, 1, 2]], [0.25, 0.25, 0.0], [0.0, 0.0, 2.0])
    assert bool(out["hit"]) and not bool(out["front"]) and float(out["t"]) == 0.5
    assert out["bary"].tolist() == [0.5, 0.25, 0.25] and out["normal"].tolist() == [0.0, 0.0, 1.0]
    # parallel to the plane, in it and above it
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], [-1.0, 0.25, 1.0], [1.0, 0.0, 0.0]))
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], [-1.0, 0.25, 2.0], [1.0, 0.0, 0.0]))
    # a zero-area face is never a hit: two equal vertices, three collinear ones
    _assert_miss(_one(dtype, TRI_V, [[0, 0, 2]], [0.0, 0.5, 2.0], [0.0, 0.0, -1.0]))
    _assert_miss(_one(dtype, [[0.0, 0.0, 1.0], [0.5, 0.0, 1.0], [1.0, 0.0, 1.0]], [[0, 1, 2]], [0.25, 0.0, 2.0], [0.0, 0.0, -1.0]))
    # the limits cut the hit off on either side, inclusive at both ends; a NaN limit; a zero and a NaN direction
    ray = ([0.25, 0.25, 2.0], [0.0, 0.0, -2.0])
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], *ray, tn=0.625))
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], *ray, tf=0.375))
    assert bool(_one(dtype, TRI_V, [[0, 1, 2]], *ray, tn=0.5)["hit"]) and bool(_one(dtype, TRI_V, [[0, 1, 2]], *ray, tf=0.5)["hit"])
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], *ray, tn=NAN))
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], *ray, tf=NAN))
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], *ray, tn=1.0, tf=0.0))
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], ray[0], [0.0, 0.0, 0.0]))
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], ray[0], [NAN, 0.0, -1.0]))
    # behind the origin: t < t_near = 0 — and found with a negative t_near
    _assert_miss(_one(dtype, TRI_V, [[0, 1, 2]], ray[0], [0.0, 0.0, 2.0]))
    assert float(_one(dtype, TRI_V, [[0, 1, 2]], ray[0], [0.0, 0.0, 2.0], tn=-1.0)["t"]) == -0.5


@pytest.mark.parametrize("dtype", [F32, F64])
def test_ties_go_to_the_lower_index_and_nearer_faces_win(dtype):
    verts = TRI_V + [[0.0, 0.0, 1.5], [1.0, 0.0, 1.5], [0.0, 1.0, 1.5]]
    ray = ([0.25, 0.25, 2.0], [0.0, 0.0, -1.0])
    # the nearer plane z = 1.5 wins wherever it stands in the list; two coplanar copies: the lower index
    assert int(_one(dtype, verts, [[0, 1, 2], [3, 4, 5]], *ray)["face"]) == 1
    assert int(_one(dtype, verts, [[3, 4, 5], [0, 1, 2]], *ray)["face"]) == 0
    out = _one(dtype, verts, [[0, 1, 2], [3, 4, 5], [3, 4, 5], [0, 1, 2]], *ray)
    assert int(out["face"]) == 1 and float(out["t"]) == 0.5
    # the chunked run (every pair a chunk of its own) gives the same
    mesh = _mesh_mod()
    v, f = M.icosphere(1, dtype=dtype)
    g = torch.Generator().manual_seed(0)
    o = torch.tensor([0.1, 0.2, 1.5], dtype=dtype).expand(1, 9, 3).contiguous()
    d = (torch.rand(1, 9, 3, generator=g, dtype=dtype) - 0.5) * 0.8 - o
    a, b = mesh.trace_mesh_reference(v, f, o, d), mesh.trace_mesh_reference(v, f, o, d, max_pairs=7)
    assert int(a["hit"].sum()) >= 5
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_reference_argument_errors():
    mesh = _mesh_mod()
    v, f = M.icosphere(0)
    o = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError, match=r"\[B, R, 3\]"):
        mesh.trace_mesh_reference(v, f, o[0], o[0])
    with pytest.raises(ValueError, match="share a dtype"):
        mesh.trace_mesh_reference(v.double(), f, o, o)
    with pytest.raises(ValueError, match="must index"):
        mesh.TriangleMesh(v, f + 1)
    with pytest.raises(ValueError, match="finite"):
        mesh.TriangleMesh(v * INF, f)
    with pytest.raises(ValueError, match="int32 / int64"):
        mesh.TriangleMesh(v, f.float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.trace_mesh(mesh.TriangleMesh(v, f), o, o)
    empty = mesh.trace_mesh(mesh.TriangleMesh(v, f[:0]), o, o + 1, reference=True)
    assert not bool(empty["hit"].any()) and bool((empty["face"] == -1).all()) and empty["bary"].shape == (1, 4, 3)


# ----------------------------------------------------------------------------- 2. no cracks along edges
def test_no_cracks_along_the_edges_of_an_icosphere():
    """float32, 1280 faces, three interior origins: every ray aimed exactly at an edge midpoint or at the quarter point of an edge
    must hit — the edge functions of the two faces at an edge are negated bits of each other.  Rays aimed at vertices are the one
    known leak: their misses are printed, not asserted."""
    mesh = _mesh_mod()
    v, f = M.icosphere(3)
    assert f.shape[0] == 1280
    e = M.edges(f)
    assert e.shape[0] == 1920
    mids, quarter = 0.5 * (v[e[:, 0]] + v[e[:, 1]]), v[e[:, 0]] + 0.25 * (v[e[:, 1]] - v[e[:, 0]])
    for origin in ([0.0, 0.0, 0.0], [0.11, -0.07, 0.19], [-0.23, 0.17, 0.05]):
        o = torch.tensor(origin, dtype=F32)
        for name, target in (("edge midpoints", mids), ("edge quarter points", quarter)):
            d = (target - o)[None].contiguous()
            out = mesh.trace_mesh_reference(v, f, o.expand_as(d).contiguous(), d)
            missed = int((~out["hit"]).sum())
            print(f"origin {origin}: {missed} of {d.shape[1]} rays aimed at {name} missed")
            assert missed == 0
        d = (v - o)[None].contiguous()
        out = mesh.trace_mesh_reference(v, f, o.expand_as(d).contiguous(), d)
        print(f"origin {origin}: {int((~out['hit']).sum())} of {d.shape[1]} rays aimed at vertices missed (the known leak)")


# ----------------------------------------------------------------------------- 3. float32 against float64
U32 = 2.0 ** -24


def _f32_vs_f64(verts, faces, c, res):
    """float32 against float64 on `ray_grid`'s rays of the labels c, the float32 inputs taken exactly into float64.

    Left out (by the float64 run): rays with min |bary| < 1e-4, |dn| / (|d| |N|) < 1e-3, t within 1e-5 of a limit or of a second
    candidate; their share must stay below 2 %.  "min |bary| < 1e-4" is taken over EVERY face the ray passes within 1e-4 of the
    boundary of, inside or outside (all three weights > −1e-4, the smallest < 1e-4, t not behind the origin), not over the winner
    alone: on a mesh with open edges a ray that float64 sends 1e-7 past the edge of a nearer face is as undecided as one that
    just hits it (on a closed mesh the two readings leave out the same rays, up to the silhouette).  The threshold presumes faces
    large enough for it: the bound on bary below, 42u S² / (|N||cos|), is 1e-5 / |cos| for the 1280-face sphere of radius 0.5 seen
    from 2.7 and 4e-5 / |cos| for radius 0.25, where rays 1.1e-4 inside an edge change face — hence these meshes.  On the rest hit and face are equal, and the errors of t and bary are held to a
    bound from the rounding of a − o and what follows from it, u = 2^-24, first order in u:
      * every component of A, B, C, b − a, c − a carries one rounding (relative u); a component x1 y2 − x2 y1 of a cross product
        adds one per product and one for the difference: |δ cross(x, y)| <= sqrt(3) · 4u |x||y| <= 7u |x||y| — relative to |x||y|,
        not to the cross product itself (cancellation);
      * a dot product adds 3u Σ|x_k y_k|: with S = max(|A|, |B|, |C|) and P = |b − a||c − a| >= |N|,
          |δU| <= 10u |d| S²,  |δdet| <= 32u |d| S²,  |δ dot(A, N)| <= 11u S P,  |δdn| <= 10u |d| P;
      * quotients: bary = U / det, |bary| <= 1, det = dn up to rounding:
          |δbary| <= (10 + 32) u |d| S² / |det| + u;    t = dot(A, N) / dn with |t||d| <= S (the hit lies in the face):
          |δt|    <= (11 + 10) u S P / |dn| + u |t|.
      With |det| ~ |dn| = |d||N||cos| these are eps · scale / |cosine|, the scale S² / |N| for bary and S P / (|d||N|) for t.  The
      relative change of the denominators is rho = 32u |d| S² / |det|; the bounds are divided by 1 − rho, and a ray with
      rho >= 1/2 (a grazing hit of a small face far away) is outside the first-order argument: it joins the rays left out, under
      the same 2 % cap (none here).  Every other hit is held to both bounds."""
    from hfa_gp_amd.cam_utils import ray_grid
    mesh = _mesh_mod()
    o, d = ray_grid(c, res)
    lo, hi_ = mesh.trace_mesh_reference(verts, faces, o, d), mesh.trace_mesh_reference(verts.double(), faces, o.double(), d.double())
    # ---- the float64 picture of every (ray, face) pair: second candidates
    tri = verts.double()[faces]                                                             # [F, 3, 3]
    b = o.shape[0]
    second = torch.full(o.shape[:2], INF, dtype=F64)
    near_any = torch.zeros(o.shape[:2], dtype=torch.bool)
    for f in range(b):
        U, V, W, det, N, dn, t = mesh._face_terms(o[f, :, None].double(), d[f, :, None].double(), tri[None, :, 0], tri[None, :, 1],
                                                  tri[None, :, 2])
        cand = mesh._candidate(U, V, W, det, dn, t, 0.0, INF)
        bmin = (torch.stack((U, V, W), -1) / det[..., None]).amin(-1)
        near_any[f] = ((bmin > -1e-4) & (bmin < 1e-4) & (dn != 0) & (t >= -1e-5)).any(1)
        cand[torch.arange(o.shape[1]), hi_["face"][f].clamp(min=0).long()] = False
        second[f] = torch.where(cand, t, torch.full_like(t, INF)).min(1).values
    hit = hi_["hit"]
    ids = faces[hi_["face"].clamp(min=0).long()]
    a_, b_, c_ = (verts.double()[ids[..., k]] for k in range(3))
    U, V, W, det, N, dn, t = mesh._face_terms(o.double(), d.double(), a_, b_, c_)
    dlen = d.double().norm(dim=-1)
    cos = dn.abs() / (dlen * N.norm(dim=-1))
    near_edge = near_any | (hit & (hi_["bary"].abs().amin(-1) < 1e-4))
    S = torch.stack(((a_ - o.double()).norm(dim=-1), (b_ - o.double()).norm(dim=-1), (c_ - o.double()).norm(dim=-1))).amax(0)
    P = (b_ - a_).norm(dim=-1) * (c_ - a_).norm(dim=-1)
    rho = 32 * U32 * dlen * S * S / det.abs()
    unbounded = hit & ~(rho < 0.5)
    out = near_edge | (hit & (cos < 1e-3)) | (hit & (t.abs() < 1e-5)) | (hit & ((second - t).abs() < 1e-5)) | unbounded
    share = float(out.double().mean())
    print(f"left out {int(out.sum())} of {out.numel()} rays ({share:.2e}); near an edge alone {float(near_edge.double().mean()):.2e}; "
          f"rho >= 1/2 alone {int(unbounded.sum())}; {int(hit.sum())} hits")
    assert share <= 0.02
    keep = ~out
    assert int((hit & keep).sum()) >= 0.02 * out.numel()
    assert torch.equal(lo["hit"][keep], hit[keep])
    assert torch.equal(lo["face"][keep], hi_["face"][keep])
    assert torch.equal(lo["front"][keep], hi_["front"][keep])
    k = hit & keep                                                                           # EVERY kept hit is held to the bounds
    bound_b = (42 * U32 * dlen * S * S / det.abs() + U32) / (1 - rho)
    bound_t = (21 * U32 * S * P / dn.abs() + U32 * t.abs()) / (1 - rho)
    err_b = (lo["bary"].double() - hi_["bary"]).abs().amax(-1)
    err_t = (lo["t"].double() - hi_["t"]).abs()
    print(f"{int(k.sum())} kept hits; max |dt| {float(err_t[k].max()):.3e}, max |dt| / bound {float((err_t / bound_t)[k].max()):.3f}; "
          f"max |dbary| {float(err_b[k].max()):.3e}, max |dbary| / bound {float((err_b / bound_b)[k].max()):.3f}")
    assert bool((err_t[k] <= bound_t[k]).all())
    assert bool((err_b[k] <= bound_b[k]).all())


def _labels(n):
    from hfa_gp_amd.cam_utils import cam_sampler
    from hfa_gp_amd.headnerf import flip_label_
    torch.manual_seed(11)
    return flip_label_(cam_sampler(n, "cpu"))                      # the label as the generator is fed it: looking at the head


def test_float32_against_float64_icosphere():
    v, f = M.icosphere(3)
    _f32_vs_f64(v, f, _labels(2), 64)


def test_float32_against_float64_slivers():
    v, f = M.sliver_mesh(300, seed=5)
    _f32_vs_f64(v, f, _labels(2), 64)


# ----------------------------------------------------------------------------- 4. the grid builder
@pytest.mark.parametrize("g", [1, 4, 7])
def test_grid_builder(g):
    mesh = _mesh_mod()
    v, f = M.icosphere(2)
    m = mesh.TriangleMesh(M.second_frame(v), f)
    cell_start, cell_faces, box, gg = m.build_grid(g)
    assert gg == g and cell_start.shape == (2, g ** 3 + 1) and cell_start.dtype == torch.int32 and cell_faces.dtype == torch.int32
    assert box.shape == (2, 6) and box.dtype == F32
    flat = cell_start.reshape(-1).long()
    assert int(flat[0]) == 0 and int(flat[-1]) == cell_faces.shape[0] and bool((flat[1:] >= flat[:-1]).all())
    assert int(cell_start[0, -1]) == int(cell_start[1, 0])
    assert bool((cell_faces >= 0).all()) and bool((cell_faces < f.shape[0]).all())
    tri = m.tri.reshape(2, -1, 3, 3).double()
    for fr in range(2):
        lo, cell = box[fr, :3].double(), box[fr, 3:].double()
        planes = lo[None] + torch.arange(g + 1, dtype=F64)[:, None] * cell[None]              # [G+1, 3]
        assert bool((tri[fr].amin((0, 1)) > planes[0]).all()) and bool((tri[fr].amax((0, 1)) < planes[-1]).all())
        member = torch.zeros(g ** 3, f.shape[0], dtype=torch.bool)
        for cidx in range(g ** 3):
            s, e = int(cell_start[fr, cidx]), int(cell_start[fr, cidx + 1])
            lst = cell_faces[s:e].long()
            assert bool((lst[1:] > lst[:-1]).all())                                            # sorted, no duplicates
            member[cidx, lst] = True
        # every face is in every cell its unpadded box touches (closed intervals, the kernel's planes taken into float64)
        fmin, fmax = tri[fr].amin(1), tri[fr].amax(1)                                          # [F, 3]
        touch = torch.ones(g, g, g, f.shape[0], dtype=torch.bool)
        for k in range(3):
            ok = (fmax[None, :, k] >= planes[:-1, k, None]) & (fmin[None, :, k] <= planes[1:, k, None])     # [G, F]
            shape = [1, 1, 1, f.shape[0]]
            shape[k] = g
            touch &= ok.reshape(shape)
        touch = touch.reshape(g ** 3, -1)
        assert bool((member | ~touch).all())
        print(f"G = {g} frame {fr}: {int(member.sum())} pairs, {int(touch.sum())} from the unpadded boxes")
    again = mesh.TriangleMesh(M.second_frame(v), f).build_grid(g)
    assert all(torch.equal(x, y) for x, y in zip((cell_start, cell_faces, box), again[:3]))


def test_grid_builder_limits():
    mesh = _mesh_mod()
    v, f = M.icosphere(1)
    m = mesh.TriangleMesh(v, f)
    with pytest.raises(ValueError, match="max_pairs"):
        m.build_grid(4, max_pairs=79)
    assert m.grid is None
    with pytest.raises(ValueError, match="resolution"):
        m.build_grid(0)
    with pytest.raises(ValueError, match="resolution"):
        m.build_grid(257)
    m.build_grid(1, max_pairs=80)
    assert m.grid[1].tolist() == list(range(80))
    assert m.build_grid()[3] == mesh._default_resolution(80)
    flat = mesh.TriangleMesh(torch.tensor(TRI_V), torch.tensor([[0, 1, 2]])).build_grid(3)        # no extent along z
    assert bool((flat[2][:, 3:] > 0).all())


# ----------------------------------------------------------------------------- 5. the gradient
def test_differentiable_gradient_against_float64_central_differences():
    """L = Σ c·(t, bary, point) over 2 x 32 rays (two misses per frame) on an 80-face sphere, per-frame vertices.  The float64
    yardstick is the central difference of the float64 reference along random directions in the vertices, the origins and the
    directions (eps = 1e-6: the hit faces do not change, the truncation error is ~eps² for this rational function); the float32
    gradients of `trace_mesh(differentiable=True)` must meet it under the project's gradient bar (normal_grad_ref.bar_ratio <= 1),
    as directional derivatives and, against the float64 autograd of the same closed form, element by element."""
    mesh = _mesh_mod()
    grads = {}
    for dtype in (F32, F64):
        v, f, o, d, coef = M.grad_case(dtype)
        v, o, d = (x.clone().requires_grad_(True) for x in (v, o, d))
        out = mesh.trace_mesh(mesh.TriangleMesh(v, f), o, d, differentiable=True, reference=True)
        plain = mesh.trace_mesh(mesh.TriangleMesh(v.detach(), f), o.detach(), d.detach(), reference=True)
        assert all(torch.equal(out[k].detach(), plain[k]) for k in plain)                     # the forward values are untouched
        assert int(out["hit"].sum()) == 60 and not out["normal"].requires_grad
        grads[dtype] = torch.autograd.grad(M.grad_loss(out, coef), [v, o, d])
        for gv in grads[dtype][1:]:
            assert bool((gv[:, 30:] == 0).all())                                               # a miss: exactly zero
    v, f, o, d, coef = M.grad_case(F64)
    base = mesh.trace_mesh_reference(v, f, o, d)
    g = torch.Generator().manual_seed(22)
    eps = 1e-6
    for trial in range(3):
        D = [torch.randn(x.shape, generator=g, dtype=F64) for x in (v, o, d)]
        fd = []
        for i in range(3):
            vals = []
            for s in (1.0, -1.0):
                args = [x + (s * eps * D[j] if j == i else 0.0) for j, x in enumerate((v, o, d))]
                out = mesh.trace_mesh_reference(args[0], f, args[1], args[2])
                assert torch.equal(out["face"], base["face"])
                vals.append(float(M.grad_loss(out, coef)))
            fd.append((vals[0] - vals[1]) / (2 * eps))
        for dtype in (F32, F64):
            got = torch.tensor([float((gv.double() * Dv).sum()) for gv, Dv in zip(grads[dtype], D)])
            ratio = bar_ratio(got, torch.tensor(fd))
            print(f"trial {trial} {dtype}: directional derivatives {got.tolist()} against differences {fd}: bar ratio {ratio:.3e}")
            assert ratio <= 1.0
    for name, a, b in zip(("vertices", "origins", "directions"), grads[F32], grads[F64]):
        ratio = bar_ratio(a, b)
        print(f"d/d{name}: float32 against float64 autograd, bar ratio {ratio:.3e}")
        assert ratio <= 1.0
    # without grad mode, or without anything that requires grad, nothing is attached
    v32, f, o32, d32, _ = M.grad_case(F32)
    out = mesh.trace_mesh(mesh.TriangleMesh(v32, f), o32, d32, differentiable=True, reference=True)
    assert not out["t"].requires_grad


# ----------------------------------------------------------------------------- 6. interpolate and mesh_maps
def test_interpolate_and_mesh_maps_shapes_and_misses():
    mesh = _mesh_mod()
    from hfa_gp_amd.cam_utils import ray_grid
    v, f = M.icosphere(2, radius=0.25)                              # (smaller than the image: there is a silhouette)
    m = mesh.TriangleMesh(v, f)
    c = _labels(2)
    res = 16
    o, d = ray_grid(c, res)
    out = mesh.trace_mesh(m, o, d, reference=True)
    hit = out["hit"]
    assert 0 < int(hit.sum()) < hit.numel()
    # the vertex positions as attributes give the hit points; one attribute set for all frames or one per frame
    pos = m.interpolate(v[None], out)
    assert pos.shape == (2, res * res, 3) and bool((pos[~hit] == 0).all())
    assert float((pos - out["point"])[hit].abs().max()) <= 1e-5
    per_frame = m.interpolate(torch.stack((v, 2 * v)), out)
    assert torch.equal(per_frame[0], pos[0]) and torch.equal(per_frame[1], 2 * pos[1])
    labels = torch.arange(v.shape[0], dtype=F32)[:, None].requires_grad_(True)
    val = m.interpolate(labels, out)
    assert val.shape == (2, res * res, 1)
    val.sum().backward()
    assert float(labels.grad.sum()) == pytest.approx(float(hit.sum()), rel=1e-5)                  # the weights of a hit sum to 1
    maps = mesh.mesh_maps(m, c, res, reference=True)
    assert maps["depth"].shape == (2, 1, res, res) and maps["mask"].shape == (2, 1, res, res)
    assert maps["normal"].shape == (2, 3, res, res) and maps["face"].shape == (2, res, res) and maps["face"].dtype == torch.int32
    mask = maps["mask"][:, 0] > 0
    assert torch.equal(mask.reshape(2, -1), hit) and torch.equal(maps["depth"].reshape(2, -1), out["t"])
    assert bool((maps["depth"][:, 0][~mask] == 0).all()) and bool((maps["face"][~mask] == -1).all())
    assert bool((maps["normal"].permute(0, 2, 3, 1)[~mask] == 0).all())
    # flipped towards the camera: n·d < 0 at every hit; unit length; on a sphere about the origin it is ± the face's own normal
    nd = (maps["normal"].permute(0, 2, 3, 1).reshape(2, -1, 3) * d).sum(-1)
    assert bool((nd[hit] < 0).all())
    assert float((maps["normal"].norm(dim=1)[mask] - 1).abs().max()) <= 1e-6
    # a window is a crop at a higher ray density: its centre pixel sees the same face as the full image's centre region
    crop = mesh.mesh_maps(m, c, res, window=(0.25, 0.25, 0.75, 0.75), reference=True)
    assert crop["mask"].mean() > maps["mask"].mean()
    assert isinstance(mesh.TriangleMesh.from_dict({"vertices": v, "faces": f.to(torch.int32)}), mesh.TriangleMesh)


# ----------------------------------------------------------------------------- 7. the C surface
@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_trace_mesh_binding_matches_header(lib):
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} HfagpTraceMeshArgs;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\w+", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in lib.TraceMeshArgs._fields_]
    assert "hfagp_trace_mesh" in lib.SYMBOLS


def test_trace_mesh_argument_validation_returns_codes(lib):
    h = lib.lib()
    assert h.hfagp_trace_mesh(None, None) == -1
    assert b"null pointer" in h.hfagp_last_error()
    a = lib.TraceMeshArgs()
    assert h.hfagp_trace_mesh(C.byref(a), None) == -1 and b"null pointer" in h.hfagp_last_error()
    for f in ("tri", "ray_origins", "ray_directions", "t_near", "t_far"):
        setattr(a, f, 1)                                             # non-null, never dereferenced: everything below is rejected
    a.B, a.R, a.F, a.tri_frames = 1, 5, 3, 1
    assert h.hfagp_trace_mesh(C.byref(a), None) == -1 and b"output" in h.hfagp_last_error()
    a.t = 1
    for field in ("B", "R", "F", "n_pairs"):
        keep = getattr(a, field)
        setattr(a, field, -1)
        assert h.hfagp_trace_mesh(C.byref(a), None) == -1 and b"negative" in h.hfagp_last_error(), field
        setattr(a, field, keep)
    a.tri_frames = 2
    assert h.hfagp_trace_mesh(C.byref(a), None) == -1 and b"tri_frames" in h.hfagp_last_error()
    a.tri_frames, a.cell_start = 1, 1
    assert h.hfagp_trace_mesh(C.byref(a), None) == -1 and b"go together" in h.hfagp_last_error()
    a.cell_faces, a.grid_box, a.G = 1, 1, 0
    assert h.hfagp_trace_mesh(C.byref(a), None) == -1 and b"G = 0" in h.hfagp_last_error()
    a.G = 257
    assert h.hfagp_trace_mesh(C.byref(a), None) == -1 and b"G = 257" in h.hfagp_last_error()
    a.G, a.B, a.tri_frames, a.R = 4, 1 << 12, 1 << 12, 1 << 20
    assert h.hfagp_trace_mesh(C.byref(a), None) == -2 and b"too many rays" in h.hfagp_last_error()
    a.B, a.tri_frames, a.R = 1, 1, 0                                  # no rays: nothing to launch
    assert h.hfagp_trace_mesh(C.byref(a), None) == 0


def test_ops_trace_mesh_refuses_before_any_launch():
    from hfa_gp_amd import ops
    o = torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.trace_mesh(torch.zeros(1, 2, 9), o, o, o[..., 0], o[..., 0])
    with pytest.raises(ValueError, match="want"):
        ops.trace_mesh(torch.zeros(1, 2, 9), o, o, o[..., 0], o[..., 0], want=("depth",))


# ----------------------------------------------------------------------------- 8. the unit's build-time resources
SRC = os.path.join(ROOT, "hfa-gp_amd", "csrc", "mesh_trace.hip")


def _build_flags():
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(mesh_trace\)$", build, re.M), "mesh_trace.hip is not on a units+= line of its own in build.sh"
    return re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_trace_mesh_kernels_have_no_scratch_and_no_spills(tmp_path):
    """Compiled with build.sh's flags: both kernels without scratch and without VGPR or SGPR spills; the brute-force kernel holds
    one tile of kMeshTile 36-byte records in LDS, the grid kernel none."""
    out = subprocess.run([HIPCC, *_build_flags(), "-c", SRC, "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    tile = int(re.search(r"constexpr int kMeshTile = (\d+);", open(SRC).read()).group(1))
    name, seen, lds = None, set(), {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not (name and "trace_mesh_" in name):
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m:
            seen.add(name)
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m:
            lds[name] = int(m.group(1))
    assert len(seen) == 2 and set(lds) == seen, seen
    assert sorted(lds.values()) == [0, tile * 36], lds
    assert [n for n in lds if "brute" in n and lds[n] == tile * 36]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_trace_mesh_unit_has_no_packed_fp32_arithmetic(tmp_path):
    """test_kernel_resources.py's rule for every unit (build.sh's note on packed fp32 ops)."""
    asm = tmp_path / "unit.s"
    out = subprocess.run([HIPCC, *_build_flags(), "-S", "--cuda-device-only", SRC, "-o", str(asm)], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = asm.read_text()
    assert "trace_mesh_brute_kernel" in text and "trace_mesh_grid_kernel" in text
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)
