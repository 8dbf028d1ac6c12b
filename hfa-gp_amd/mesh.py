"""Ray lists against triangle meshes: which face a ray sees first, where, and with which barycentric weights — the depth, normal,
silhouette and face-index maps of a 3DMM mesh or a scan from any camera, on the device and pixel-aligned with the renderer's own
`image_depth`, `image_mask` and `image_normal`.

  * `trace_mesh_reference` — the definition, brute force in plain torch, in the dtype of its inputs, usable on the CPU;
  * `TriangleMesh` — one topology, per-frame vertices, checked once on the host; `build_grid` adds a uniform grid of face lists;
  * `trace_mesh` — hfagp_trace_mesh (csrc/mesh_trace.hip) on a `TriangleMesh`: the reference's float32 bits, brute force or through
    the grid; ``differentiable=True`` attaches the gradient of t, bary and point w.r.t. the vertices and the rays (face held fixed);
  * `TriangleMesh.interpolate` — vertex attributes at the hits; `mesh_maps` — the maps of a camera label.

The definition.  Per ray o, d with limits tn, tf and per face with vertices a, b, c, every operation rounded once:

    A = a−o, B = b−o, C = c−o
    cross(x,y) = (x1*y2 − x2*y1,  x2*y0 − x0*y2,  x0*y1 − x1*y0);   dot(x,y) = (x0*y0 + x1*y1) + x2*y2
    U = dot(d, cross(B,C));  V = dot(d, cross(C,A));  W = dot(d, cross(A,B));  det = (U + V) + W
    N = cross(b−a, c−a);  dn = dot(d, N);  t = dot(A, N) / dn
    candidate  iff  ((U≥0 & V≥0 & W≥0) | (U≤0 & V≤0 & W≤0)) & det≠0 & dn≠0 & tn ≤ t & t ≤ tf     (a NaN fails every comparison)
    winner     = the candidate of smallest t; equal t: the smallest face index

The edge functions U, V, W are exactly antisymmetric: the face across an edge forms the same products in the other order and gets
the negated bits, so a ray through a shared edge is accepted by one of the two faces — a consistently wound closed mesh has no
cracks along its edges.  The one known leak: a ray aimed exactly at a VERTEX can miss, when rounding gives every edge of the fan
around it the same sign (0, 6 and 11 of the 642 such rays on a 1280-face icosphere, from three interior origins).  Hits are two-sided."""
from __future__ import annotations

import math
from typing import Optional

import torch

INF = float("inf")
# The padding of a face's box when it is sorted into the grid, as a fraction of a cell, and the margin of the grid's box around
# the mesh, as a fraction of its largest extent ("Mesh tracing", has the reasons and the sizes).
GRID_PAD = 0.125
GRID_MARGIN = 1.0 / 64


def _cross(x, y):
    x0, x1, x2 = x.unbind(-1)
    y0, y1, y2 = y.unbind(-1)
    return torch.stack((x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0), -1)


def _dot(x, y):
    x0, x1, x2 = x.unbind(-1)
    y0, y1, y2 = y.unbind(-1)
    return (x0 * y0 + x1 * y1) + x2 * y2


def _face_terms(o, d, a, b, c):
    """(U, V, W, det, N, dn, t) of rays against faces, broadcast over the leading dimensions: the definition, one rounding each."""
    A, B, C = a - o, b - o, c - o
    U, V, W = _dot(d, _cross(B, C)), _dot(d, _cross(C, A)), _dot(d, _cross(A, B))
    det = (U + V) + W
    N = _cross(b - a, c - a)
    dn = _dot(d, N)
    t = _dot(A, N) / dn
    return U, V, W, det, N, dn, t


def _sqrt_rn(x):
    """The correctly rounded square root, whatever `torch.sqrt` does in float32 on the device at hand: float32 goes through
    float64 — the exactly converted operand's root, rounded to 53 bits and then to 24, is the correctly rounded float32 root
    (53 >= 2·24 + 2: double rounding is exact for the square root) —, as the kernel's root is the correctly rounded one."""
    return torch.sqrt(x.double()).to(x.dtype) if x.dtype == torch.float32 else torch.sqrt(x)


def _candidate(U, V, W, det, dn, t, tn, tf):
    same = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
    return same & (det != 0) & (dn != 0) & (tn <= t) & (t <= tf)


def _limits(x, like: torch.Tensor, name: str) -> torch.Tensor:
    b, r = like.shape[:2]
    if not torch.is_tensor(x):
        return torch.full((b, r), float(x), dtype=like.dtype, device=like.device)
    if tuple(x.shape) != (b, r):
        raise ValueError(f"trace_mesh: {name} must be a float or [B, R] = [{b}, {r}], got {tuple(x.shape)}")
    return x.detach().to(like.dtype).contiguous()


def _check_rays(who: str, origins: torch.Tensor, directions: torch.Tensor) -> None:
    if origins.dim() != 3 or origins.shape[-1] != 3 or origins.shape != directions.shape:
        raise ValueError(f"{who}: origins / directions must be [B, R, 3], got {tuple(origins.shape)}, {tuple(directions.shape)}")


def trace_mesh_reference(vertices: torch.Tensor, faces: torch.Tensor, origins: torch.Tensor, directions: torch.Tensor,
                         t_near=0.0, t_far=INF, max_pairs: int = 1 << 22) -> dict:
    """The definition of `trace_mesh` (the module's docstring) by brute force over rays × faces in plain torch, in the dtype of
    the rays — float32 as the kernel computes, float64 as the yardstick —, usable on the CPU.  Only elementwise * + − /,
    comparisons, `where` and `min`, so every operation is rounded once.  Chunked so that rays × faces stays below ``max_pairs``.
    vertices [B or 1, V, 3] (or [V, 3]), faces [F, 3] integer, rays [B, R, 3], limits floats or [B, R] →
    {'hit' [B,R] bool, 'face' [B,R] int32 (−1: miss), 't' [B,R], 'bary' [B,R,3] = (U, V, W)/det, 'point' [B,R,3] = o + t·d,
    'normal' [B,R,3] = N / sqrt(dot(N,N)) (the winding's, not flipped), 'front' [B,R] bool = dn < 0}.  A miss has exact zeros in every
    float entry and front = False.  Not differentiable (computed under no_grad)."""
    who = "trace_mesh_reference"
    _check_rays(who, origins, directions)
    if vertices.dim() == 2:
        vertices = vertices[None]
    b, r = origins.shape[:2]
    if vertices.dim() != 3 or vertices.shape[-1] != 3 or vertices.shape[0] not in (1, b):
        raise ValueError(f"{who}: vertices must be [B or 1, V, 3] for {b} frames, got {tuple(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[-1] != 3:
        raise ValueError(f"{who}: faces must be [F, 3], got {tuple(faces.shape)}")
    dt, dev = origins.dtype, origins.device
    if vertices.dtype != dt or directions.dtype != dt:
        raise ValueError(f"{who}: vertices, origins and directions must share a dtype, got {vertices.dtype}, {dt}, {directions.dtype}")
    with torch.no_grad():
        vertices, origins, directions = vertices.detach(), origins.detach(), directions.detach()
        tn_all, tf_all = _limits(t_near, origins, "t_near"), _limits(t_far, origins, "t_far")
        nf = faces.shape[0]
        big = torch.iinfo(torch.int64).max
        best_t = torch.full((b, r), INF, dtype=dt, device=dev)
        best_f = torch.full((b, r), big, dtype=torch.int64, device=dev)
        f_chunk = max(1, min(nf, int(max_pairs)))
        r_chunk = max(1, int(max_pairs) // f_chunk)
        fl = faces.long()
        for f in range(b):
            vf = vertices[f if vertices.shape[0] > 1 else 0]
            for f0 in range(0, nf, f_chunk):
                ids = fl[f0:f0 + f_chunk]
                a, bb, c = vf[ids[:, 0]][None], vf[ids[:, 1]][None], vf[ids[:, 2]][None]             # [1, n_f, 3]
                index = torch.arange(f0, f0 + ids.shape[0], device=dev)[None]
                for r0 in range(0, r, r_chunk):
                    sl = slice(r0, r0 + r_chunk)
                    o, d = origins[f, sl, None, :], directions[f, sl, None, :]                           # [n_r, 1, 3]
                    U, V, W, det, _, dn, t = _face_terms(o, d, a, bb, c)
                    cand = _candidate(U, V, W, det, dn, t, tn_all[f, sl, None], tf_all[f, sl, None])
                    t_c = torch.where(cand, t, torch.full_like(t, INF)).min(1).values
                    first = cand & (t == t_c[:, None])
                    f_c = torch.where(first, index, torch.full_like(index, big)).min(1).values
                    better = (f_c != big) & ((t_c < best_t[f, sl]) | ((t_c == best_t[f, sl]) & (f_c < best_f[f, sl])))
                    best_t[f, sl] = torch.where(better, t_c, best_t[f, sl])
                    best_f[f, sl] = torch.where(better, f_c, best_f[f, sl])
        hit = best_f != big
        face = torch.where(hit, best_f, torch.zeros_like(best_f))
        zero = torch.zeros((), dtype=dt, device=dev)
        if nf == 0:
            z3 = torch.zeros(b, r, 3, dtype=dt, device=dev)
            return {"hit": hit, "face": torch.full((b, r), -1, dtype=torch.int32, device=dev), "t": z3[..., 0].clone(), "bary": z3,
                    "point": z3.clone(), "normal": z3.clone(), "front": hit.clone()}
        # the winner's own evaluation: the same expressions on [B, R, 3]
        vb = vertices.expand(b, -1, -1)
        ids = fl[face]                                                                                # [B, R, 3]
        a, bb, c = (torch.gather(vb, 1, ids[..., k:k + 1].expand(-1, -1, 3)) for k in range(3))
        U, V, W, det, N, dn, t = _face_terms(origins, directions, a, bb, c)
        h3 = hit[..., None]
        return {"hit": hit,
                "face": torch.where(hit, best_f, torch.full_like(best_f, -1)).to(torch.int32),
                "t": torch.where(hit, t, zero),
                "bary": torch.where(h3, torch.stack((U, V, W), -1) / det[..., None], zero),
                "point": torch.where(h3, origins + t[..., None] * directions, zero),
                "normal": torch.where(h3, N / _sqrt_rn(_dot(N, N))[..., None], zero),
                "front": hit & (dn < 0)}


def _default_resolution(n_faces: int) -> int:
    """Cells per axis when `build_grid` is not told: (8 F)^(1/3), at most 128.  From the runs in profiles/mesh_trace/README.md:
    on marching-cubes heads of 67 k and 271 k faces (G = 82 and 128 by this rule, both measured) the trace got faster with
    every step from G = 32 to G = 128 while the build time did not move and the pairs per face stayed below 11; G above 128 was
    not measured, hence the cap."""
    return max(1, min(128, int(math.ceil((8.0 * max(n_faces, 1)) ** (1.0 / 3.0)))))


class TriangleMesh:
    """One topology with per-frame vertex positions: ``vertices`` [B or 1, V, 3] (or [V, 3]) float32, ``faces`` [F, 3] int32 or
    int64 — a 3DMM sequence, or one static scan for all frames.  Construction checks on the host, with one synchronisation, that
    0 ≤ faces < V, that the vertices are finite and that F and V fit in int32, and gathers the per-face vertex records ``tri``
    [B or 1, F, 9] the kernels read: they never index with unchecked data.  ``vertices`` is kept as given (it may require grad: see
    `trace_mesh(differentiable=True)`); the records are a snapshot — after changing the vertices make a new mesh.  float64 vertices
    are accepted for `trace_mesh(reference=True)` only."""

    def __init__(self, vertices: torch.Tensor, faces: torch.Tensor):
        if vertices.dim() == 2:
            vertices = vertices[None]
        if vertices.dim() != 3 or vertices.shape[-1] != 3 or vertices.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"TriangleMesh: vertices must be float32 (float64 for reference=True) [B or 1, V, 3], got {vertices.dtype} "
                             f"{tuple(vertices.shape)}")
        if faces.dim() != 2 or faces.shape[-1] != 3 or faces.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"TriangleMesh: faces must be int32 / int64 [F, 3], got {faces.dtype} {tuple(faces.shape)}")
        if faces.device != vertices.device:
            raise ValueError(f"TriangleMesh: vertices on {vertices.device}, faces on {faces.device}")
        nv, nf = vertices.shape[1], faces.shape[0]
        if nv >= 2 ** 31 or nf >= 2 ** 31:
            raise ValueError(f"TriangleMesh: V = {nv} and F = {nf} must fit in int32")
        with torch.no_grad():
            flags = [torch.isfinite(vertices).all()]
            if nf:
                flags += [faces.min() >= 0, faces.max() < nv]
            flags = torch.stack(flags).tolist()                       # the one synchronisation
            if not flags[0]:
                raise ValueError("TriangleMesh: vertices must be finite")
            if not all(flags[1:]):
                raise ValueError(f"TriangleMesh: faces must index the {nv} vertices (0 <= faces < V)")
            self.vertices = vertices
            self.faces = faces.to(torch.int32).contiguous()
            self.tri = vertices.detach()[:, self.faces.long().reshape(-1)].reshape(vertices.shape[0], nf, 9).contiguous()
        self.grid = None

    @classmethod
    def from_dict(cls, m: dict) -> "TriangleMesh":
        """A mesh dict of `TriPlaneGenerator.extract_mesh` ({'vertices' [V, 3], 'faces' [F, 3], ...})."""
        return cls(m["vertices"], m["faces"])

    @property
    def frames(self) -> int:
        return self.vertices.shape[0]

    @property
    def num_faces(self) -> int:
        return self.faces.shape[0]

    def build_grid(self, resolution: Optional[int] = None, max_pairs: int = 1 << 26):
        """A uniform grid of G³ cells over each frame's bounding box with, per cell, the list of the faces whose padded box touches
        it; `trace_mesh` then walks the cells instead of testing every face.  Entirely in torch, without atomics: building twice
        gives the same tensors.  Per frame: the box is the vertices' bounding box grown by GRID_MARGIN of its largest extent; each
        face's box, grown by GRID_PAD of a cell, becomes integer cell ranges; the (cell, face) pairs are formed by
        `repeat_interleave` arithmetic, sorted stably by cell (so every list is ascending in the face index), and `cell_start`
        [G³+1] is a bincount's cumsum.  More than ``max_pairs`` pairs raises before any of them is allocated.  ``resolution`` = G
        in [1, 256]; None: `_default_resolution`.  Two synchronisations (the pair count; the final check of the lists).
        Sets and returns ``self.grid`` = (cell_start [frames, G³+1] int32, cell_faces [P] int32, box [frames, 6] float32, G):
        offsets of all frames into one list; box = the lower corner and the cell size per axis."""
        nf, frames, dev = self.num_faces, self.frames, self.tri.device
        g = _default_resolution(nf) if resolution is None else int(resolution)
        if not 1 <= g <= 256:
            raise ValueError(f"build_grid: resolution must be in [1, 256], got {resolution}")
        if self.tri.dtype != torch.float32:
            raise ValueError("build_grid: float32 vertices only")
        if nf == 0:
            raise ValueError("build_grid: the mesh has no faces")
        with torch.no_grad():
            tri = self.tri.reshape(frames, nf, 3, 3)
            vmin, vmax = tri.amin((1, 2)), tri.amax((1, 2))                                         # [frames, 3]
            extent = (vmax - vmin).amax(-1, keepdim=True)
            margin = torch.where(extent > 0, extent * GRID_MARGIN, torch.ones_like(extent))
            lo = vmin - margin
            cell = ((vmax + margin) - lo) / g
            pad = cell * GRID_PAD
            fmin, fmax = tri.amin(2), tri.amax(2)                                                   # [frames, F, 3]
            i0 = torch.floor((fmin - pad[:, None] - lo[:, None]) / cell[:, None]).clamp(0, g - 1).long()
            i1 = torch.floor((fmax + pad[:, None] - lo[:, None]) / cell[:, None]).clamp(0, g - 1).long()
            ext = i1 - i0 + 1                                                                       # [frames, F, 3], >= 1
            count = ext.prod(-1)                                                                    # [frames, F]
            totals = count.sum(1).tolist()                                                          # synchronisation 1
            if sum(totals) > int(max_pairs):
                raise ValueError(f"build_grid: {sum(totals)} (cell, face) pairs at resolution {g} exceed max_pairs = {max_pairs}")
            starts, lists = [], []
            offset = 0
            for f in range(frames):
                n = count[f]
                face = torch.repeat_interleave(torch.arange(nf, device=dev), n, output_size=totals[f])
                local = torch.arange(totals[f], device=dev) - torch.repeat_interleave(torch.cumsum(n, 0) - n, n, output_size=totals[f])
                ey, ez = ext[f, face, 1], ext[f, face, 2]
                dx, rem = local // (ey * ez), local % (ey * ez)
                dy, dz = rem // ez, rem % ez
                key = ((i0[f, face, 0] + dx) * g + (i0[f, face, 1] + dy)) * g + (i0[f, face, 2] + dz)
                key, order = torch.sort(key, stable=True)
                lists.append(face[order])
                filled = torch.bincount(key, minlength=g ** 3)
                start = torch.zeros(g ** 3 + 1, dtype=torch.int64, device=dev)
                start[1:] = torch.cumsum(filled, 0)
                starts.append(start + offset)
                offset += totals[f]
            cell_start = torch.stack(starts).to(torch.int32).contiguous()
            cell_faces = torch.cat(lists).to(torch.int32).contiguous()
            box = torch.cat((lo, cell), -1).contiguous()
            flat = cell_start.reshape(-1)
            ok = (flat[1:] >= flat[:-1]).all() & (flat[0] == 0) & (flat[-1] == cell_faces.shape[0]) & \
                (cell_faces >= 0).all() & (cell_faces < nf).all() & torch.isfinite(box).all() & (cell > 0).all()
            if not bool(ok):                                                                        # synchronisation 2
                raise RuntimeError("build_grid: inconsistent cell lists (this is a bug)")
        self.grid = (cell_start, cell_faces, box, g)
        return self.grid

    def interpolate(self, attributes: torch.Tensor, out: dict) -> torch.Tensor:
        """Vertex attributes [B or 1, V, C] at the hits of ``out`` (a result of `trace_mesh` on this mesh) → [B, R, C] =
        Σ bary·attribute over the hit face's vertices, in plain torch: vertex normals, colours, UVs, 3DMM semantic labels.
        Differentiable w.r.t. the attributes and, through out['bary'] of a ``differentiable=True`` trace, the vertices.  Misses
        give zeros."""
        if attributes.dim() == 2:
            attributes = attributes[None]
        b, r = out["face"].shape
        if attributes.dim() != 3 or attributes.shape[1] != self.vertices.shape[1] or attributes.shape[0] not in (1, b):
            raise ValueError(f"interpolate: attributes must be [B or 1, V = {self.vertices.shape[1]}, C] for B = {b}, got "
                             f"{tuple(attributes.shape)}")
        ch = attributes.shape[-1]
        hit = out["hit"].bool()
        if self.num_faces == 0:
            return torch.zeros(b, r, ch, dtype=attributes.dtype, device=attributes.device)
        ids = self.faces.long()[out["face"].clamp(min=0).long()]                                    # [B, R, 3]
        ab = attributes.expand(b, -1, -1)
        corner = [torch.gather(ab, 1, ids[..., k:k + 1].expand(-1, -1, ch)) for k in range(3)]
        bary = out["bary"].to(attributes.dtype)
        val = (bary[..., 0:1] * corner[0] + bary[..., 1:2] * corner[1]) + bary[..., 2:3] * corner[2]
        return torch.where(hit[..., None], val, torch.zeros_like(val))


# a well-conditioned triangle and ray, in place of a miss's operands when the closed form is re-evaluated for its gradient
_SAFE = {"a": (0.0, 0.0, 1.0), "b": (1.0, 0.0, 1.0), "c": (0.0, 1.0, 1.0), "o": (0.25, 0.25, 0.0), "d": (0.0, 0.0, 1.0)}


def trace_mesh(mesh: TriangleMesh, origins: torch.Tensor, directions: torch.Tensor, t_near=0.0, t_far=INF,
               differentiable: bool = False, reference: bool = False) -> dict:
    """The first hit of every ray [B, R, 3] (directions not normalised) with the mesh, limits floats or [B, R] → the dict of
    `trace_mesh_reference`: 'hit', 'face', 't', 'bary', 'point', 'normal', 'front'.  One launch of hfagp_trace_mesh; through the grid
    if `mesh.build_grid` was called, brute force otherwise.  Brute force gives the float32 bits of the reference on every ray; the
    grid gives the same bits wherever every float32 candidate's computed point lies within 1/8 cell of its face — not for the
    phantom candidates that near-degenerate faces (edges below ~1e-5 of the scene) or grazing faces produce in float32, which
    the grid usually does not report (profiles/mesh_trace/README.md has the counts on marching-cubes meshes).
    ``reference=True`` evaluates `trace_mesh_reference` instead (any device, float32 or float64): the kernel is never replaced
    silently — CPU tensors without it raise.
    ``differentiable=True`` (under grad): 't', 'bary' and 'point' carry gradients w.r.t. ``mesh.vertices`` and the rays with the
    hit face held fixed: the winning face's vertices are gathered, the closed form is re-evaluated for that one face per ray in
    torch, and the result is kernel_value + (recomputed − recomputed.detach()).  A miss gets exactly zero gradient; 'normal' is
    not differentiable."""
    who = "trace_mesh"
    _check_rays(who, origins, directions)
    b, r = origins.shape[:2]
    if mesh.frames not in (1, b):
        raise ValueError(f"{who}: the mesh has {mesh.frames} frames of vertices, the rays {b}")
    tn, tf = _limits(t_near, origins, "t_near"), _limits(t_far, origins, "t_far")
    o, d = origins.detach().contiguous(), directions.detach().contiguous()
    if reference:
        out = trace_mesh_reference(mesh.vertices.detach(), mesh.faces, o, d, tn, tf)
    else:
        from . import ops
        out = ops.trace_mesh(mesh.tri, o, d, tn, tf, grid=mesh.grid)
        out["hit"], out["front"] = out["hit"].bool(), out["front"].bool()
    grad = differentiable and torch.is_grad_enabled() and \
        (mesh.vertices.requires_grad or origins.requires_grad or directions.requires_grad)
    if not grad or mesh.num_faces == 0:
        return out
    hit = out["hit"]
    h3 = hit[..., None]
    ids = mesh.faces.long()[out["face"].clamp(min=0).long()]                                         # [B, R, 3]
    vb = mesh.vertices.expand(b, -1, -1)
    safe = {k: torch.tensor(v, dtype=origins.dtype, device=origins.device) for k, v in _SAFE.items()}
    a, bb, c = (torch.where(h3, torch.gather(vb, 1, ids[..., k:k + 1].expand(-1, -1, 3)), safe[n]) for k, n in enumerate("abc"))
    og, dg = torch.where(h3, origins, safe["o"]), torch.where(h3, directions, safe["d"])
    U, V, W, det, _, _, t = _face_terms(og, dg, a, bb, c)
    rec = {"t": t, "bary": torch.stack((U, V, W), -1) / det[..., None], "point": og + t[..., None] * dg}
    out = dict(out)
    for k, v in rec.items():
        out[k] = out[k] + (v - v.detach())
    return out


def mesh_maps(mesh: TriangleMesh, c: torch.Tensor, res: int, window=None, t_near=0.0, t_far=INF, reference: bool = False) -> dict:
    """The geometry maps of a mesh from the camera labels c [B, 25], on `cam_utils.ray_grid`'s rays (unit directions, pixel centres
    in row order; ``window`` as there) — pixel-aligned with `image_depth`, `image_mask` and `image_normal` of `synthesis` at that
    label and rendering resolution, the targets of ``geometry=True`` and ``normal_grad=True`` fitting steps:
    {'depth' [B,1,res,res] (t along the unit ray, 0 at a miss), 'mask' [B,1,res,res] (1 at a hit), 'normal' [B,3,res,res] (world
    space, the face's geometric normal flipped towards the camera, 0 at a miss), 'face' [B,res,res] int32 (−1 at a miss)}."""
    from .cam_utils import ray_grid
    with torch.no_grad():
        o, d = ray_grid(c, int(res), window)
        out = trace_mesh(mesh, o.contiguous(), d, t_near, t_far, reference=reference)
        b = c.shape[0]
        n = torch.where(out["front"][..., None], out["normal"], -out["normal"])
        n = torch.where(out["hit"][..., None], n, torch.zeros_like(n))                               # (no −0 at a miss)
        return {"depth": out["t"].reshape(b, 1, res, res),
                "mask": out["hit"].to(out["t"].dtype).reshape(b, 1, res, res),
                "normal": n.reshape(b, res, res, 3).permute(0, 3, 1, 2).contiguous(),
                "face": out["face"].reshape(b, res, res)}
