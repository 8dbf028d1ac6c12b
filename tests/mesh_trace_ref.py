"""Meshes, ray sets and the gradient case shared by the mesh-tracing tests (tests/test_mesh_trace_cpu.py,
tests/test_gpu_mesh_trace.py)."""
import functools
import math

import torch

F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _icosphere64(levels: int):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
             (-t, 0, -1), (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [tuple(x / math.sqrt(1 + t * t) for x in v) for v in verts]
    for _ in range(levels):
        mid = {}

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = [(verts[i][k] + verts[j][k]) / 2 for k in range(3)]
                n = math.sqrt(sum(x * x for x in m))
                verts.append(tuple(x / n for x in m))
                mid[key] = len(verts) - 1
            return mid[key]

        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return torch.tensor(verts, dtype=F64), torch.tensor(faces, dtype=torch.int64)


def icosphere(levels: int, radius: float = 0.5, dtype=torch.float32):
    """(vertices [V, 3], faces [F, 3] int64) of the icosahedron subdivided `levels` times (20·4^levels faces: 20, 80, 320, 1280),
    consistently wound counter-clockwise seen from outside, closed."""
    v, f = _icosphere64(levels)
    return (v * radius).to(dtype), f.clone()


def edges(faces: torch.Tensor) -> torch.Tensor:
    """The unique undirected edges [E, 2] of a face list."""
    e = torch.cat((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]))
    return torch.unique(torch.sort(e, dim=1).values, dim=0)


def sliver_mesh(n: int, seed: int, length: float = 0.4, height: float = 0.04, spread: float = 0.35, dtype=torch.float32):
    """n randomly placed and oriented triangles of base `length` and height `height` (aspect 10 by default), centres within
    `spread` of the origin: overlapping, inconsistently wound, nothing shared — a deliberately bad mesh."""
    g = torch.Generator().manual_seed(seed)
    centre = (torch.rand(n, 3, generator=g, dtype=F64) - 0.5) * 2 * spread
    u = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=F64), dim=-1)
    w = torch.nn.functional.normalize(torch.cross(u, torch.randn(n, 3, generator=g, dtype=F64), dim=-1), dim=-1)
    s = torch.rand(n, 1, generator=g, dtype=F64) - 0.5
    verts = torch.stack((centre - 0.5 * length * u, centre + 0.5 * length * u, centre + s * length * u + height * w), 1).reshape(-1, 3)
    return verts.to(dtype), torch.arange(3 * n).reshape(n, 3)


def second_frame(vertices: torch.Tensor) -> torch.Tensor:
    """[2, V, 3]: the vertices, and the same rotated, scaled and moved (a second frame of a sequence)."""
    c, s = math.cos(0.7), math.sin(0.7)
    rot = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=vertices.dtype)
    return torch.stack((vertices, (vertices @ rot.T) * 1.3 + torch.tensor([0.11, -0.07, 0.05], dtype=vertices.dtype)))


def adversarial_rays(vertices: torch.Tensor, faces: torch.Tensor, box, g: int, seed: int):
    """Rays [n, 3] x 2 and limits [n] x 2 (float32) against one frame of a mesh with the grid box (lo [3], cell [3]) at G = g: the
    special rays first, then rays aimed at vertices, edge midpoints and grid lattice points from inside and outside, axis-parallel
    rays (some lying exactly in a cell-boundary plane), origins inside the mesh and inside the box, and random ones."""
    gen = torch.Generator().manual_seed(seed)
    f32 = torch.float32
    lo, cell = box
    hi = lo + g * cell
    centre = vertices.mean(0)
    size = float((vertices - centre).norm(dim=-1).max())
    o_list, d_list, tn_list, tf_list = [], [], [], []

    def add(o, d, tn=0.0, tf=float("inf")):
        o, d = o.to(f32).reshape(-1, 3), d.to(f32).reshape(-1, 3)
        n = max(o.shape[0], d.shape[0])
        o_list.append(o.expand(n, 3))
        d_list.append(d.expand(n, 3))
        tn_list.append(torch.full((n,), tn, dtype=f32))
        tf_list.append(torch.full((n,), tf, dtype=f32))

    outside = centre + torch.tensor([0.3, -0.4, 2.7], dtype=f32) * max(size, 1e-3) / 0.5
    inside = centre + torch.tensor([0.013, -0.021, 0.017], dtype=f32) * size
    nan = float("nan")
    # ---- the specials
    add(outside, torch.zeros(3))                                                    # zero direction
    add(outside, torch.tensor([nan, 0.0, -1.0]))                                    # NaN direction
    add(outside, centre - outside, tn=5.0, tf=1.0)                                  # t_far < t_near
    add(outside, centre - outside, tn=nan)                                          # NaN limit
    add(outside, outside - centre)                                                  # points away: misses the box
    add(hi + (hi - lo), torch.tensor([1.0, 0.0, 0.0]))                              # axis-parallel and beside the box
    add(outside, centre - outside, tn=0.0, tf=1e-3)                                 # stops before the mesh
    add(torch.tensor([nan, 0.0, 0.0]), torch.tensor([0.0, 0.0, 1.0]))               # NaN origin
    # ---- aimed at vertices and edge midpoints, from inside and outside
    e = edges(faces)
    mids = 0.5 * (vertices[e[:, 0]] + vertices[e[:, 1]])
    pick_v = torch.randperm(vertices.shape[0], generator=gen)[:48]
    pick_e = torch.randperm(mids.shape[0], generator=gen)[:64]
    for origin in (inside, outside):
        add(origin, vertices[pick_v] - origin)
        add(origin, mids[pick_e] - origin)
    # ---- aimed at grid lattice points
    idx = torch.randint(0, g + 1, (48, 3), generator=gen)
    lattice = lo + idx.to(f32) * cell
    add(outside, lattice - outside)
    add(inside, lattice - inside)
    # ---- axis-parallel rays from outside the box; half of them start exactly on cell-boundary planes of the other two axes
    for axis in range(3):
        for sign in (1.0, -1.0):
            u = torch.rand(16, 3, generator=gen)
            p = lo + u * (hi - lo)
            snap = lo + torch.randint(0, g + 1, (16, 3), generator=gen).to(f32) * cell
            p[8:] = snap[8:]
            p[:, axis] = float(lo[axis] - (hi - lo)[axis]) if sign > 0 else float(hi[axis] + (hi - lo)[axis])
            d = torch.zeros(3)
            d[axis] = sign
            add(p, d)
            add(p[:4], d * 0.37, tn=-1.0)                                           # not unit, a negative t_near
    # ---- origins inside the box (some inside the mesh), random directions, finite limits on some
    p = lo + torch.rand(48, 3, generator=gen) * (hi - lo)
    add(p, torch.randn(48, 3, generator=gen))
    add(p[:16], torch.randn(16, 3, generator=gen), tn=0.05 * size, tf=0.8 * size)
    add(inside, torch.randn(32, 3, generator=gen))
    # ---- random rays from outside towards the mesh
    aim = centre + (torch.rand(96, 3, generator=gen) - 0.5) * 2.2 * size
    add(outside, aim - outside)
    return torch.cat(o_list).contiguous(), torch.cat(d_list).contiguous(), torch.cat(tn_list), torch.cat(tf_list)


def grad_case(dtype):
    """The case of the gradient tests: an 80-face sphere in two frames, 2 x 32 rays (30 aimed well inside faces, from outside and
    from inside; two misses per frame) and the coefficients of L = Σ c·(t, bary, point)."""
    v, f = icosphere(1, dtype=F64)
    g = torch.Generator().manual_seed(21)
    pick = torch.randperm(f.shape[0], generator=g)[:30]
    w = torch.rand(30, 3, generator=g, dtype=F64) + 0.15
    w = w / w.sum(-1, keepdim=True)
    target = (v[f[pick]] * w[..., None]).sum(1)                                                 # well inside 30 faces
    o = torch.tensor([[0.3, -0.4, 2.2], [0.02, 0.03, -0.05]], dtype=F64)[:, None].expand(2, 30, 3).contiguous()
    d = (target[None] - o) * (0.5 + torch.rand(2, 30, 1, generator=g, dtype=F64))
    o = torch.cat((o, torch.tensor([0.0, 0.0, 3.0], dtype=F64).expand(2, 2, 3)), 1)               # two misses per frame
    d = torch.cat((d, torch.tensor([0.0, 1.0, 0.0], dtype=F64).expand(2, 2, 3)), 1)
    coef = {k: torch.randn(2, 32, n, generator=g, dtype=F64) for k, n in (("t", 1), ("bary", 3), ("point", 3))}
    return second_frame(v).to(dtype), f, o.to(dtype).contiguous(), d.to(dtype).contiguous(), coef


def grad_loss(out, coef):
    return sum((out[k].reshape(2, 32, -1).double() * coef[k]).sum() for k in coef)
