"""numpy reference of the marching-cubes contract (include/hfagp.h, csrc/marching_cubes.hip) for tests/test_mesh_cpu.py and
tests/test_gpu_mesh.py: the welded vertices in contract order, the faces from the kernel's own case table (read from its
source), and the closed / oriented / edge-manifold check."""
import os
import re

import numpy as np

from tests.util import ROOT

MC_SRC = os.path.join(ROOT, "hfa-gp_amd", "csrc", "marching_cubes.hip")
EDGE_LOW = [0, 1, 2, 3, 0, 1, 4, 5, 0, 2, 4, 6]          # low corner of edge e; axis = e // 4


def mc_table():
    """(counts [256], edges [256][3 * max]) as compiled into marching_cubes.hip"""
    src = open(MC_SRC).read()
    body = re.search(r"kTriCount\[256\] = \{(.*?)\};", src, re.S).group(1)
    counts = np.array([int(x) for x in re.findall(r"\d+", body)], dtype=np.int64)
    body = re.search(r"kTriEdges\[256\]\[\d+\] = \{(.*?)\n\};", src, re.S).group(1)
    rows = [re.sub(r"//.*", "", line) for line in body.splitlines() if "{" in line]
    edges = np.array([[int(x) for x in re.findall(r"\d+", r)] for r in rows], dtype=np.int64)
    assert counts.shape == (256,) and edges.shape[0] == 256
    return counts, edges


def _flags(inside):
    n0, n1, n2 = inside.shape
    f = np.zeros((n0, n1, n2, 3), dtype=bool)
    f[:-1, :, :, 0] = inside[:-1] != inside[1:]
    f[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    f[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    return f


def mc_vertices(vol, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """vertices [V, 3] float64 in the contract order (owning point's linear index, then axis)"""
    vol = np.asarray(vol, dtype=np.float32)
    f = _flags(vol > level).reshape(-1)
    sel = np.nonzero(f)[0]
    point, axis = sel // 3, sel % 3
    n0, n1, n2 = vol.shape
    ijk = np.stack([point // (n1 * n2), (point // n2) % n1, point % n2], 1)
    step = np.eye(3, dtype=np.int64)[axis]
    q = ijk + step
    flat = vol.reshape(-1).astype(np.float64)
    v0 = flat[(ijk[:, 0] * n1 + ijk[:, 1]) * n2 + ijk[:, 2]]
    v1 = flat[(q[:, 0] * n1 + q[:, 1]) * n2 + q[:, 2]]
    t = (np.float64(np.float32(level)) - v0) / (v1 - v0)
    p = ijk.astype(np.float64) + step * t[:, None]
    return np.asarray(origin, np.float64) + np.asarray(spacing, np.float64) * p


def mc_faces(vol, level):
    """faces [F, 3] int64 in the contract order, from the kernel's table"""
    vol = np.asarray(vol, dtype=np.float32)
    inside = vol > level
    n0, n1, n2 = vol.shape
    f = _flags(inside).reshape(-1)
    ids = np.cumsum(f) - 1
    counts, edges = mc_table()
    ci, cj, ck = np.meshgrid(np.arange(n0 - 1), np.arange(n1 - 1), np.arange(n2 - 1), indexing="ij")
    ci, cj, ck = ci.reshape(-1), cj.reshape(-1), ck.reshape(-1)
    case = np.zeros(ci.shape, dtype=np.int64)
    for c in range(8):
        case |= inside[ci + (c >> 2 & 1), cj + (c >> 1 & 1), ck + (c & 1)].astype(np.int64) << c
    nt = counts[case]
    cube = np.repeat(np.arange(case.size), nt)
    slot = np.arange(cube.size) - np.repeat(np.cumsum(nt) - nt, nt)
    out = np.zeros((cube.size, 3), dtype=np.int64)
    for s in range(3):
        e = edges[case[cube], 3 * slot + s]
        low = np.array(EDGE_LOW)[e]
        pi, pj, pk = ci[cube] + (low >> 2 & 1), cj[cube] + (low >> 1 & 1), ck[cube] + (low & 1)
        lin = (pi * n1 + pj) * n2 + pk
        slot_id = lin * 3 + e // 4
        assert f[slot_id].all(), "a face uses an edge that is not crossed"
        out[:, s] = ids[slot_id]
    return out


def closed_manifold(faces, nverts):
    """every undirected edge bounds exactly two faces, once in each direction (closed, oriented, edge-manifold);
    returns the number of undirected edges"""
    faces = np.asarray(faces, dtype=np.int64)
    a = faces.reshape(-1)
    b = faces[:, [1, 2, 0]].reshape(-1)
    directed = a * nverts + b
    u = np.unique(directed)
    assert u.size == directed.size, "a directed edge is used twice (inconsistent orientation or non-manifold)"
    rev = b * nverts + a
    assert np.isin(rev, u).all(), "an edge without its opposite (open surface)"
    return directed.size // 2


def signed_volume_and_area(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    vol = np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0
    area = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1).sum()
    return vol, area
