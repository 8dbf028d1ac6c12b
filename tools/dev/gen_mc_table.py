#!/usr/bin/env python
"""Generate the marching-cubes triangle table of csrc/marching_cubes.hip (the block between the `mc-table` markers).

    python tools/dev/gen_mc_table.py            # print the C block
    python tools/dev/gen_mc_table.py --write    # rewrite it in place

Built from one rule per cube face, so that two cubes sharing a face always cut it the same way:
  * corner c of a cube sits at offset (c >> 2 & 1, c >> 1 & 1, c & 1) along (axis 0, 1, 2); the case is sum(inside(c) << c);
  * edge e = 4 * axis + r joins corner LOW[e] to LOW[e] + (1 << (2 - axis)), r enumerating the corners whose bit of that
    axis is 0 (EDGES below); an edge is crossed iff exactly one end is inside;
  * on a face, each crossed edge is joined to the next crossed edge round the face; where a face has 4 crossed edges (two
    diagonal inside corners) each inside corner is cut off on its own (inside corners never connect across a face diagonal),
  * each such segment d is directed so that n x d (n the face's outward normal) points away from the inside: the segments
    of a cube then chain into closed loops, and a segment on a face shared by two cubes is traversed once in each direction;
  * each loop is cut into triangles in loop order (normal toward decreasing values), never by a diagonal whose two
    vertices lie on one cube face (a shared face therefore carries only its segments, so every edge of the mesh of a
    volume with an outside boundary layer bounds exactly two triangles).
The table lists, per case, the triangles as edge triples; the kernel maps edges to welded vertex indices.
"""
from __future__ import annotations

import itertools
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TARGET = os.path.join(HERE, "..", "..", "hfa-gp_amd", "csrc", "marching_cubes.hip")


def corner_pos(c):
    return np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1], dtype=float)


EDGES = []          # (low corner, axis), index 4 * axis + r
for axis in range(3):
    bit = 1 << (2 - axis)
    EDGES += [(c, axis) for c in range(8) if not c & bit]


def edge_ends(e):
    c, axis = EDGES[e]
    return c, c | (1 << (2 - axis))


def edge_mid(e):
    a, b = edge_ends(e)
    return (corner_pos(a) + corner_pos(b)) / 2


def edge_faces(e):
    """the two cube faces (axis, side) that hold edge e"""
    c, axis = EDGES[e]
    return {(a, int(corner_pos(c)[a])) for a in range(3) if a != axis}


def face_cycle(axis, side):
    """corners of face (axis, side) in cyclic order, and the outward normal"""
    b, c = [a for a in range(3) if a != axis]
    out = []
    for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
        pos = [0, 0, 0]
        pos[axis], pos[b], pos[c] = side, u, v
        out.append((pos[0] << 2) | (pos[1] << 1) | pos[2])
    n = np.zeros(3)
    n[axis] = 1.0 if side else -1.0
    return out, n


def edge_of(c0, c1):
    lo, hi = min(c0, c1), max(c0, c1)
    for e in range(12):
        if edge_ends(e) == (lo, hi):
            return e
    raise AssertionError((c0, c1))


def segments(case):
    inside = [(case >> c) & 1 for c in range(8)]
    segs = []
    for axis, side in itertools.product(range(3), range(2)):
        cyc, n = face_cycle(axis, side)
        ring = [(edge_of(cyc[i], cyc[(i + 1) % 4]), cyc[i], cyc[(i + 1) % 4]) for i in range(4)]
        crossed = [i for i in range(4) if inside[cyc[i]] != inside[cyc[(i + 1) % 4]]]
        pairs = []
        if len(crossed) == 2:
            ref = next(c for c in cyc if inside[c])
            pairs.append((ring[crossed[0]][0], ring[crossed[1]][0], ref))
        elif len(crossed) == 4:
            for i in range(4):
                if inside[cyc[i]]:                       # cut this inside corner off: its two ring edges
                    pairs.append((ring[(i - 1) % 4][0], ring[i][0], cyc[i]))
        for e1, e2, ref in pairs:
            p1, p2 = edge_mid(e1), edge_mid(e2)
            d = p2 - p1
            if np.dot(np.cross(n, d), corner_pos(ref) - (p1 + p2) / 2) > 0:
                e1, e2 = e2, e1
            segs.append((e1, e2))
    return segs


def loops(case):
    succ = {}
    for e1, e2 in segments(case):
        assert e1 not in succ, (case, e1)
        succ[e1] = e2
    assert sorted(succ) == sorted(succ.values()), case
    out, seen = [], set()
    for start in sorted(succ):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = succ[e]
        assert e == start
        out.append(loop)
    return out


def share_face(e1, e2):
    return bool(edge_faces(e1) & edge_faces(e2))


def triangulate(poly):
    """triangles of polygon `poly` (loop order kept), no diagonal between two edges of one face; None if impossible"""
    if len(poly) == 3:
        return [tuple(poly)]
    a, b = poly[0], poly[1]
    for m in range(2, len(poly)):
        apex = poly[m]
        if m != 2 and share_face(b, apex):
            continue
        if m != len(poly) - 1 and share_face(apex, a):
            continue
        left = triangulate(poly[1:m + 1]) if m != 2 else []
        right = triangulate(poly[m:] + [a]) if m != len(poly) - 1 else []
        if left is None or right is None:
            continue
        return [(a, b, apex)] + left + right
    return None


def table():
    tris = []
    for case in range(256):
        t = []
        for loop in loops(case):
            got = triangulate(loop)
            assert got is not None, (case, loop)
            t += got
        tris.append(t)
    return tris


def c_block():
    tris = table()
    width = max(len(t) for t in tris)
    lines = ["// mc-table begin (generated by tools/dev/gen_mc_table.py; do not edit by hand)",
             "__constant__ unsigned char kTriCount[256] = {"]
    counts = [str(len(t)) for t in tris]
    for i in range(0, 256, 32):
        lines.append("    " + ", ".join(counts[i:i + 32]) + ",")
    lines.append("};")
    lines.append(f"__constant__ unsigned char kTriEdges[256][{3 * width}] = {{")
    for case, t in enumerate(tris):
        flat = [e for tri in t for e in tri] + [0] * (3 * (width - len(t)))
        lines.append("    {" + ", ".join(str(e) for e in flat) + f"}},  // {case}")
    lines.append("};")
    lines.append("// mc-table end")
    return "\n".join(lines) + "\n"


def main(argv):
    block = c_block()
    if "--write" not in argv:
        sys.stdout.write(block)
        return 0
    src = open(TARGET).read()
    new, n = re.subn(r"// mc-table begin.*?// mc-table end\n", lambda _: block, src, flags=re.S)
    if n != 1:
        raise SystemExit(f"{TARGET}: no mc-table block")
    with open(TARGET, "w") as f:
        f.write(new)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
