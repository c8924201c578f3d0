#!/usr/bin/env python3
"""Generates the marching-cubes case table of the TSDF mesh extraction (include/idh_fusion.h) and writes it to
implicit-depth_amd/csrc/mc_table.h.  The table is derived, not typed in; tests/test_tsdf_mesh_cpu.py asserts that the committed header
is what this file generates.

Numbering (the header's): corner c = dx + 2 dy + 4 dz; case bit c is set when corner c is inside; cube edge e = 4 * axis + j with
axis 0/1/2 = x/y/z and j = first + 2 * second of the lower corner's two other coordinates in x < y < z order.

Construction, per case:
  1. Segments per cube face (faces axis-major, low side first).  The face's four corners are taken in the cyclic order that is
     counter-clockwise seen from outside the cube, and its four edges in that order.  Every maximal cyclic run of inside corners is cut
     off by one segment between the edge where the walk enters the run and the edge where it leaves it: a face with two crossed edges
     has one run and one segment, an ambiguous face (inside corners on a diagonal) has two runs of one corner and the two segments that
     each cut off one inside corner.  The rule sees the face's four signs only, and the neighbouring cell walks the shared face the
     other way round, so the two cells draw the same segments in opposite directions: the mesh is closed.
  2. A cube edge belongs to two faces that walk it in opposite directions, so it is entered by one segment and left by one: the
     segments chain into loops.  Loops start at their lowest edge id and are ordered by it.
  3. Each loop is fan-triangulated from its first vertex.
  4. Orientation: segments run from the enter edge to the leave edge or the other way for ALL cases at once; the direction is chosen
     by one test - the triangle of case 1 (corner 0 inside) must have its right-hand normal pointing away from corner 0, to the
     positive side.

Run `python tools/gen_mc_table.py` to rewrite the header, `--check` to compare only."""
import os
import sys

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "implicit-depth_amd", "csrc", "mc_table.h")
MAX_TRIS = 5


def corner_id(p):
    return p[0] + 2 * p[1] + 4 * p[2]


def edge_id(p, q):
    """Cube edge between corners p and q (coordinate triples that differ along one axis)."""
    axis = [i for i in range(3) if p[i] != q[i]]
    assert len(axis) == 1
    axis = axis[0]
    lo = [min(a, b) for a, b in zip(p, q)]
    first, second = [lo[i] for i in range(3) if i != axis]
    return 4 * axis + first + 2 * second


def edge_corners(e):
    """(lower corner, upper corner) of cube edge e as coordinate triples."""
    axis, j = divmod(e, 4)
    others = [i for i in range(3) if i != axis]
    lo = [0, 0, 0]
    lo[others[0]], lo[others[1]] = j & 1, j >> 1
    hi = list(lo)
    hi[axis] = 1
    return tuple(lo), tuple(hi)


def face_cycles():
    """The six faces (axis-major, low side first): the four corners, counter-clockwise seen from outside the cube."""
    out = []
    for axis in range(3):
        u, v = [i for i in range(3) if i != axis]
        for side in (0, 1):
            cyc = []
            for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[axis], p[u], p[v] = side, a, b
                cyc.append(tuple(p))
            # (u, v) in x < y < z order: e_u x e_v = +e_axis for axis x and z, -e_axis for axis y; outward is +e_axis on the high side
            ccw_from_outside = (axis != 1) == (side == 1)
            out.append(cyc if ccw_from_outside else cyc[::-1])
    return out


FACES = face_cycles()


def face_segments(case):
    """[(enter edge, leave edge)] over the six faces: one per maximal run of inside corners."""
    segs = []
    for cyc in FACES:
        ins = [(case >> corner_id(p)) & 1 for p in cyc]
        for k in range(4):
            if ins[k] and not ins[k - 1]:  # the walk enters a run at corner k
                m = k
                while ins[(m + 1) % 4]:
                    m += 1
                enter = edge_id(cyc[k - 1], cyc[k])
                leave = edge_id(cyc[m % 4], cyc[(m + 1) % 4])
                segs.append((enter, leave))
    return segs


def loops_of(case, flip):
    nxt = {}
    for enter, leave in face_segments(case):
        a, b = (leave, enter) if flip else (enter, leave)
        assert a not in nxt
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())  # every crossed edge: one outgoing, one incoming
    loops, left = [], set(nxt)
    while left:
        start = min(left)
        loop, e = [], start
        while True:
            loop.append(e)
            left.remove(e)
            e = nxt[e]
            if e == start:
                break
        loops.append(loop)
    return loops


def triangles_of(case, flip):
    tris = []
    for loop in loops_of(case, flip):
        assert len(loop) >= 3
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


def _mid(e):
    lo, hi = edge_corners(e)
    return [(a + b) / 2 for a, b in zip(lo, hi)]


def _needs_flip():
    (t,) = triangles_of(1, False)
    a, b, c = (_mid(e) for e in t)
    u, v = [b[i] - a[i] for i in range(3)], [c[i] - a[i] for i in range(3)]
    n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    return sum(n) < 0  # must point away from corner 0, along (1, 1, 1)


FLIP = _needs_flip()
TABLE = [triangles_of(case, FLIP) for case in range(256)]  # TABLE[case] = [(e0, e1, e2), ...]
TRI_COUNT = [len(t) for t in TABLE]
assert max(TRI_COUNT) <= MAX_TRIS


def crossed_edges(case):
    return sorted(e for e in range(12) if ((case >> corner_id(edge_corners(e)[0])) ^ (case >> corner_id(edge_corners(e)[1]))) & 1)


def in_face_diagonals():
    """Interior fan diagonals (edges of a fan that are not loop edges) whose two cube edges lie in one cube face."""
    n = 0
    for case in range(256):
        for loop in loops_of(case, FLIP):
            for i in range(2, len(loop) - 1):
                a, b = set(edge_corners(loop[0])), set(edge_corners(loop[i]))
                pts = a | b
                n += any(len({p[ax] for p in pts}) == 1 for ax in range(3))
    return n


def render():
    lines = [
        "// Marching-cubes case table of the TSDF mesh extraction.  GENERATED by tools/gen_mc_table.py - do not edit; the construction and the",
        "// numbering are described there and in include/idh_fusion.h.  mc_tri_count[case]: triangles of the case; mc_tri_edges[case]: their",
        "// cube edge ids (e = 4 * axis + j), three per triangle, -1 past the end.",
        "#ifndef IDH_MC_TABLE_H_",
        "#define IDH_MC_TABLE_H_",
        "#ifndef IDH_MC_TABLE_ATTR",
        "#define IDH_MC_TABLE_ATTR static const",
        "#endif",
        "",
        "IDH_MC_TABLE_ATTR unsigned char mc_tri_count[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(c) for c in TRI_COUNT[r:r + 32]) + ",")
    lines += ["};", "", "IDH_MC_TABLE_ATTR signed char mc_tri_edges[256][16] = {"]
    for case in range(256):
        flat = [e for t in TABLE[case] for e in t]
        flat += [-1] * (16 - len(flat))
        lines.append("    {" + ", ".join(f"{e:2d}" for e in flat) + "},  // " + f"{case:3d}")
    lines += ["};", "", "#endif  // IDH_MC_TABLE_H_", ""]
    return "\n".join(lines)


def main(argv):
    text = render()
    if "--check" in argv:
        with open(HEADER) as f:
            same = f.read() == text
        print("mc_table.h is up to date" if same else "mc_table.h differs from the generator's output")
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    hist = {k: TRI_COUNT.count(k) for k in sorted(set(TRI_COUNT))}
    print(f"wrote {os.path.normpath(HEADER)}: {sum(TRI_COUNT)} triangles, histogram {hist}, {in_face_diagonals()} in-face fan diagonals")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
