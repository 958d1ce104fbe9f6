"""Generate prv_mc_tables.hpp: the marching-cubes case table, built from first principles instead of typed in.

    python nerf_prv_amd/csrc/gen_mc_tables.py          # rewrites prv_mc_tables.hpp next to this file
    python nerf_prv_amd/csrc/gen_mc_tables.py --check  # exit 1 if the committed header differs

Numbering (the header repeats it):
  corner c in 0..7 sits at (c & 1, (c >> 1) & 1, (c >> 2) & 1)                 (x, y, z offsets in the cell)
  edge e in 0..11: axis = e >> 2, k = e & 3; the edge runs along `axis` from its low corner, whose other two offsets are
    axis 0 (x): (y, z) = (k & 1, k >> 1)   axis 1 (y): (x, z) = (k & 1, k >> 1)   axis 2 (z): (x, y) = (k & 1, k >> 1)
  case = sum over corners of (inside(c) << c); a corner is inside iff sigma > threshold (strict; NaN is outside)

For each case the surface is built face by face:
  1. on each of the 6 faces the crossing edges are joined into segments; a face with 4 crossings (the inside corners on
     a diagonal) always cuts each inside corner off on its own -- the rule reads that face's 4 corner states only, so the
     two cells sharing a face draw the same segments and the mesh is watertight;
  2. every segment is directed so that, seen from outside the cell, the surface's outside (lower sigma) is on a fixed
     side; the directed segments then chain into closed loops (every crossing edge has one segment in and one out);
  3. loops wind counter-clockwise seen from the surface's outside (right-hand normal towards lower sigma);
  4. each loop is fan-triangulated from its lowest-numbered edge -- of those whose fan draws no diagonal between two
     edges of a face with 4 crossings (such a diagonal lies in the face, where the neighbouring cell may draw it too:
     four triangles on one edge); loops are listed by their lowest edge.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "prv_mc_tables.hpp")

CORNERS = np.array([(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)], np.float64)


def edge_corners(e):
    """(low corner, high corner) of edge e"""
    axis, k = e >> 2, e & 3
    off = [0, 0, 0]
    others = [a for a in range(3) if a != axis]
    off[others[0]], off[others[1]] = k & 1, k >> 1
    lo = off[0] | off[1] << 1 | off[2] << 2
    return lo, lo | (1 << axis)


EDGES = [edge_corners(e) for e in range(12)]
MIDS = np.array([(CORNERS[a] + CORNERS[b]) / 2 for a, b in EDGES])


def faces():
    """(outward normal, corners, edges) of the 6 faces"""
    out = []
    for axis in range(3):
        for side in range(2):
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            cs = [c for c in range(8) if ((c >> axis) & 1) == side]
            es = [e for e in range(12) if EDGES[e][0] in cs and EDGES[e][1] in cs]
            out.append((n, cs, es))
    return out


FACES = faces()


def face_segments(case, normal, corners, edges):
    inside = lambda c: (case >> c) & 1
    cross = [e for e in edges if inside(EDGES[e][0]) != inside(EDGES[e][1])]
    if not cross:
        return []
    if len(cross) == 2:
        pairs = [tuple(cross)]
    else:  # 4 crossings: cut off each inside corner of the face on its own
        assert len(cross) == 4
        pairs = []
        for c in corners:
            if inside(c):
                pairs.append(tuple(e for e in cross if c in EDGES[e]))
    segs = []
    for p, q in pairs:
        shared = set(EDGES[p]) & set(EDGES[q])
        mid = (MIDS[p] + MIDS[q]) / 2
        if shared:  # the segment cuts off one corner k
            k = shared.pop()
            m = mid - CORNERS[k] if inside(k) else CORNERS[k] - mid
        else:  # parallel edges: the face's inside half against its outside half
            ins = [CORNERS[c] for c in corners if inside(c)]
            outs = [CORNERS[c] for c in corners if not inside(c)]
            m = np.mean(outs, axis=0) - np.mean(ins, axis=0)
        d = MIDS[q] - MIDS[p]
        # the surface (normal ~ m, towards lower sigma) lies inside the cell, i.e. to the LEFT (m x d) of its boundary
        # when the boundary runs counter-clockwise around that normal: m x d must point into the cell (-normal)
        s = np.dot(np.cross(m, d), normal)
        assert s != 0
        segs.append((p, q) if s < 0 else (q, p))
    return segs


def case_loops(case):
    """-> (loops as lists of edges starting at their lowest edge, pairs of edges that share a face with 4 crossings)"""
    nxt, ambiguous = {}, set()
    for normal, corners, edges in FACES:
        segs = face_segments(case, normal, corners, edges)
        for p, q in segs:
            assert p not in nxt, (case, p)
            nxt[p] = q
        if len(segs) == 2:
            fe = [e for s in segs for e in s]
            ambiguous |= {(a, b) for a in fe for b in fe if a != b}
    assert sorted(nxt) == sorted(nxt.values()), case  # every crossing edge: one segment in, one out
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops, ambiguous


def fan(loop, ambiguous):
    """fan triangles of a loop from its lowest-numbered edge whose diagonals stay off the faces with 4 crossings: a
    diagonal between two edges of such a face would lie in the face, where the neighbouring cell can draw the same one
    (an edge of four triangles, a pinched surface)"""
    n = len(loop)
    for r in sorted(range(n), key=lambda i: loop[i]):
        lp = loop[r:] + loop[:r]
        if not any((lp[0], lp[i]) in ambiguous for i in range(2, n - 1)):
            return [(lp[0], lp[i], lp[i + 1]) for i in range(1, n - 1)]
    raise AssertionError(f"no fan of {loop} avoids the ambiguous faces")


def build_tables():
    """-> (edge_mask[256], triangles: list of 256 lists of (e0, e1, e2))"""
    masks, tris = [], []
    for case in range(256):
        m = 0
        for e, (a, b) in enumerate(EDGES):
            if ((case >> a) & 1) != ((case >> b) & 1):
                m |= 1 << e
        t = []
        loops, ambiguous = case_loops(case)
        for loop in loops:
            t += fan(loop, ambiguous)
        masks.append(m)
        tris.append(t)
    _check_orientation(tris)
    return masks, tris


def _check_orientation(tris):
    """a lone inside corner: every triangle's normal points away from it; a lone outside corner: towards it"""
    for case in range(256):
        ins = [c for c in range(8) if (case >> c) & 1]
        if len(ins) == 1 or len(ins) == 7:
            c = ins[0] if len(ins) == 1 else [k for k in range(8) if k not in ins][0]
            sign = 1.0 if len(ins) == 1 else -1.0
            for a, b, d in tris[case]:
                n = np.cross(MIDS[b] - MIDS[a], MIDS[d] - MIDS[a])
                assert sign * np.dot(n, (MIDS[a] + MIDS[b] + MIDS[d]) / 3 - CORNERS[c]) > 0, case


def render_header():
    masks, tris = build_tables()
    max_tris = max(len(t) for t in tris)
    lines = [
        "// prv_mc_tables.hpp -- marching-cubes case table.  GENERATED by gen_mc_tables.py: do not edit, re-run the generator.",
        "//",
        "// corner c in 0..7 sits at (c & 1, (c >> 1) & 1, (c >> 2) & 1) in the cell (x, y, z offsets)",
        "// edge e in 0..11: axis = e >> 2, k = e & 3; the edge runs along `axis` from its low corner, whose other two offsets are",
        "//   axis 0 (x): (y, z) = (k & 1, k >> 1)   axis 1 (y): (x, z) = (k & 1, k >> 1)   axis 2 (z): (x, y) = (k & 1, k >> 1)",
        "// case = sum over corners of (inside(c) << c); a corner is inside iff sigma > threshold (strict; NaN is outside)",
        "// kMcEdgeMask[case]: bit e set = edge e crosses the surface",
        "// kMcTriCount[case], kMcTris[case]: triangles as edge triples, counter-clockwise seen from the outside (lower sigma),",
        "//   faces with 4 crossings cut each inside corner off on its own (watertight: the rule reads only the face's corners);",
        "//   each loop is fanned from its lowest edge whose diagonals stay off such faces",
        "#pragma once",
        "#include <hip/hip_runtime.h>",
        "#include <stdint.h>",
        "",
        "namespace prv {",
        "",
        f"constexpr int kMcMaxTris = {max_tris};",
        "",
        "__constant__ const uint16_t kMcEdgeMask[256] = {",
    ]
    for r in range(0, 256, 16):
        lines.append("    " + ", ".join(f"0x{m:03x}" for m in masks[r:r + 16]) + ",")
    lines += ["};", "", "__constant__ const uint8_t kMcTriCount[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in tris[r:r + 32]) + ",")
    lines += ["};", "", f"__constant__ const int8_t kMcTris[256][kMcMaxTris * 3] = {{"]
    for case, t in enumerate(tris):
        flat = [e for tri in t for e in tri] + [-1] * (3 * (max_tris - len(t)))
        lines.append("    {" + ", ".join(str(e) for e in flat) + f"}}, // {case}")
    lines += ["};", "", "} // namespace prv", ""]
    return "\n".join(lines)


def main(argv):
    text = render_header()
    if "--check" in argv:
        with open(HEADER) as fh:
            same = fh.read() == text
        print("prv_mc_tables.hpp is " + ("up to date" if same else "STALE: re-run gen_mc_tables.py"))
        return 0 if same else 1
    with open(HEADER, "w") as fh:
        fh.write(text)
    print(f"wrote {HEADER}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
