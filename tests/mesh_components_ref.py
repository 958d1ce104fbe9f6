"""Connected components of a triangle mesh and the floater filter, restated in numpy from their definitions (include/prv.h,
the mesh section) -- not from the kernels.

  connected    two vertices are connected if a triangle uses both; a vertex no triangle uses is a set of its own
  label        the smallest vertex id of a vertex's connected set
  component c  the set whose label is the c-th smallest label; a triangle belongs to the component of its first vertex
  table        per component: first vertex (= its label), vertex count, triangle count, bounding box.  The box is the
               minimum / maximum under the total order of the floats' unsigned images (-0 below +0), as bits
  keep rule    min_triangles, then the keep_largest with the most triangles (ties to the lower id), then min_diagonal with
               the diagonal sqrt((dx*dx + dy*dy) + dz*dz) in float64
  filter       boolean-mask compaction of every array, triangle ids remapped
"""
import numpy as np


def labels(n_vertices, tri):
    """(n,) int64: the smallest vertex id of every vertex's connected set (min-label iteration with pointer jumping)"""
    lab = np.arange(n_vertices, dtype=np.int64)
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    if len(t) == 0:
        return lab
    while True:
        low = lab[t].min(axis=1)  # the smallest label a triangle sees goes to the labels of its three vertices
        new = lab.copy()
        for k in range(3):
            np.minimum.at(new, lab[t[:, k]], low)
        while True:  # pointer jumping: a label is a vertex id, follow it down
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            return lab
        lab = new


def float_key(x):
    """order-preserving unsigned image of float32 values"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def key_float(k):
    k = np.asarray(k, np.uint32)
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def components(vertices, tri):
    """the dict api.Mesh.components() returns, from (n, 3) float32 vertices and (m, 3) triangles"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    lab = labels(len(v), t)
    roots = np.flatnonzero(lab == np.arange(len(v)))  # ascending: the ranking
    rank = np.zeros(len(v), np.int64)
    rank[roots] = np.arange(len(roots))
    vc = rank[lab]
    tc = vc[t[:, 0]] if len(t) else np.zeros(0, np.int64)
    nc = len(roots)
    key = float_key(v)
    lo = np.full((nc, 3), 0xFFFFFFFF, np.uint32)
    hi = np.zeros((nc, 3), np.uint32)
    for a in range(3):
        np.minimum.at(lo[:, a], vc, key[:, a])
        np.maximum.at(hi[:, a], vc, key[:, a])
    return dict(first_vertex=roots.astype(np.uint32), n_vertices=np.bincount(vc, minlength=nc).astype(np.uint64),
                n_triangles=np.bincount(tc, minlength=nc).astype(np.uint64), lo=key_float(lo).reshape(nc, 3), hi=key_float(hi).reshape(nc, 3),
                vertex_component=vc.astype(np.uint32), triangle_component=tc.astype(np.uint32))


def keep_mask(comp, min_triangles=0, keep_largest=0, min_diagonal=0.0):
    """(n_components,) bool"""
    nt = comp["n_triangles"].astype(np.int64)
    keep = np.ones(len(nt), bool)
    if min_triangles > 0:
        keep &= nt >= min_triangles
    if keep_largest > 0:
        ids = np.flatnonzero(keep)
        order = ids[np.lexsort((ids, -nt[ids]))]  # most triangles first, equal counts by ascending id
        keep[order[keep_largest:]] = False
    if min_diagonal > 0:
        d = comp["hi"].astype(np.float64) - comp["lo"].astype(np.float64)
        diag = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        keep &= ~(diag < np.float64(np.float32(min_diagonal)))
    return keep


def compact(comp, keep, vertices, normals, colors, tri):
    """mask compaction -> (vertices, normals, colors, triangles) of the kept components; order kept, ids remapped"""
    vm = keep[comp["vertex_component"]] if len(keep) else np.zeros(0, bool)
    tm = keep[comp["triangle_component"]] if len(keep) else np.zeros(0, bool)
    new_id = np.cumsum(vm) - 1
    t = np.asarray(tri, np.int64).reshape(-1, 3)[tm]
    assert vm[t].all()  # a kept triangle's vertices are kept
    return vertices[vm], normals[vm], colors[vm], new_id[t].astype(np.uint32).reshape(-1, 3)


def filter_mesh(vertices, normals, colors, tri, min_triangles=0, keep_largest=0, min_diagonal=0.0):
    comp = components(vertices, tri)
    return compact(comp, keep_mask(comp, min_triangles, keep_largest, min_diagonal), vertices, normals, colors, tri)


# ---------------------------------------------------------------- test grids (shapes are numpy's (rz, ry, rx); threshold 2.5)
def snake_grid():
    """48 x 48 x 12 (x, y, z): a serpentine tube of eleven rows joined by bends at alternating ends -- one component whose
    graph is 447 hops deep from its smallest vertex, where neighbour-to-neighbour label propagation needs as many rounds --
    and 121 one-point floaters in a layer above it (8 triangles each)"""
    s = np.zeros((12, 48, 48), np.float32)
    for k, y in enumerate(range(3, 45, 4)):
        s[5:7, y:y + 2, 3:45] = 10
        if y + 4 < 45:
            x = 43 if k % 2 == 0 else 3
            s[5:7, y:y + 6, x:x + 2] = 10
    for y in range(2, 46, 4):
        for x in range(2, 46, 4):
            s[10, y, x] = 10
    return s


def touching_cubes(along_edge):
    """8^3: two 2x2x2-point cubes that touch at a grid corner, or along a grid edge: two components either way"""
    s = np.zeros((8, 8, 8), np.float32)
    s[2:4, 2:4, 2:4] = 10
    if along_edge:
        s[2:4, 4:6, 4:6] = 10
    else:
        s[4:6, 4:6, 4:6] = 10
    return s


def crowd_grid(res=96, n=1000, seed=20261019):
    """res^3: n seeded small spheres of random radius (1.2 to 3.5 cells), some overlapping, none at the border"""
    rng = np.random.default_rng(seed)
    s = np.zeros((res, res, res), np.float32)
    centres = rng.uniform(5.0, res - 6.0, (n, 3))
    radii = rng.uniform(1.2, 3.5, n)
    for c, r in zip(centres, radii):
        lo = np.floor(c - r - 1).astype(int)
        hi = np.ceil(c + r + 2).astype(int)
        z, y, x = np.meshgrid(*[np.arange(lo[a], hi[a]) for a in range(3)], indexing="ij")
        d = np.sqrt((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2)
        box = s[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        np.maximum(box, (2.5 + 4.0 * (r - d)).astype(np.float32), out=box)
    return np.maximum(s, 0.0).astype(np.float32)
