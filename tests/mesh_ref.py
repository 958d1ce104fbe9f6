"""CPU reference of the marching-cubes pipeline (numpy; test infrastructure).

Reads the case table through the generator (nerf_prv_amd/csrc/gen_mc_tables.py), never through the HIP code, and
states the kernels' output order and arithmetic (nerf_prv_amd/csrc/prv_mesh.hip):
  * vertices in edge-id order, edge id = 3 * point + axis, points numbered x fastest;
  * grid point i on axis a at lo[a] + float(i) * step[a], step[a] = (hi[a] - lo[a]) / float(res[a] - 1), all fp32;
  * vertex = pa + t * (pb - pa) per component, t = (thr - sa) / (sb - sa), fp32, no fma;
  * normal = -(ga + t * (gb - ga)) normalised; g = central differences of sigma, one-sided at the border;
  * triangles in cell order (x fastest), each cell's in table order, as vertex ids.
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN_PATH = os.path.join(ROOT, "nerf_prv_amd", "csrc", "gen_mc_tables.py")

_tables = None


def generator():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", GEN_PATH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tables():
    """-> (edge_mask[256], tri[256, max_tris, 3] edge ids with -1 padding, ntri[256])"""
    global _tables
    if _tables is None:
        masks, tris = generator().build_tables()
        mt = max(len(t) for t in tris)
        arr = np.full((256, mt, 3), -1, np.int64)
        for c, t in enumerate(tris):
            if t:
                arr[c, :len(t)] = t
        _tables = (np.array(masks, np.int64), arr, np.array([len(t) for t in tris], np.int64))
    return _tables


def grid_axes(res, lo, hi):
    """per axis the fp32 coordinates of the grid points (x, y, z order)"""
    f = np.float32
    axes = []
    for a in range(3):
        step = (f(hi[a]) - f(lo[a])) / f(res[a] - 1)
        axes.append(f(lo[a]) + np.arange(res[a]).astype(np.float32) * step)
    return axes


def gradient(sigma, res, lo, hi):
    """(rz, ry, rx, 3) central differences (x, y, z components), one-sided at the border, fp32"""
    f = np.float32
    s = sigma.astype(np.float32)
    g = np.zeros(s.shape + (3,), np.float32)
    for a in range(3):
        ax = 2 - a  # numpy axis of grid axis a
        n = res[a]
        step = (f(hi[a]) - f(lo[a])) / f(n - 1)
        i = np.arange(n)
        ip, im = np.minimum(i + 1, n - 1), np.maximum(i - 1, 0)
        den = (ip - im).astype(np.float32) * step
        diff = np.take(s, ip, axis=ax) - np.take(s, im, axis=ax)
        shape = [1, 1, 1]
        shape[ax] = n
        g[..., a] = diff / den.reshape(shape)
    return g


def marching_cubes(sigma, lo=(0, 0, 0), hi=(1, 1, 1), threshold=2.5):
    """sigma: (rz, ry, rx) float32 -> (vertices (n, 3) f32, normals (n, 3) f32, triangles (m, 3) uint32)"""
    f = np.float32
    sigma = np.ascontiguousarray(sigma, np.float32)
    rz, ry, rx = sigma.shape
    res = (rx, ry, rz)
    thr = f(threshold)
    inside = sigma > thr  # NaN compares false: outside
    # crossing flags of every point's +x, +y, +z edge
    cross = np.zeros(sigma.shape + (3,), bool)
    cross[:, :, :-1, 0] = inside[:, :, :-1] != inside[:, :, 1:]
    cross[:, :-1, :, 1] = inside[:, :-1, :] != inside[:, 1:, :]
    cross[:-1, :, :, 2] = inside[:-1, :, :] != inside[1:, :, :]
    flat = cross.reshape(-1)  # edge id order: 3 * point + axis
    vid = np.cumsum(flat) - 1
    eids = np.nonzero(flat)[0]
    pts, axis = eids // 3, eids % 3
    pz, rem = pts // (rx * ry), pts % (rx * ry)
    py, px = rem // rx, rem % rx
    ia = np.stack([px, py, pz], 1)
    ib = ia.copy()
    ib[np.arange(len(ib)), axis] += 1
    axes = grid_axes(res, lo, hi)
    pa = np.stack([axes[a][ia[:, a]] for a in range(3)], 1)
    pb = np.stack([axes[a][ib[:, a]] for a in range(3)], 1)
    sa = sigma[ia[:, 2], ia[:, 1], ia[:, 0]]
    sb = sigma[ib[:, 2], ib[:, 1], ib[:, 0]]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((thr - sa) / (sb - sa)).astype(np.float32)
        verts = (pa + t[:, None] * (pb - pa)).astype(np.float32)
        g = gradient(sigma, res, lo, hi)
        ga = g[ia[:, 2], ia[:, 1], ia[:, 0]]
        gb = g[ib[:, 2], ib[:, 1], ib[:, 0]]
        n = -(ga + t[:, None] * (gb - ga))
        n2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        inv = np.where(n2 > 0, f(1) / np.sqrt(n2), f(0)).astype(np.float32)
        normals = (n * inv[:, None]).astype(np.float32)
    # cells: case, then triangles in cell order
    _, tri_tab, ntri = tables()
    ins = inside.astype(np.int64)
    case = np.zeros((rz - 1, ry - 1, rx - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[dz:dz + rz - 1, dy:dy + ry - 1, dx:dx + rx - 1] << c
    case = case.reshape(-1)
    cz, crem = np.divmod(np.arange(case.size), (rx - 1) * (ry - 1))
    cy, cx = np.divmod(crem, rx - 1)
    base = cx + rx * (cy + ry * cz)
    keep = ntri[case] > 0
    case, base = case[keep], base[keep]
    edges = tri_tab[case]  # (cells, max_tris, 3)
    valid = edges[:, :, 0] >= 0
    e = np.where(edges >= 0, edges, 0)
    ax, k = e >> 2, e & 3
    lo_bit, hi_bit = k & 1, k >> 1
    ox = np.where(ax == 0, 0, lo_bit)
    oy = np.where(ax == 0, lo_bit, np.where(ax == 1, 0, hi_bit))
    oz = np.where(ax == 2, 0, hi_bit)
    q = base[:, None, None] + ox + rx * (oy + ry * oz)
    gid = 3 * q + ax
    tri = vid[gid][valid]
    return verts, normals, tri.astype(np.uint32).reshape(-1, 3)


def edge_use(tri):
    """{(a, b): count} of directed mesh edges"""
    d = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)
    keys, counts = np.unique(d[:, 0] * (1 << 32) + d[:, 1], return_counts=True)
    return dict(zip(keys.tolist(), counts.tolist()))


def is_closed_manifold(tri):
    """every undirected edge in exactly two triangles, once in each direction"""
    use = edge_use(tri)
    for key, n in use.items():
        a, b = key >> 32, key & 0xFFFFFFFF
        if n != 1 or use.get((b << 32) | a, 0) != 1:
            return False
    return True


def signed_volume(verts, tri):
    v = verts.astype(np.float64)
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def euler_characteristic(n_vertices, tri):
    d = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64), axis=1)
    n_edges = len(np.unique(d[:, 0] * (1 << 32) + d[:, 1]))
    used = len(np.unique(tri))
    return used - n_edges + len(tri), used == n_vertices
