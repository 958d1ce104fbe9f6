"""CPU reference of the marching-cubes pipeline (numpy; test infrastructure).

Reads the case table through the generator (nerf_prv_amd/csrc/gen_mc_tables.py), never through the HIP code, and
states the kernels' output order and arithmetic (nerf_prv_amd/csrc/prv_mesh.hip):
  * vertices in edge-id order, edge id = 3 * point + axis, points numbered x fastest;
  * grid point i on axis a at lo[a] + float(i) * step[a], step[a] = (hi[a] - lo[a]) / float(res[a] - 1), all fp32;
  * vertex = pa + t * (pb - pa) per component, t = (thr - sa) / (sb - sa), fp32, no fma; a NaN t (an infinite or NaN end,
    or a difference that overflows) becomes 0.5 -- on a crossing edge nothing else can leave [0, 1];
  * normal = -(ga + t * (gb - ga)) normalised; g = central differences of sigma, one-sided at the border; (0, 0, 0) where
    the squared length is 0, infinite or NaN;
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


def crossing_edges(sigma, threshold):
    """the crossing edges of a (rz, ry, rx) grid in edge-id order -> (inside, vid, ia, ib): the corner states, the vertex
    id of every edge id (valid where the edge crosses), and per vertex the (x, y, z) indices of its edge's two ends"""
    rz, ry, rx = sigma.shape
    inside = sigma > np.float32(threshold)  # NaN compares false: outside
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
    return inside, vid, ia, ib


def cell_cases(inside):
    """(rz - 1, ry - 1, rx - 1) case of every cell: bit c = corner c inside"""
    rz, ry, rx = inside.shape
    ins = inside.astype(np.int64)
    case = np.zeros((rz - 1, ry - 1, rx - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[dz:dz + rz - 1, dy:dy + ry - 1, dx:dx + rx - 1] << c
    return case


def marching_cubes(sigma, lo=(0, 0, 0), hi=(1, 1, 1), threshold=2.5):
    """sigma: (rz, ry, rx) float32 -> (vertices (n, 3) f32, normals (n, 3) f32, triangles (m, 3) uint32)"""
    f = np.float32
    sigma = np.ascontiguousarray(sigma, np.float32)
    rz, ry, rx = sigma.shape
    res = (rx, ry, rz)
    thr = f(threshold)
    inside, vid, ia, ib = crossing_edges(sigma, thr)
    axes = grid_axes(res, lo, hi)
    pa = np.stack([axes[a][ia[:, a]] for a in range(3)], 1)
    pb = np.stack([axes[a][ib[:, a]] for a in range(3)], 1)
    sa = sigma[ia[:, 2], ia[:, 1], ia[:, 0]]
    sb = sigma[ib[:, 2], ib[:, 1], ib[:, 0]]
    with np.errstate(all="ignore"):
        t = ((thr - sa) / (sb - sa)).astype(np.float32)
        t = np.where(np.isnan(t), f(0.5), t)
        verts = (pa + t[:, None] * (pb - pa)).astype(np.float32)
        g = gradient(sigma, res, lo, hi)
        ga = g[ia[:, 2], ia[:, 1], ia[:, 0]]
        gb = g[ib[:, 2], ib[:, 1], ib[:, 0]]
        n = -(ga + t[:, None] * (gb - ga))
        n2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        inv = np.where(n2 > 0, f(1) / np.sqrt(n2), f(0)).astype(np.float32)
        normals = np.where(np.isfinite(n2)[:, None], n * inv[:, None], f(0)).astype(np.float32)
    # cells: case, then triangles in cell order
    _, tri_tab, ntri = tables()
    case = cell_cases(inside).reshape(-1)
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


# ---------------------------------------------------------------- test grids (seeded; shapes are numpy's (rz, ry, rx))
def adversarial_grids():
    """20 seeded sigma grids up to 24^3 whose surface stays off the border -> [(sigma, threshold)]"""
    rng = np.random.default_rng(20261016)
    out = []
    for k in range(14):
        shape = tuple(int(x) for x in rng.integers(5, 25, size=3))
        out.append((rng.random(shape).astype(np.float32), 0.5))
    for n in (6, 11, 17):  # checkerboards: every face of every interior cell ambiguous
        z, y, x = np.indices((n, n + 1, n + 2))
        out.append((((x + y + z) % 2).astype(np.float32), 0.5))
    for n in (8, 13, 24):  # all-ambiguous faces in two directions, random values
        z, y, x = np.indices((n, n, n))
        s = np.where((x + y) % 2 == 0, 1.0 + rng.random((n, n, n)), rng.random((n, n, n)) * 0.5)
        out.append((s.astype(np.float32), 0.75))
    grids = []
    for s, thr in out:
        s = s.copy()
        s[0], s[-1], s[:, 0], s[:, -1], s[:, :, 0], s[:, :, -1] = 0, 0, 0, 0, 0, 0
        grids.append((s, thr))
    return grids


# (2, 2, 31) is 124 points, a full wave and a partly empty one; (2, 2, 15), 60 points, is the single, partly empty wave
THIN_SHAPES = ((2, 2, 2), (2, 3, 5), (2, 2, 31), (33, 2, 2), (2, 40, 2), (9, 9, 2), (3, 3, 3), (2, 2, 15))
# the ends (a, b) of one edge that the non-finite grids hold along every axis; 0.25 is outside and 0.75 inside at 0.5
NONFINITE_PAIRS = ((np.inf, 0.25), (0.75, -np.inf), (np.nan, 0.75), (np.inf, np.nan), (np.inf, -np.inf))


def _nonfinite(rng, block):
    s = rng.random((14, 15, 16)).astype(np.float32)
    kind = rng.random(s.shape)
    s[kind < 0.03] = np.inf
    s[(kind >= 0.03) & (kind < 0.06)] = -np.inf
    s[(kind >= 0.06) & (kind < 0.09)] = np.nan
    if block:  # gradients inside are inf - inf
        s[5:8, 6:9, 9:12] = np.inf
    for ax in range(3):  # numpy axis the pair lies along
        for p, (a, b) in enumerate(NONFINITE_PAIRS):
            at = [2 + 2 * p, 2 + 4 * ax, 4]
            s[tuple(at)] = a
            at[ax] += 1
            s[tuple(at)] = b
    return s


def edge_grids():
    """small sigma grids at the edges of the kernels' domain -> [(name, sigma, threshold)]: scans with a ragged last chunk
    and dense counts, grids of a cell or a wave, values on the threshold, signed zeros, subnormals, differences that
    overflow, infinities and NaNs.  Their surfaces are open (they reach the border)."""
    f = np.float32

    def rng(k):
        return np.random.default_rng([20261018, k])

    out = [("noise_ragged_scan", rng(0).random((65, 64, 64)).astype(f), 0.5),  # 4160 waves: a full scan chunk + 64
           ("noise_4097_waves", rng(1).random((197, 11, 121)).astype(f), 0.5),  # 4096 * 64 + 63 points
           # thin slices: the last scan chunk's waves still hold cells, so the triangle offsets cross the chunk border too
           ("noise_ragged_cells", rng(2).random((977, 17, 16)).astype(f), 0.5)]
    for k, shape in enumerate(THIN_SHAPES):
        out.append(("thin_%dx%dx%d" % shape, rng(10 + k).random(shape).astype(f), 0.5))
    plateau = rng(20).integers(0, 4, (20, 21, 22)).astype(f)
    out += [("plateau_thr1", plateau, 1.0), ("plateau_thr2", plateau, 2.0)]
    r = rng(30)
    signed = (r.random((15, 16, 17)) * 2.0 - 1.0).astype(f)
    signed[r.random(signed.shape) < 0.05] = -0.0
    out += [("signed_thr0", signed, 0.0), ("signed_thr-0.25", signed, -0.25)]
    r = rng(40)
    sub = r.integers(0, 1 << 20, (12, 13, 14)).astype(np.uint32).view(f)  # k * 2^-149: the bit pattern of k
    sub[r.random(sub.shape) < 0.25] = 0.0
    out.append(("subnormal", sub, 0.0))
    huge = rng(50).choice(np.array([3e38, -3e38, 1e38, -1e38], f), (10, 11, 12))
    # 3e38: nothing is above it, an empty mesh; 1e38 (added): thr - sa and sb - sa both overflow, t = inf / inf
    out += [("huge_thr0", huge, 0.0), ("huge_thr3e38", huge, 3.0e38), ("huge_thr1e38", huge, 1.0e38)]
    out += [("nonfinite", _nonfinite(rng(60), False), 0.5), ("nonfinite_block", _nonfinite(rng(61), True), 0.5)]
    return out
