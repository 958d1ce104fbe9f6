"""CPU reference of depth-map fusion (test infrastructure, in the spirit of tests/coverage_ref.py and tests/raster_ref.py).

Restates the contracts of prv_tsdf_integrate, prv_tsdf_grid, prv_tsdf_info, prv_tsdf_mesh and prv_marching_cubes_grid_valid
(include/prv.h) in numpy float32, operation by operation.  f32 and fmaf are tests/march_ref.py's (a float64 product and sum,
rounded to float32), the projection is tests/coverage_ref.py's, the grid and the unmasked extraction tests/mesh_ref.py's; nothing
here is shared with prv_tsdf.hip or prv_mesh.hip.
"""
import numpy as np

from tests import mesh_ref
from tests.coverage_ref import project
from tests.march_ref import f32, fmaf

INF = f32(np.inf)


class Volume:
    """res = (rx, ry, rz), lo / hi the box (engine frame), trunc in engine units.  State: D, W, WC (n,) and C (3, n) float32, the
    points numbered x fastest"""

    def __init__(self, res, lo, hi, trunc, colors=True):
        self.res = tuple(int(r) for r in res)
        self.lo, self.hi = tuple(float(x) for x in lo), tuple(float(x) for x in hi)
        axes = mesh_ref.grid_axes(self.res, self.lo, self.hi)
        z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        self.points = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)
        self.n = len(self.points)
        self.trunc = f32(trunc)
        self.inv = f32(f32(1) / self.trunc)  # formed once
        self.colors = bool(colors)
        self.D, self.W, self.WC = (np.zeros(self.n, np.float32) for _ in range(3))
        self.C = np.zeros((3, self.n), np.float32)

    def integrate(self, cams, w, h, depth, weight=None, rgba8=None):
        """cams: coverage_ref.Cam per view at w x h, in list order; depth / weight (n_views, h, w) float32, rgba8 (n_views, h,
        w, 4) uint8"""
        depth = np.asarray(depth, np.float32).reshape(len(cams), h, w)
        weight = None if weight is None else np.asarray(weight, np.float32).reshape(len(cams), h, w)
        rgba8 = None if rgba8 is None else np.asarray(rgba8, np.uint8).reshape(len(cams), h, w, 4)
        for j, cam in enumerate(cams):
            with np.errstate(all="ignore"):
                # 1. the projection and the pixel
                ok, u, v, z = project(cam, self.points)
                fu, fv = np.floor(u), np.floor(v)
                ok = ok & (fu >= 0) & (fu < f32(w)) & (fv >= 0) & (fv < f32(h))  # a NaN fails
                xi, yi = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
                # 2. depth and weight
                d = depth[j][yi, xi]
                ws = weight[j][yi, xi] if weight is not None else np.ones(self.n, np.float32)
                ok = ok & (d > 0) & (d < INF) & (ws > 0) & (ws < INF)
                # 3. the signed distance
                sdf = d - z
                ok = ok & ~(sdf < -self.trunc)
                # 4. distance and weight
                s = np.minimum(sdf * self.inv, f32(1))
                Wn = self.W + ws
                Dn = fmaf(self.D, self.W, s * ws) / Wn
                self.D = np.where(ok, Dn, self.D).astype(np.float32)
                # 5. colour, with the weight it had before this view
                if self.colors and rgba8 is not None:
                    paint = ok & (sdf <= self.trunc)
                    WCn = self.WC + ws
                    px = rgba8[j][yi, xi]
                    for k in range(3):
                        Cn = fmaf(self.C[k], self.WC, px[:, k].astype(np.float32) * ws) / WCn
                        self.C[k] = np.where(paint, Cn, self.C[k]).astype(np.float32)
                    self.WC = np.where(paint, WCn, self.WC).astype(np.float32)
                self.W = np.where(ok, Wn, self.W).astype(np.float32)

    def shaped(self, a):
        rx, ry, rz = self.res
        return a.reshape(a.shape[:-1] + (rz, ry, rx))

    def grid(self, min_weight=0.0):
        """-> (grid (rz, ry, rx) float32: -D, NaN where not valid; valid (rz, ry, rx) bool)"""
        valid = (self.W > 0) & (self.W >= f32(min_weight))
        return self.shaped(np.where(valid, -self.D, f32(np.nan)).astype(np.float32)), self.shaped(valid)

    def info(self):
        obs = self.W > 0
        return dict(points=self.n, observed=int(obs.sum()), inside=int((obs & (self.D < 0)).sum()),
                    band=int((obs & (np.abs(self.D) < 1)).sum()))

    def mesh(self, min_weight=0.0):
        """-> (vertices, normals, colours (n, 3) uint8, triangles): prv_tsdf_mesh"""
        grid, valid = self.grid(min_weight)
        v, nrm, tri = masked_marching_cubes(grid, valid, self.lo, self.hi, 0.0)
        rgb = np.zeros((len(v), 3), np.uint8)
        if self.colors and len(v):
            f = np.float32
            at, stride = np.zeros(len(v), np.int64), 1
            for a in range(3):
                step = (f(self.hi[a]) - f(self.lo[a])) / f(self.res[a] - 1)
                q = np.rint((v[:, a] - f(self.lo[a])) / step)  # float32 throughout; round half to even
                at += np.clip(q.astype(np.int64), 0, self.res[a] - 1) * stride
                stride *= self.res[a]
            has = self.WC[at] > 0
            for k in range(3):
                byte = np.minimum(f(255), np.floor(self.C[k][at] + f(0.5)))
                rgb[:, k] = np.where(has, byte, 0).astype(np.uint8)
        return v, nrm, rgb, tri


def look_at(eye, target, w, h, fov_x, up=(0.0, 0.0, 1.0)):
    """a pinhole coverage_ref.Cam at `eye` looking at `target` (engine frame): the columns of c2w are right, down, forward, the
    depth of the projection is the distance along forward; principal point at the image centre"""
    from tests.coverage_ref import Cam

    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, np.asarray(up, np.float64))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w = np.stack([right, down, fwd, eye], 1).astype(np.float32)
    fx = 0.5 * w / np.tan(0.5 * fov_x)
    return Cam(c2w, fx, fx, 0.5 * w, 0.5 * h)


def adversarial_images(rng, n_views, w, h, z0, first=None):
    """depth, weight (n_views, h, w) float32 and rgba8 (n_views, h, w, 4) uint8 around a plane at depth z0 (per pixel z0 plus a
    little noise) with every value a view must skip sown in: depths 0, -0, negative, NaN, +Inf, -Inf; weights 0, negative, NaN, Inf.
    Each of 24 kinds (10 bad, 14 good) takes a 24th of the pixels, dealt out over a random order of them; `first` (flat pixel
    indices) go to the head of that order, so a caller can make sure that pixels of its choice get every kind.
    -> (depth, weight, rgba8, bad_depth, bad_weight) with the two (n_views, h, w) bool masks of the sown pixels"""
    depth = (z0 + 0.05 * rng.standard_normal((n_views, h, w))).astype(np.float32)
    weight = rng.uniform(0.25, 2.0, (n_views, h, w)).astype(np.float32)
    rgba8 = rng.integers(0, 256, (n_views, h, w, 4)).astype(np.uint8)
    order = rng.permutation(n_views * h * w)
    if first is not None:
        first = np.unique(np.asarray(first, np.int64))
        order = np.concatenate([first, order[~np.isin(order, first)]])
    kind = np.zeros(n_views * h * w, np.int64)
    kind[order] = np.arange(len(order)) % 24
    kind = kind.reshape(n_views, h, w)
    for k, val in enumerate((0.0, -0.0, -1.5, np.nan, np.inf, -np.inf)):
        depth[kind == k] = val
    for k, val in enumerate((0.0, -0.5, np.nan, np.inf)):
        weight[kind == 8 + k] = val
    return depth, weight, rgba8, kind < 6, (kind >= 8) & (kind < 12)


def kept_cells(valid):
    """(rz, ry, rx) bool -> (rz - 1, ry - 1, rx - 1) bool: all eight corners valid"""
    valid = np.asarray(valid, bool)
    rz, ry, rx = valid.shape
    kept = np.ones((rz - 1, ry - 1, rx - 1), bool)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        kept &= valid[dz:dz + rz - 1, dy:dy + ry - 1, dx:dx + rx - 1]
    return kept


def masked_marching_cubes(grid, valid, lo=(0, 0, 0), hi=(1, 1, 1), threshold=0.0):
    """prv_marching_cubes_grid_valid: the reference mesh of the grid with the triangles of the cells that are not kept dropped
    and the then-unused vertices removed, order preserved.  valid None: mesh_ref.marching_cubes itself"""
    v, nrm, tri = mesh_ref.marching_cubes(grid, lo, hi, threshold)
    if valid is None:
        return v, nrm, tri
    grid = np.asarray(grid, np.float32)
    rz, ry, rx = grid.shape
    # the cell of every triangle: mesh_ref emits them in cell order, each cell's ntri[case] in a row
    _, _, ntri = mesh_ref.tables()
    case = mesh_ref.cell_cases(grid > np.float32(threshold)).reshape(-1)
    keep_tri = np.repeat(kept_cells(valid).reshape(-1), ntri[case])
    assert len(keep_tri) == len(tri)
    tri = tri[keep_tri]
    used = np.zeros(len(v), bool)
    used[tri.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    return v[used], nrm[used], new_id[tri].astype(np.uint32).reshape(-1, 3)
