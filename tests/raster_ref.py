"""CPU reference of the triangle rasteriser (test infrastructure, in the spirit of tests/coverage_ref.py).

Restates the contract of prv_mesh_depth and prv_coverage_create_occluded (include/prv.h, "mesh depth and the mesh occluder") in
numpy: the projection is tests/coverage_ref.py's float32 restatement, the snap is one float32 multiply and a round half to even,
the edge functions are exact int64, the depth is float64 operation by operation, and the buffer is a minimum over uint32 keys.
Nothing here is shared with prv_raster.hip.
"""
import numpy as np

from tests import coverage_ref
from tests.march_ref import f32

NEVER = coverage_ref.NEVER
WALK = 6  # boxes of at most WALK x WALK pixels are walked offset by offset, all such triangles at once; larger ones one at a time


def edge(xp, yp, xq, yq, px, py):
    """E_pq(P) = (Xq - Xp)(Py - Yp) - (Yq - Yp)(Px - Xp), int64"""
    return (xq - xp) * (py - yp) - (yq - yp) * (px - xp)


class Setup:
    """the triangles of a mesh that can write something in one view: snapped and oriented vertices (int64), A2, the inverse
    depths (float64), the clipped pixel boxes (inclusive) and the triangles' ids"""

    def __init__(self, cam, vertices, triangles, w, h):
        vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
        tri = np.asarray(triangles, np.int64).reshape(-1, 3)
        if len(tri) == 0 or len(vertices) == 0:
            self.ids = np.zeros(0, np.int64)
            return
        ok, u, v, z = coverage_ref.project(cam, vertices)
        with np.errstate(all="ignore"):
            ok = ok & (np.abs(u) < f32(32768)) & (np.abs(v) < f32(32768))  # a NaN fails
            X = np.where(ok, np.rint(u * f32(256)), 0).astype(np.int64)  # float32 product, round half to even
            Y = np.where(ok, np.rint(v * f32(256)), 0).astype(np.int64)
            inv = np.where(ok, 1.0 / np.where(ok, z, f32(1)).astype(np.float64), 0.0)
        keep = ok[tri].all(axis=1)
        xa, ya, xb, yb, xc, yc = X[tri[:, 0]], Y[tri[:, 0]], X[tri[:, 1]], Y[tri[:, 1]], X[tri[:, 2]], Y[tri[:, 2]]
        ia, ib, ic = inv[tri[:, 0]], inv[tri[:, 1]], inv[tri[:, 2]]
        a2 = edge(xa, ya, xb, yb, xc, yc)
        keep &= a2 != 0
        flip = a2 < 0  # b <-> c
        xb, xc = np.where(flip, xc, xb), np.where(flip, xb, xc)
        yb, yc = np.where(flip, yc, yb), np.where(flip, yb, yc)
        ib, ic = np.where(flip, ic, ib), np.where(flip, ib, ic)
        a2 = np.abs(a2)
        lox, hix = np.minimum(xa, np.minimum(xb, xc)), np.maximum(xa, np.maximum(xb, xc))
        loy, hiy = np.minimum(ya, np.minimum(yb, yc)), np.maximum(ya, np.maximum(yb, yc))
        # centres 256 x + 128 within [lo, hi]: x = ceil((lo - 128) / 256) .. floor((hi - 128) / 256), clipped to the image
        x0, x1 = np.maximum(-((128 - lox) // 256), 0), np.minimum((hix - 128) // 256, w - 1)
        y0, y1 = np.maximum(-((128 - loy) // 256), 0), np.minimum((hiy - 128) // 256, h - 1)
        keep &= (x1 >= x0) & (y1 >= y0)
        for name, a in dict(xa=xa, ya=ya, xb=xb, yb=yb, xc=xc, yc=yc, ia=ia, ib=ib, ic=ic, a2=a2, x0=x0, x1=x1, y0=y0, y1=y1).items():
            setattr(self, name, a[keep])
        self.ids = np.nonzero(keep)[0]

    def box_pixels(self):
        return (self.x1 - self.x0 + 1) * (self.y1 - self.y0 + 1)


def _write(keys, s, sel, x, y):
    """triangles sel (index array into the setup) at pixels (x, y), one pixel per triangle (or one triangle, many pixels)"""
    px, py = 256 * x + 128, 256 * y + 128
    wa = edge(s.xb[sel], s.yb[sel], s.xc[sel], s.yc[sel], px, py)
    wb = edge(s.xc[sel], s.yc[sel], s.xa[sel], s.ya[sel], px, py)
    wc = edge(s.xa[sel], s.ya[sel], s.xb[sel], s.yb[sel], px, py)
    inside = (wa >= 0) & (wb >= 0) & (wc >= 0)
    if not inside.any():
        return
    a2 = np.broadcast_to(s.a2[sel], inside.shape)[inside]
    ia, ib, ic = (np.broadcast_to(i[sel], inside.shape)[inside] for i in (s.ia, s.ib, s.ic))
    iz = (wa[inside].astype(np.float64) * ia + wb[inside].astype(np.float64) * ib) + wc[inside].astype(np.float64) * ic
    z = (a2.astype(np.float64) / iz).astype(np.float32)
    np.minimum.at(keys, (np.broadcast_to(y, inside.shape)[inside], np.broadcast_to(x, inside.shape)[inside]), z.view(np.uint32))


def depth_keys(cam, vertices, triangles, w, h):
    """-> (h, w) uint32: the bits of the nearest depth, NEVER where no triangle covers the pixel's centre"""
    keys = np.full((h, w), NEVER, np.uint32)
    s = Setup(cam, vertices, triangles, w, h)
    if len(s.ids) == 0:
        return keys
    bw, bh = s.x1 - s.x0 + 1, s.y1 - s.y0 + 1
    small = (bw <= WALK) & (bh <= WALK)
    for j in range(WALK):
        for i in range(WALK):
            sel = np.nonzero(small & (i < bw) & (j < bh))[0]
            if len(sel):
                _write(keys, s, sel, s.x0[sel] + i, s.y0[sel] + j)
    for k in np.nonzero(~small)[0]:  # one triangle at a time over its clipped box
        ys, xs = np.mgrid[s.y0[k]:s.y1[k] + 1, s.x0[k]:s.x1[k] + 1]
        _write(keys, s, np.full(xs.size, k), xs.ravel(), ys.ravel())
    return keys


def depth(cam, vertices, triangles, w, h):
    """-> (h, w) float32, 0 where empty: what prv_mesh_depth writes for one view"""
    keys = depth_keys(cam, vertices, triangles, w, h)
    return np.where(keys == NEVER, np.uint32(0), keys).view(np.float32)


def visible(cam, points, keys, w, h, depth_tol):
    """stage B with a mesh's buffer -> (n,) bool: an empty pixel passes"""
    ok, u, v, z = coverage_ref.project(cam, points)
    tol1 = f32(f32(1) + f32(depth_tol))
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u), np.floor(v)
        ok = ok & (fu >= 0) & (fu < f32(w)) & (fv >= 0) & (fv < f32(h))
    vis = np.zeros(len(z), bool)
    if ok.any():
        k = keys[fv[ok].astype(np.int64), fu[ok].astype(np.int64)]
        with np.errstate(all="ignore"):
            vis[ok] = (k == NEVER) | (z[ok] <= k.view(np.float32) * tol1)  # float32 * float32: one rounding; NaN <= is False
    return vis


def matrix(cams, points, vertices, triangles, w, h, depth_tol=0.02):
    """-> (vis (n_views, n) bool, depth (n_views, h, w) float32)"""
    vis, depths = [], []
    for cam in cams:
        keys = depth_keys(cam, vertices, triangles, w, h)
        vis.append(visible(cam, points, keys, w, h, depth_tol))
        depths.append(np.where(keys == NEVER, np.uint32(0), keys).view(np.float32))
    return np.stack(vis), np.stack(depths)
