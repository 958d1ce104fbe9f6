"""CPU reference of the colour images of a mesh (test infrastructure, in the spirit of tests/raster_ref.py).

Restates the contract of prv_mesh_render (include/prv.h, "mesh colour images") in numpy: stage A is the setup of
tests/raster_ref.py (projection, snap, orientation, clipped boxes) with a minimum over uint64 keys, bits of the depth << 32 |
triangle id; stage B forms the edge functions again at each covered pixel and interpolates the vertex colours in float64,
operation by operation; then the alpha rule and the 180-degree turn.  Nothing here is shared with prv_raster.hip.
"""
import numpy as np

from tests import coverage_ref, raster_ref
from tests.march_ref import f32

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_TRIANGLE = 0xFFFFFFFF
BACKGROUND = (255, 255, 255, 0)
edge = raster_ref.edge


def _weights(s, sel, x, y):
    px, py = 256 * x + 128, 256 * y + 128
    wa = edge(s.xb[sel], s.yb[sel], s.xc[sel], s.yc[sel], px, py)
    wb = edge(s.xc[sel], s.yc[sel], s.xa[sel], s.ya[sel], px, py)
    wc = edge(s.xa[sel], s.ya[sel], s.xb[sel], s.yb[sel], px, py)
    return wa, wb, wc


def _products(s, sel, wa, wb, wc):
    """p_a, p_b, p_c and iz = (p_a + p_b) + p_c, float64"""
    pa, pb, pc = wa.astype(np.float64) * s.ia[sel], wb.astype(np.float64) * s.ib[sel], wc.astype(np.float64) * s.ic[sel]
    return pa, pb, pc, (pa + pb) + pc


def _write(keys, s, sel, x, y):
    """triangles sel (rows of the setup) at pixels (x, y), one pixel per entry"""
    sel, x, y = np.broadcast_arrays(sel, x, y)
    wa, wb, wc = _weights(s, sel, x, y)
    inside = (wa >= 0) & (wb >= 0) & (wc >= 0)
    if not inside.any():
        return
    sel, x, y = sel[inside], x[inside], y[inside]
    iz = _products(s, sel, wa[inside], wb[inside], wc[inside])[3]
    z = (s.a2[sel].astype(np.float64) / iz).astype(np.float32)
    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | s.ids[sel].astype(np.uint64)
    np.minimum.at(keys, (y, x), key)


def visibility_keys(cam, vertices, triangles, w, h, setup=None):
    """stage A -> (h, w) uint64: (bits of the nearest depth << 32) | the lowest id among the triangles at that depth; EMPTY
    where no triangle covers the pixel's centre"""
    keys = np.full((h, w), EMPTY, np.uint64)
    s = setup if setup is not None else raster_ref.Setup(cam, vertices, triangles, w, h)
    if len(s.ids) == 0:
        return keys
    bw, bh = s.x1 - s.x0 + 1, s.y1 - s.y0 + 1
    small = (bw <= raster_ref.WALK) & (bh <= raster_ref.WALK)
    for j in range(raster_ref.WALK):
        for i in range(raster_ref.WALK):
            sel = np.nonzero(small & (i < bw) & (j < bh))[0]
            if len(sel):
                _write(keys, s, sel, s.x0[sel] + i, s.y0[sel] + j)
    for k in np.nonzero(~small)[0]:  # one triangle at a time over its clipped box
        ys, xs = np.mgrid[s.y0[k]:s.y1[k] + 1, s.x0[k]:s.x1[k] + 1]
        _write(keys, s, np.full(xs.size, k), xs.ravel(), ys.ravel())
    return keys


def oriented_ids(cam, vertices, triangles, ids):
    """the vertex ids (a, b, c) of triangles `ids` as the setup orients them in this view: b and c exchanged where A2 < 0"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)[ids]
    ok, u, v, _ = coverage_ref.project(cam, np.asarray(vertices, np.float32).reshape(-1, 3))
    with np.errstate(all="ignore"):
        X = np.where(ok, np.rint(u * f32(256)), 0).astype(np.int64)
        Y = np.where(ok, np.rint(v * f32(256)), 0).astype(np.int64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    a2 = edge(X[a], Y[a], X[b], Y[b], X[c], Y[c])
    return a, np.where(a2 < 0, c, b), np.where(a2 < 0, b, c)


def flip180(image):
    """pixel (x, y) -> (w - 1 - x, h - 1 - y); image: (h, w, ...)"""
    return image[::-1, ::-1].copy()


def render(cam, vertices, triangles, colors, w, h, flip=False, interpolate="perspective"):
    """one view -> (rgba (h, w, 4) uint8, depth (h, w) float32 with 0 = empty, triangle id (h, w) uint32 with NO_TRIANGLE = empty):
    what prv_mesh_render writes.  Only the image is turned by `flip`.  interpolate="screen" weights the colours by w_k / A2
    instead (affine in the image: NOT the contract, the comparison of the host test)"""
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    s = raster_ref.Setup(cam, vertices, triangles, w, h)
    keys = visibility_keys(cam, vertices, triangles, w, h, setup=s)
    high = (keys >> np.uint64(32)).astype(np.uint32)
    covered = high != np.uint32(NO_TRIANGLE)
    depth = np.where(covered, high, np.uint32(0)).view(np.float32)
    tri_id = np.where(covered, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.uint32(NO_TRIANGLE))
    rgba = np.empty((h, w, 4), np.uint8)
    rgba[...] = BACKGROUND
    if covered.any():
        y, x = np.nonzero(covered)
        row = np.full(len(np.asarray(triangles).reshape(-1, 3)), -1, np.int64)
        row[s.ids] = np.arange(len(s.ids))
        sel = row[tri_id[y, x].astype(np.int64)]
        assert (sel >= 0).all()
        wa, wb, wc = _weights(s, sel, x, y)
        if interpolate == "perspective":
            pa, pb, pc, iz = _products(s, sel, wa, wb, wc)
        else:
            pa, pb, pc, iz = wa.astype(np.float64), wb.astype(np.float64), wc.astype(np.float64), s.a2[sel].astype(np.float64)
        a, b, c = oriented_ids(cam, vertices, triangles, s.ids)
        Ca, Cb, Cc = (colors[v[sel]].astype(np.float64) for v in (a, b, c))
        out = np.empty((len(sel), 4), np.uint8)
        for k in range(3):
            ck = ((pa * Ca[:, k] + pb * Cb[:, k]) + pc * Cc[:, k]) / iz
            out[:, k] = np.minimum(255.0, np.floor(ck + 0.5)).astype(np.uint8)
        out[:, 3] = np.where((out[:, :3] == 255).all(axis=1), 0, 255)  # convertToAlpha: exactly white is transparent
        rgba[y, x] = out
    return (flip180(rgba) if flip else rgba), depth, tri_id


def render_views(cams, vertices, triangles, colors, w, h, flip=False):
    """-> (rgba (n, h, w, 4), depth (n, h, w), triangle id (n, h, w))"""
    out = [render(c, vertices, triangles, colors, w, h, flip) for c in cams]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))
