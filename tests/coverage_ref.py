"""CPU reference of the surface coverage stage (test infrastructure, in the spirit of tests/select_ref.py).

Restates the contract of prv_coverage_create / _curve / _greedy (include/prv.h) in numpy float32, operation by operation: the
projection, the depth buffers, the visibility bits, the coverage curve and the greedy rounds in exact integers.  fmaf and f32
are tests/march_ref.py's (a float64 product and sum, rounded to float32); nothing here is shared with prv_coverage.hip.
"""
import numpy as np

from tests.march_ref import f32, fmaf

NEVER = 0xFFFFFFFF


class Cam:
    """an engine-frame camera at an image size: c2w (3, 4) float32, fx, fy, cx, cy float32, lens (4,) float32 or None"""

    def __init__(self, c2w, fx, fy, cx, cy, lens=None):
        self.c2w = np.ascontiguousarray(c2w, np.float32).reshape(3, 4)
        self.fx, self.fy, self.cx, self.cy = f32(fx), f32(fy), f32(cx), f32(cy)
        self.lens = None if lens is None or not np.any(np.asarray(lens, np.float32) != 0) else np.asarray(lens, np.float32)


def cam_at(camset, view, w, h, dataset=False):
    """camera `view` of an api.CamSet at w x h, as the library rescales it: fov-at-centre sets put the principal point at the
    image centre and scale both focal lengths by w / width; dataset sets scale per axis and keep their principal point"""
    c2w, intr = camset.get(int(view))
    cw, ch = camset.size
    s = f32(f32(w) / f32(cw))
    if dataset:
        sy = f32(f32(h) / f32(ch))
        return Cam(c2w, f32(intr[0] * s), f32(intr[1] * sy), f32(intr[2] * s), f32(intr[3] * sy), camset.lens(int(view)))
    return Cam(c2w, f32(intr[0] * s), f32(intr[1] * s), f32(f32(0.5) * f32(w)), f32(f32(0.5) * f32(h)), camset.lens(int(view)))


def _lens(L, x, y):
    """lens_eval's distorted point, in the ray generator's order of operations"""
    k1, k2, p1, p2 = (f32(v) for v in L)
    r2 = fmaf(x, x, y * y)  # (x, y: float32 arrays, so every array operation here is one float32 rounding)
    radial = fmaf(fmaf(k2, r2, k1), r2, f32(1))
    xy = x * y
    fx = fmaf(x, radial, fmaf(f32(f32(2) * p1), xy, p2 * fmaf(f32(2) * x, x, r2)))
    fy = fmaf(y, radial, fmaf(p1, fmaf(f32(2) * y, y, r2), f32(f32(2) * p2) * xy))
    return fx, fy


def project(cam, e):
    """e: (n, 3) float32 engine-frame points -> (ok (n,) bool, u, v, z (n,) float32)"""
    e = np.asarray(e, np.float32).reshape(-1, 3)
    n = len(e)
    if n < 2:  # march_ref.fmaf / f32 turn a one-element array into a scalar: two padding points, cut off again below
        e = np.concatenate([e, np.zeros((2, 3), np.float32)])
    M = cam.c2w
    with np.errstate(all="ignore"):
        d = [e[:, a] - M[a, 3] for a in range(3)]  # float32 arrays: every array operation is one float32 rounding
        c = [fmaf(M[0, a], d[0], fmaf(M[1, a], d[1], M[2, a] * d[2])) for a in range(3)]
        ok = (c[2] > f32(1e-6)) & (c[2] < f32(np.inf))
        x, y = c[0] / c[2], c[1] / c[2]
        if cam.lens is not None:
            x, y = _lens(cam.lens, x, y)
        u, v = fmaf(cam.fx, x, cam.cx), fmaf(cam.fy, y, cam.cy)
    return ok[:n], u[:n], v[:n], c[2][:n]


def depth_buffer(cam, e, w, h, point_size):
    """stage A -> (h, w) float32: the nearest depth of the points whose block covers the pixel, 0 where none does"""
    ok, u, v, z = project(cam, e)
    ps = f32(point_size)
    with np.errstate(all="ignore"):
        fx0 = np.floor((u - f32(f32(0.5) * ps)) + f32(0.5))
        fy0 = np.floor((v - f32(f32(0.5) * ps)) + f32(0.5))
        ok = ok & (fx0 > -ps) & (fx0 < f32(w)) & (fy0 > -ps) & (fy0 < f32(h))  # a NaN fails
    keys = np.full((h, w), NEVER, np.uint32)
    if ok.any():
        x0, y0 = fx0[ok].astype(np.int64), fy0[ok].astype(np.int64)
        zb = z[ok].view(np.uint32)
        for j in range(point_size):
            for i in range(point_size):
                x, y = x0 + i, y0 + j
                inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
                np.minimum.at(keys, (y[inside], x[inside]), zb[inside])
    return np.where(keys == NEVER, np.uint32(0), keys).view(np.float32)


def visible(cam, e, w, h, point_size, depth_tol):
    """stages A and B of one view -> (visible (n,) bool, depth (h, w) float32)"""
    depth = depth_buffer(cam, e, w, h, point_size)
    ok, u, v, z = project(cam, e)
    tol1 = f32(f32(1) + f32(depth_tol))
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u), np.floor(v)
        ok = ok & (fu >= 0) & (fu < f32(w)) & (fv >= 0) & (fv < f32(h))
    vis = np.zeros(len(z), bool)
    if ok.any():
        zmin = depth[fv[ok].astype(np.int64), fu[ok].astype(np.int64)]
        zmin = np.where(zmin == 0, f32(np.nan), zmin)  # an empty pixel fails
        with np.errstate(all="ignore"):
            vis[ok] = z[ok] <= zmin * tol1  # float32 * float32: one rounding
    return vis, depth


def matrix(cams, e, w, h, point_size=1, depth_tol=0.02):
    """-> (vis (n_views, n) bool, depth (n_views, h, w) float32)"""
    out = [visible(c, e, w, h, point_size, depth_tol) for c in cams]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def pack(vis):
    """(n,) bool -> uint64 words, bit j of word w = point 64 w + j"""
    vis = np.asarray(vis, bool)
    padded = np.zeros((len(vis) + 63) // 64 * 64, np.uint8)
    padded[: len(vis)] = vis
    return np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1, 8).copy().view("<u8").ravel()


def curve(vis, order):
    """-> (covered [k] cumulative ints, first_seen (n,) uint32)"""
    vis = np.asarray(vis, bool)
    seen = np.zeros(vis.shape[1], bool)
    first = np.full(vis.shape[1], NEVER, np.uint32)
    covered = []
    for j, v in enumerate(order):
        fresh = vis[v] & ~seen
        first[fresh] = j
        seen |= vis[v]
        covered.append(int(seen.sum()))
    return covered, first


def greedy(vis, k):
    """-> (chosen positions [k], covered [k] cumulative ints); ties: the smallest position; a gain of 0 is taken like any other"""
    vis = np.asarray(vis, bool)
    seen = np.zeros(vis.shape[1], bool)
    left = list(range(len(vis)))
    chosen, covered = [], []
    for _ in range(k):
        best, best_gain = None, -1
        for i in left:
            gain = int((vis[i] & ~seen).sum())
            if gain > best_gain:
                best, best_gain = i, gain
        chosen.append(best)
        left.remove(best)
        seen |= vis[best]
        covered.append(int(seen.sum()))
    return chosen, covered
