"""CPU reference of the view selection stage (test infrastructure, in the spirit of tests/depth_ref.py).

Restates the contract of prv_select_from_images (include/prv.h) in numpy float32, operation by operation: the gain word, the
point a pixel's expected depth names, its voxel, and the greedy rounds in exact integers.  Rays come from
Context.debug_raygen, the forward cosine from march_ref.forward_cos, whose FMAs are march_ref.fmaf; nothing here is shared
with prv_select.hip.
"""
import numpy as np

from tests import march_ref

f32 = np.float32
UNLOCATED = 0xFFFFFFFF
Q_CAP = f32(4294967040.0)  # the largest float32 below 2^32


class _Cam:
    """what march_ref.forward_cos reads of a camera: c2w, 12 float32, row-major 3x4"""

    def __init__(self, c2w):
        self.c2w = np.ascontiguousarray(c2w, np.float32).reshape(12)


def gain_words(H):
    """q = H > 0 ? (uint32) min(floorf(H * 65536), 4294967040) : 0; NaN and negative H give 0"""
    H = np.asarray(H, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.minimum(np.floor(H * f32(65536.0)), Q_CAP)
        v = np.where(H > 0, v, f32(0))
    return v.astype(np.float64).astype(np.uint64).astype(np.uint32)


def voxels_from_rays(o, d, cos, alpha, z, G, alpha_min):
    """o, d: (n, 3) float32 rays; cos: (n,) forward cosines; alpha, z: (n,) -> (n,) uint32 voxel words"""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    alpha, z, cos = np.asarray(alpha, np.float32).ravel(), np.asarray(z, np.float32).ravel(), np.asarray(cos, np.float32).ravel()
    fG = f32(G)
    with np.errstate(all="ignore"):
        located = (alpha >= f32(alpha_min)) & (z > 0)
        t = ((z / alpha).astype(np.float32) / cos).astype(np.float32)
        g = np.zeros((len(t), 3), np.float32)
        for a in range(3):
            prod = (t * d[:, a]).astype(np.float32)  # a multiply, then an add: no FMA
            p = (o[:, a] + prod).astype(np.float32)
            g[:, a] = np.floor((p * fG).astype(np.float32))
        inside = ((g >= 0) & (g < fG)).all(axis=1)  # a NaN fails both
    ok = located & inside
    gi = np.where(ok[:, None], g, 0).astype(np.int64)
    vox = gi[:, 0] + G * (gi[:, 1] + G * gi[:, 2])
    return np.where(ok, vox, UNLOCATED).astype(np.uint32)


def footprint(ctx, camset, view, w, h, H, alpha, z, G, alpha_min):
    """(h, w) planes of one view -> (voxel, q), (h, w) uint32 each"""
    o, d, _ = ctx.debug_raygen(camset, int(view), w, h, 0)
    c2w, _ = camset.get(int(view))
    cos = march_ref.forward_cos(_Cam(c2w), d.T)
    vox = voxels_from_rays(o, d, cos, np.asarray(alpha).ravel(), np.asarray(z).ravel(), G, alpha_min)
    return vox.reshape(h, w), gain_words(H).reshape(h, w)


def greedy(voxel, q, k, G):
    """voxel, q: (n_views, ...) uint32 -> (chosen positions [k], gains [k]) in exact integers; ties: the first view"""
    voxel = np.asarray(voxel, np.uint32).reshape(len(voxel), -1)
    q = np.asarray(q, np.uint32).reshape(len(q), -1)
    covered = np.zeros(G ** 3, bool)
    left = list(range(len(voxel)))
    chosen, gains = [], []
    for _ in range(k):
        best, best_gain = None, -1
        for i in left:
            loc = voxel[i] != UNLOCATED
            fresh = ~loc
            fresh[loc] = ~covered[voxel[i][loc]]
            gain = int(q[i][fresh].astype(np.uint64).sum(dtype=np.uint64))
            if gain > best_gain:
                best, best_gain = i, gain
        chosen.append(best)
        gains.append(best_gain)
        left.remove(best)
        loc = voxel[best] != UNLOCATED
        covered[voxel[best][loc]] = True
    return chosen, gains


def unlocated_sum(voxel, q):
    voxel, q = np.asarray(voxel, np.uint32).ravel(), np.asarray(q, np.uint32).ravel()
    return int(q[voxel == UNLOCATED].astype(np.uint64).sum(dtype=np.uint64))
