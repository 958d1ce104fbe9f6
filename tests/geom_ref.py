"""numpy restatement of the three contracts of the geometric evaluation (include/prv.h): the area-weighted mesh sampler,
the nearest-neighbour arithmetic and the distance metrics.  Checker only: nothing under nerf_prv_amd/ imports it."""
import numpy as np

M64 = (1 << 64) - 1
AREA_SCALE = float(1 << 40)
STREAM_STRATUM, STREAM_BARY = 0x5A0, 0x5A2


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rng_u24(seed, stream, i):
    """the project's counter RNG: 24 bits keyed by (seed, stream, i)"""
    return mix64((seed + (stream + 1) * 0xD1B54A32D192ED03 + i * 0x9E3779B97F4A7C15) & M64) >> 40


def rng_u24_array(seed, stream, n):
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + np.uint64(((stream + 1) * 0xD1B54A32D192ED03) & M64) + i * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return (z ^ (z >> np.uint64(31))) >> np.uint64(40)


def triangle_weights(vertices, triangles):
    """floor(area * 2^40) as Python ints; area in fp64 from the fp32 vertices, 0 for anything without positive finite area"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        w = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz) * AREA_SCALE
    return [int(x) if (x >= 1.0 and x < 2.0 ** 62) else 0 for x in w]


def sample_mesh(vertices, triangles, n, seed):
    """-> (xyz float32 (n, 3), triangle ids int64 (n,)): prv_mesh_sample's rule, exact integers for the choice and float32
    operation by operation for the position"""
    v = np.asarray(vertices, np.float32)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    w = triangle_weights(v, t)
    scan = [0] * len(w)
    run = 0
    for i, x in enumerate(w):
        scan[i] = run
        run += x
    W = run
    if W == 0 or n == 0:
        raise ValueError("nothing to sample")
    r0 = rng_u24_array(seed, STREAM_STRATUM, n)
    r1 = rng_u24_array(seed, STREAM_STRATUM + 1, n)
    targets = np.empty(n, dtype=object)
    for k in range(n):
        lo, hi = k * W // n, (k + 1) * W // n
        u48 = (int(r0[k]) << 24) | int(r1[k])
        targets[k] = lo + (((hi - lo) * u48) >> 48)
    if W < 2 ** 63:
        tri = np.searchsorted(np.array(scan, np.uint64), np.array([int(x) for x in targets], np.uint64), side="right") - 1
    else:
        import bisect

        tri = np.array([bisect.bisect_right(scan, x) - 1 for x in targets])
    tri = tri.astype(np.int64)
    u = rng_u24_array(seed, STREAM_BARY, n).astype(np.float32) * np.float32(1.0 / 16777216.0)
    w2 = rng_u24_array(seed, STREAM_BARY + 1, n).astype(np.float32) * np.float32(1.0 / 16777216.0)
    fold = (u + w2) > np.float32(1.0)
    u = np.where(fold, np.float32(1.0) - u, u).astype(np.float32)
    w2 = np.where(fold, np.float32(1.0) - w2, w2).astype(np.float32)
    a, b, c = v[t[tri, 0]], v[t[tri, 1]], v[t[tri, 2]]
    e1, e2 = (b - a).astype(np.float32), (c - a).astype(np.float32)
    xyz = ((a + u[:, None] * e1).astype(np.float32) + (w2[:, None] * e2).astype(np.float32)).astype(np.float32)
    return xyz, tri


def nearest(queries, reference, chunk=256):
    """brute force in float32: d2 = (dx*dx + dy*dy) + dz*dz, the minimum over all reference points, ties to the smallest id
    -> (d2 float32 (m,), ids int64 (m,))"""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    p = np.ascontiguousarray(reference, np.float32).reshape(-1, 3)
    d2 = np.empty(len(q), np.float32)
    ids = np.empty(len(q), np.int64)
    with np.errstate(over="ignore"):
        for s in range(0, len(q), chunk):
            c = q[s:s + chunk]
            dx = c[:, None, 0] - p[None, :, 0]
            dy = c[:, None, 1] - p[None, :, 1]
            dz = c[:, None, 2] - p[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            k = np.argmin(d, axis=1)  # the first minimum: the smallest id
            ids[s:s + chunk] = k
            d2[s:s + chunk] = d[np.arange(len(c)), k]
    return d2, ids


FIELDS = ("n_rec", "n_ref", "accuracy", "completeness", "accuracy_sq", "completeness_sq", "chamfer", "precision", "recall", "fscore",
          "hausdorff_rec", "hausdorff_ref")


def metrics_from_d2(d2_rec, d2_ref, tau):
    """prv_geom_metrics from the two directions' squared distances (float32): dist = float32 sqrt, sums in float64"""
    out = {"n_rec": len(d2_rec), "n_ref": len(d2_ref)}
    within = []
    for name, sq, side, d2 in (("accuracy", "accuracy_sq", "rec", d2_rec), ("completeness", "completeness_sq", "ref", d2_ref)):
        d2 = np.asarray(d2, np.float32)
        d = np.sqrt(d2)
        assert d.dtype == np.float32
        out[name] = float(np.sum(d.astype(np.float64)) / len(d))
        out[sq] = float(np.sum(d2.astype(np.float64)) / len(d))
        out["hausdorff_" + side] = float(d.max())
        within.append(int(np.count_nonzero(d <= np.float32(tau))))
    out["chamfer"] = (out["accuracy"] + out["completeness"]) / 2.0
    out["precision"], out["recall"] = within[0] / len(d2_rec), within[1] / len(d2_ref)
    pr = out["precision"] + out["recall"]
    out["fscore"] = 2.0 * out["precision"] * out["recall"] / pr if pr > 0 else 0.0
    out["within_rec"], out["within_ref"] = within
    return out


def metrics(rec, ref, tau):
    return metrics_from_d2(nearest(rec, ref)[0], nearest(ref, rec)[0], tau)


def sphere_points(n, radius, centre=(0.5, 0.5, 0.5), seed=0):
    """n points placed analytically on a sphere (a Fibonacci spiral: near-uniform, deterministic)"""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0))) + seed
    s = np.sqrt(1.0 - z * z)
    return (np.asarray(centre) + radius * np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)).astype(np.float32)
