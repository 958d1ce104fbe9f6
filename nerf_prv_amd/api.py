"""Python host side of the render + view-scoring path, over the C ABI (include/prv.h).

Two layers:
  * `Context` / `CamSet`: thin object wrappers of the C entry points.  Device buffers are
    torch tensors (torch is only plumbing here: memory, streams, torch.distributed).
  * `Testbed`: mirrors the slice of `pyngp.Testbed` that the reference's
    Instantngp_scripts/run.py drives on this path (run.py:90-145, 226-247, 284-309):
    same attribute names and argument meaning, so a screenshot loop written against the
    reference reads the same here.

No CPU fallback: every call goes to libprv_hip.so; errors raise `PrvError`.
"""
import ctypes as C
import enum
import json
import math

import numpy as np

from . import _lib as L

RECORD_DTYPE = np.dtype([("score", "<f8"), ("psnr", "<f4"), ("coverage", "<f4")])

# the two synthetic fields BASELINE.md names
FIELD_256 = dict(n_levels=8, n_features=4, log2_hashmap=19, base_res=16, finest_res=256, occ_res=128,
                 density_bias=3.0, table_amp=4.0)
FIELD_512 = dict(n_levels=16, n_features=2, log2_hashmap=21, base_res=16, finest_res=512, occ_res=128,
                 density_bias=3.0, table_amp=4.0)
# a table that really leaves the caches (round 6): log2T = 24 at F = 2 -- seven hashed levels of 64 MiB each (448 MiB of random
# 4-byte gathers against a 256 MiB Infinity Cache) behind nine dense ones; levels beyond 16 MiB take the generic gather's 32-bit
# offsets (prv_field_plan.hpp: plan_field, FieldDev::wide_offsets)
FIELD_HBM = dict(n_levels=16, n_features=2, log2_hashmap=24, base_res=16, finest_res=2048, occ_res=128,
                 density_bias=3.0, table_amp=4.0)


def replica_level(res, n_features=4):
    """(entries per row, z stride in bytes, bytes) of the dense replica of a hashed level of `res` vertices per axis
    (prv_debug_replica_level; needs no GPU)"""
    row, mz, b = C.c_uint32(), C.c_uint64(), C.c_uint64()
    if L.load().prv_debug_replica_level(int(res), int(n_features), C.byref(row), C.byref(mz), C.byref(b)) != 0:
        raise PrvError(L.PRV_E_INVALID, "prv_debug_replica_level failed")
    return row.value, mz.value, b.value


def replica_layout(ctx, model_slot):
    """(levels, bytes) of the dense replicas the field in a slot of Context `ctx` holds of its leading hashed levels: the replica
    variant its render launches, 0 = the plain instance (prv_debug_replica_layout; the tests' hook, like Context.model_layout,
    whose answer does not change with replicas)"""
    n, b = C.c_int32(), C.c_uint64()
    ctx._chk(ctx.lib.prv_debug_replica_layout(ctx.handle, int(model_slot), C.byref(n), C.byref(b)))
    return n.value, b.value


class RenderMode(enum.IntEnum):
    """testbed.render_mode (run.py:287: `testbed.render_mode = ngp.Depth` for --screenshot_depth)"""

    Shade = 0
    Depth = 1


Shade, Depth = RenderMode.Shade, RenderMode.Depth  # as pyngp exports them (ngp.Depth)


class PrvError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"prv error {code}: {msg}")
        self.code = code


def field_desc(**kw):
    d = dict(FIELD_256)
    d.update(kw)
    return L.FieldDesc(**d)


def render_opts(width, height, samples_per_ray=128, spp=1, min_transmittance=1e-4, background=(0.0, 0.0, 0.0, 0.0),
                step_mode=L.STEP_FIXED_S):
    o = L.RenderOpts()
    o.width, o.height, o.samples_per_ray, o.spp = int(width), int(height), int(samples_per_ray), int(spp)
    o.step_mode = int(step_mode)
    o.min_transmittance = float(min_transmittance)
    for k in range(4):
        o.background[k] = float(background[k])
    return o


def engine_render_opts(width, height, samples_per_ray, spp, min_transmittance, background=(0.0, 0.0, 0.0, 0.0)):
    """render options as the run.py mirrors (Testbed, the flag-file server) state them: samples_per_ray 0 = the engine's
    own stepping rule (PRV_STEP_NGP: dt = sqrt(3)/1024, what pyngp renders with behind run.py:304), N > 0 = N uniform
    samples per ray (PRV_STEP_FIXED_S, the BASELINE configs' rule)"""
    n = int(samples_per_ray)
    return render_opts(width, height, n, spp, min_transmittance, background, step_mode=L.STEP_NGP if n == 0 else L.STEP_FIXED_S)


def select_opts(k=None, grid_res=None, alpha_min=None):
    """prv_select_opts: the library's defaults (k 1, grid_res 64, alpha_min 0.5) with the given fields replaced"""
    o = L.SelectOpts()
    if L.load().prv_select_default_opts(C.byref(o)) != 0:
        raise PrvError(L.PRV_E_INVALID, "prv_select_default_opts failed")
    if k is not None:
        o.k = int(k)
    if grid_res is not None:
        o.grid_res = int(grid_res)
    if alpha_min is not None:
        o.alpha_min = float(alpha_min)
    return o


def model_sizes(desc):
    lib = L.load()
    t, m, o = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = lib.prv_model_sizes(C.byref(desc), C.byref(t), C.byref(m), C.byref(o))
    if rc != 0:
        raise PrvError(rc, "invalid field descriptor")
    return t.value, m.value, o.value


def _ptr(a):
    """device or host pointer of a torch tensor / numpy array / None"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(a.data_ptr())


class _Handle:
    """what the library's objects share on this side: the context, the C handle, the call that destroys it, the error lookup"""
    _destroy = None  # the C function that destroys the handle

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def _chk(self, rc):
        """a failed call's error: the message is the context's, or the thread's if the handle or its context is gone (or the
        context has none)"""
        if rc != 0:
            lib = self.ctx.lib
            msg = (lib.prv_last_error(self.ctx.handle) if self.ctx.handle else None) or b""
            if not (self.handle and msg) or rc == L.PRV_E_STATE:
                msg = lib.prv_last_error(None) or msg
            raise PrvError(rc, msg.decode())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if getattr(self, "handle", None):
            getattr(self.ctx.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CamSet(_Handle):
    _destroy = "prv_camset_destroy"

    def __len__(self):
        return self.ctx.lib.prv_camset_count(self.handle)

    @property
    def size(self):
        w, h = C.c_int(), C.c_int()
        self.ctx.lib.prv_camset_size(self.handle, C.byref(w), C.byref(h))
        return w.value, h.value

    def get(self, i):
        c2w = np.zeros(12, np.float32)
        intr = np.zeros(4, np.float32)
        rc = self.ctx.lib.prv_camset_get(self.handle, i, _ptr(c2w), _ptr(intr))
        if rc != 0:
            raise PrvError(rc, "camera index out of range")
        return c2w.reshape(3, 4), intr

    def lens(self, i):
        """{k1, k2, p1, p2} of camera i"""
        lens = np.zeros(4, np.float32)
        if self.ctx.lib.prv_camset_lens(self.handle, i, _ptr(lens)) != 0:
            raise PrvError(L.PRV_E_INVALID, "camera index out of range")
        return lens


class Context:
    """One context per process per GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device=0, use_torch_stream=True):
        import torch

        self.torch = torch
        self.lib = L.load()
        h = C.c_void_p()
        rc = self.lib.prv_create(C.byref(h), int(device))
        if rc != 0:
            raise PrvError(rc, (self.lib.prv_last_error(None) or b"").decode())
        self.handle = h
        self.device = torch.device("cuda", int(device))
        if use_torch_stream:
            with torch.cuda.device(self.device):
                self.set_stream(torch.cuda.current_stream().cuda_stream)

    # -- plumbing
    def _chk(self, rc):
        if rc != 0:
            raise PrvError(rc, (self.lib.prv_last_error(self.handle) or b"").decode())

    def set_stream(self, raw_stream):
        self._chk(self.lib.prv_set_stream(self.handle, C.c_void_p(raw_stream)))

    def synchronize(self):
        self._chk(self.lib.prv_synchronize(self.handle))

    def set_coverage_weight(self, weight):
        """SCORE_PSNR_COVERAGE's key = -PSNR + weight * mean((1 - alpha)^2); default 1, 0 = PSNR alone"""
        self._chk(self.lib.prv_set_coverage_weight(self.handle, float(weight)))

    def profile_begin(self):
        self._chk(self.lib.prv_profile_begin(self.handle))

    def profile_end(self):
        """-> dict(render_ms, render_launches, march_ms, march_launches) from HIP events"""
        rm, mm, rn, mn = C.c_double(), C.c_double(), C.c_int(), C.c_int()
        self._chk(self.lib.prv_profile_end(self.handle, C.byref(rm), C.byref(rn), C.byref(mm), C.byref(mn)))
        each = (C.c_float * max(1, rn.value))()
        n = self.lib.prv_profile_render_launches(self.handle, each, rn.value)
        return dict(render_ms=rm.value, render_launches=rn.value, march_ms=mm.value, march_launches=mn.value,
                    render_launch_ms=[float(each[i]) for i in range(max(0, min(n, rn.value)))])

    def close(self):
        if getattr(self, "handle", None):
            self.lib.prv_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- model
    def load_model(self, slot, desc, table, mlp, occ):
        table = np.ascontiguousarray(table, np.uint16)
        mlp = np.ascontiguousarray(mlp, np.uint16)
        occ = np.ascontiguousarray(occ, np.uint32)
        t, m, o = model_sizes(desc)
        if table.size != t or mlp.size != m or occ.size != o:
            raise PrvError(L.PRV_E_INVALID, f"parameter sizes {table.size},{mlp.size},{occ.size} != {t},{m},{o}")
        self._chk(self.lib.prv_model_load(self.handle, slot, C.byref(desc), _ptr(table), _ptr(mlp), _ptr(occ)))

    def synthetic_model(self, slot, desc, seed):
        self._chk(self.lib.prv_model_synthetic(self.handle, slot, C.byref(desc), C.c_uint64(seed)))

    def fresh_model(self, slot, desc, seed):
        """training start: small random table, Xavier MLP, all cells occupied"""
        self._chk(self.lib.prv_model_fresh(self.handle, slot, C.byref(desc), C.c_uint64(seed)))

    def export_model(self, slot, desc):
        t, m, o = model_sizes(desc)
        table, mlp, occ = np.empty(t, np.uint16), np.empty(m, np.uint16), np.empty(o, np.uint32)
        self._chk(self.lib.prv_model_export(self.handle, slot, _ptr(table), _ptr(mlp), _ptr(occ)))
        return table, mlp, occ

    def save_model(self, slot, path):
        self._chk(self.lib.prv_model_save_file(self.handle, slot, str(path).encode()))

    def load_model_file(self, slot, path):
        self._chk(self.lib.prv_model_load_file(self.handle, slot, str(path).encode()))

    def load_ingp(self, slot, path):
        """an instant-ngp snapshot (.ingp / .msgpack) -> slot; returns its FieldDesc"""
        self._chk(self.lib.prv_model_load_ingp(self.handle, slot, str(path).encode()))
        return self.model_desc(slot)

    def save_ingp(self, slot, path):
        self._chk(self.lib.prv_model_save_ingp(self.handle, slot, str(path).encode()))

    def model_desc(self, slot):
        d = L.FieldDesc()
        self._chk(self.lib.prv_model_desc(self.handle, slot, C.byref(d)))
        return d

    # -- cameras
    def cameras_from_json(self, path):
        h = C.c_void_p()
        self._chk(self.lib.prv_cameras_from_json(self.handle, str(path).encode(), C.byref(h)))
        return CamSet(self, h)

    def cameras_from_dataset_json(self, path):
        """the json's own intrinsics block (fl, principal point, lens): the engine's view of a dataset"""
        h = C.c_void_p()
        self._chk(self.lib.prv_cameras_from_dataset_json(self.handle, str(path).encode(), C.byref(h)))
        return CamSet(self, h)

    def cameras_from_matrices_intr(self, tm, intr, scale, offset):
        """intr: dict with fl_x fl_y cx cy w h and optional k1 k2 p1 p2"""
        tm = np.ascontiguousarray(tm, np.float64).reshape(-1, 16)
        off = np.ascontiguousarray(offset, np.float64)
        ci = L.Intrinsics(**{k: (int(v) if k in ("w", "h") else float(v)) for k, v in intr.items()})
        h = C.c_void_p()
        self._chk(self.lib.prv_cameras_from_matrices_intr(self.handle, _ptr(tm), tm.shape[0], C.byref(ci), float(scale),
                                                          _ptr(off), C.byref(h)))
        return CamSet(self, h)

    def cameras_from_matrices(self, tm, camera_angle_x, width, height, scale, offset):
        tm = np.ascontiguousarray(tm, np.float64).reshape(-1, 16)
        off = np.ascontiguousarray(offset, np.float64)
        h = C.c_void_p()
        self._chk(self.lib.prv_cameras_from_matrices(self.handle, _ptr(tm), tm.shape[0], float(camera_angle_x),
                                                     int(width), int(height), float(scale), _ptr(off), C.byref(h)))
        return CamSet(self, h)

    def splat_points(self, xyz, rgb, scale, offset, camset, view_ids, width, height, point_size=5, flip180=True):
        """ground-truth images of a coloured cloud (get_coverage's rgbaClip images) -> uint8 [n, h, w, 4] on the device"""
        t = self.torch
        xyz = t.as_tensor(np.ascontiguousarray(xyz, np.float32)).to(self.device).contiguous().reshape(-1, 3)
        rgb = t.as_tensor(np.ascontiguousarray(rgb, np.uint8)).to(self.device).contiguous().reshape(-1, 3)
        ids = self._ids(camset, view_ids)
        off = np.ascontiguousarray(offset, np.float64)
        out = t.empty((len(ids), height, width, 4), dtype=t.uint8, device=self.device)
        self._chk(self.lib.prv_splat_points(self.handle, _ptr(xyz), _ptr(rgb), xyz.shape[0], float(scale), _ptr(off),
                                            camset.handle, _ptr(ids), len(ids), int(width), int(height), int(point_size),
                                            int(flip180), _ptr(out)))
        return out

    # -- render
    def _ids(self, camset, view_ids):
        if view_ids is None:
            view_ids = np.arange(len(camset), dtype=np.int32)
        return np.ascontiguousarray(view_ids, np.int32)

    def render(self, slot, camset, view_ids, opts, out=None, want_stats=True):
        ids = self._ids(camset, view_ids)
        if out is None:
            out = self.torch.empty((len(ids), opts.height, opts.width, 4), dtype=self.torch.float32, device=self.device)
        st = L.Stats()
        self._chk(self.lib.prv_render(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(opts), _ptr(out),
                                      C.byref(st) if want_stats else None))
        return out, st

    def render_rgba8(self, slot, camset, view_ids, opts, out=None, want_stats=True):
        ids = self._ids(camset, view_ids)
        if out is None:
            out = self.torch.empty((len(ids), opts.height, opts.width, 4), dtype=self.torch.uint8, device=self.device)
        st = L.Stats()
        self._chk(self.lib.prv_render_rgba8(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(opts),
                                            _ptr(out), C.byref(st) if want_stats else None))
        return out, st

    def render_depth(self, slot, camset, view_ids, opts, out=None, out_depth=None, want_stats=True):
        """prv_render_depth -> (rgba [n, h, w, 4] as `render`, depth [n, h, w] float32, stats).  depth: z-depth along each
        view's optical axis in engine units, premultiplied by opacity like the colour (include/prv.h)"""
        ids = self._ids(camset, view_ids)
        if out is None:
            out = self.torch.empty((len(ids), opts.height, opts.width, 4), dtype=self.torch.float32, device=self.device)
        if out_depth is None:
            out_depth = self.torch.empty((len(ids), opts.height, opts.width), dtype=self.torch.float32, device=self.device)
        st = L.Stats()
        self._chk(self.lib.prv_render_depth(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(opts), _ptr(out),
                                            _ptr(out_depth), C.byref(st) if want_stats else None))
        return out, out_depth, st

    def render_entropy(self, slot, camset, view_ids, opts, out=None, out_alpha=None, want_stats=True):
        """prv_render_entropy -> (entropy [n, h, w] float32 in bits, alpha [n, h, w] float32, stats).  entropy: per ray the
        entropy of its compositing weights and the escape term (include/prv.h); alpha: `render`'s alpha channel, bit for
        bit.  One model, no reference image, no colour evaluated."""
        ids = self._ids(camset, view_ids)
        if out is None:
            out = self.torch.empty((len(ids), opts.height, opts.width), dtype=self.torch.float32, device=self.device)
        if out_alpha is None:
            out_alpha = self.torch.empty((len(ids), opts.height, opts.width), dtype=self.torch.float32, device=self.device)
        st = L.Stats()
        self._chk(self.lib.prv_render_entropy(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(opts), _ptr(out),
                                              _ptr(out_alpha), C.byref(st) if want_stats else None))
        return out, out_alpha, st

    def render_termination(self, slot, camset, view_ids, opts, n_bins=L.TERMINATION_BINS_DEFAULT, want_stats=True):
        """prv_render_termination -> (bins [n_bins, n, h, w] float32, alpha [n, h, w] float32, stats).  bins[k]: the ray's
        compositing weights that fall in depth bin k of its unit-cube span (bin positions do not depend on the field, so
        different models' histograms line up); alpha: `render_entropy`'s, bit for bit.  No colour evaluated."""
        ids = self._ids(camset, view_ids)
        bins = self.torch.empty((max(int(n_bins), 0), len(ids), opts.height, opts.width), dtype=self.torch.float32, device=self.device)
        alpha = self.torch.empty((len(ids), opts.height, opts.width), dtype=self.torch.float32, device=self.device)
        st = L.Stats()
        self._chk(self.lib.prv_render_termination(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(opts), int(n_bins),
                                                  _ptr(bins), _ptr(alpha), C.byref(st) if want_stats else None))
        return bins, alpha, st

    def termination_divergence(self, bins, alphas, want_image=True):
        """prv_termination_divergence on the members' device planes (bins[e]: [n_bins, n, h, w], alphas[e]: [n, h, w], as
        `render_termination` returns them) -> (jsd [n, h, w] float32 in bits or None, view mean jsd [n] float64, view mean
        opacity [n] float64)"""
        if len(bins) == 0 or len(bins) != len(alphas):
            raise ValueError("one bins tensor and one alpha plane per member, at least one member")
        n_bins, n, h, w = (int(x) for x in bins[0].shape)
        for b, a in zip(bins, alphas):
            if tuple(b.shape) != (n_bins, n, h, w) or tuple(a.shape) != (n, h, w) or not b.is_contiguous() or not a.is_contiguous():
                raise ValueError("every member needs contiguous planes of one shape: bins [n_bins, n, h, w], alpha [n, h, w]")
        barr = (C.c_void_p * len(bins))(*[b.data_ptr() for b in bins])
        aarr = (C.c_void_p * len(alphas))(*[a.data_ptr() for a in alphas])
        out = self.torch.empty((n, h, w), dtype=self.torch.float32, device=self.device) if want_image else None
        vj, vo = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self._chk(self.lib.prv_termination_divergence(self.handle, barr, aarr, len(bins), n, w, h, n_bins, _ptr(out), _ptr(vj), _ptr(vo)))
        return out, vj, vo

    def render_footprint(self, slot, camset, view_ids, opts, want_stats=True):
        """prv_render_footprint -> (entropy, alpha, depth: [n, h, w] float32 each, stats): `render_entropy`'s two planes and
        `render_depth`'s depth plane, bit for bit, from one density-only launch"""
        ids = self._ids(camset, view_ids)
        ent, alpha, depth = (self.torch.empty((len(ids), opts.height, opts.width), dtype=self.torch.float32, device=self.device)
                             for _ in range(3))
        st = L.Stats()
        self._chk(self.lib.prv_render_footprint(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(opts), _ptr(ent),
                                                _ptr(alpha), _ptr(depth), C.byref(st) if want_stats else None))
        return ent, alpha, depth, st

    def render_surface(self, slot, camset, view_ids, opts, level=0.5, want_stats=True):
        """prv_render_surface -> (entropy, alpha, depth, hit: [n, h, w] float32 each, stats): `render_entropy`'s two planes bit
        for bit; depth = the premultiplied z-depth of the first sample at which the ray's accumulated opacity reaches `level`,
        hit = the share of the pixel's sub-samples that get there (depth / hit: the mean z of those that do)"""
        ids = self._ids(camset, view_ids)
        ent, alpha, depth, hit = (self.torch.empty((len(ids), opts.height, opts.width), dtype=self.torch.float32, device=self.device)
                                  for _ in range(4))
        st = L.Stats()
        self._chk(self.lib.prv_render_surface(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(opts), float(level),
                                              _ptr(ent), _ptr(alpha), _ptr(depth), _ptr(hit), C.byref(st) if want_stats else None))
        return ent, alpha, depth, hit, st

    def select_from_images(self, camset, view_ids, entropy, alpha, depth, opts, want_words=False):
        """prv_select_from_images on device planes [n, h, w] -> (chosen view ids [k] int32, gains [k] uint64) and, with
        want_words, the per-pixel (voxel, q) words as int32-typed device tensors [n, h, w] holding uint32 bit patterns"""
        ids = self._ids(camset, view_ids)
        h, w = int(entropy.shape[1]), int(entropy.shape[2])
        k = max(int(opts.k), 0)
        chosen, gains = np.zeros(k, np.int32), np.zeros(k, np.uint64)
        voxel = q = None
        if want_words:
            voxel = self.torch.empty((len(ids), h, w), dtype=self.torch.int32, device=self.device)
            q = self.torch.empty((len(ids), h, w), dtype=self.torch.int32, device=self.device)
        self._chk(self.lib.prv_select_from_images(self.handle, camset.handle, _ptr(ids), len(ids), w, h, _ptr(entropy), _ptr(alpha),
                                                  _ptr(depth), C.byref(opts), _ptr(chosen), _ptr(gains), _ptr(voxel), _ptr(q)))
        return (chosen, gains, voxel, q) if want_words else (chosen, gains)

    def select_views(self, slot, camset, view_ids, render_opts, opts, want_stats=False, locator="expected", level=0.5):
        """prv_select_views: the footprint render of the candidates, then the greedy rounds -> (chosen [k], gains [k], stats).
        locator="surface": prv_select_views_surface -- the candidates' pixels are located at the first sample at which the
        accumulated opacity reaches `level` (`render_surface`) instead of at the expected depth"""
        if locator not in ("expected", "surface"):
            raise ValueError(f"locator must be 'expected' or 'surface', got {locator!r}")
        ids = self._ids(camset, view_ids)
        k = max(int(opts.k), 0)
        chosen, gains = np.zeros(k, np.int32), np.zeros(k, np.uint64)
        st = L.Stats()
        tail = (C.byref(opts), _ptr(chosen), _ptr(gains), C.byref(st) if want_stats else None)
        if locator == "surface":
            self._chk(self.lib.prv_select_views_surface(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(render_opts),
                                                        float(level), *tail))
        else:
            self._chk(self.lib.prv_select_views(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(render_opts), *tail))
        return chosen, gains, st

    def first_hit(self, slot, camset, view_ids, width, height, max_range=1e30):
        ids = self._ids(camset, view_ids)
        out = self.torch.empty((len(ids), height, width), dtype=self.torch.int32, device=self.device)
        self._chk(self.lib.prv_first_hit(self.handle, slot, camset.handle, _ptr(ids), len(ids), width, height,
                                         float(max_range), _ptr(out)))
        return out

    def precept(self, slot, voxels, c2w, intr, max_range=1.0):
        """Perception_3D::precept per voxel (main.cpp:98-284): voxels = device float tensor n x 3 -> int32 cells"""
        c = np.ascontiguousarray(c2w, np.float64).reshape(16)
        out = self.torch.empty((voxels.shape[0],), dtype=self.torch.int32, device=self.device)
        self._chk(self.lib.prv_precept(self.handle, slot, _ptr(voxels), voxels.shape[0], _ptr(c), C.byref(intr),
                                       float(max_range), _ptr(out)))
        return out

    def quantize_rgba8(self, rgba, background):
        out = self.torch.empty(rgba.shape, dtype=self.torch.uint8, device=self.device)
        bg = np.asarray(background, np.float32)
        self._chk(self.lib.prv_quantize_rgba8(self.handle, _ptr(rgba), rgba.numel() // 4, _ptr(bg), _ptr(out)))
        return out

    # -- scores
    def score_ensemble_images(self, method, images):
        n_views = images[0].shape[0]
        npix = images[0].numel() // 4 // max(n_views, 1)
        arr = (C.c_void_p * len(images))(*[im.data_ptr() for im in images])
        rec = np.zeros(n_views, RECORD_DTYPE)
        self._chk(self.lib.prv_score_ensemble_images(self.handle, method, arr, len(images), n_views, npix, _ptr(rec)))
        return rec

    def score_psnr_images(self, rgba, gt, background=(0, 0, 0, 0)):
        n_views = rgba.shape[0]
        npix = rgba.numel() // 4 // max(n_views, 1)
        bg = np.asarray(background, np.float32)
        rec = np.zeros(n_views, RECORD_DTYPE)
        self._chk(self.lib.prv_score_psnr_images(self.handle, _ptr(rgba), _ptr(gt), n_views, npix, _ptr(bg), _ptr(rec)))
        return rec

    def evaluate_images(self, rgba, gt, background=(0, 0, 0, 0)):
        """per-image PSNR and SSIM (run.py:257-263) -> (psnr[n], ssim[n]) float64"""
        n, h, w = rgba.shape[0], rgba.shape[1], rgba.shape[2]
        bg = np.asarray(background, np.float32)
        ps, ss = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self._chk(self.lib.prv_evaluate_images(self.handle, _ptr(rgba), _ptr(gt), n, w, h, _ptr(bg), _ptr(ps), _ptr(ss)))
        return ps, ss

    def evaluate(self, slot, camset, view_ids, opts, gt):
        """the evaluation loop of run.py:240-277 -> (mean psnr, mean ssim)"""
        ids = self._ids(camset, view_ids)
        p, s = C.c_double(), C.c_double()
        self._chk(self.lib.prv_evaluate(self.handle, slot, camset.handle, _ptr(ids), len(ids), C.byref(opts), _ptr(gt),
                                        C.byref(p), C.byref(s)))
        return p.value, s.value

    def score_views(self, method, slots, camset, view_ids, opts, gt=None, records_dev=None, to_host=True,
                    want_stats=False):
        """prv_score_views: SCORE_ENSEMBLE_RGB / _RGB_DENSITY (slots = the ensemble), SCORE_PSNR_COVERAGE (one slot, gt = the
        views' reference images), SCORE_RAY_ENTROPY (one slot, no gt: the mean of `render_entropy` per view) or
        SCORE_TERMINATION_JSD (slots = an ensemble of 2..8, no gt: the mean of `termination_divergence` per view at 16 bins)"""
        ids = self._ids(camset, view_ids)
        slots = np.ascontiguousarray(slots, np.int32)
        rec = np.zeros(len(ids), RECORD_DTYPE) if to_host else None
        st = L.Stats()
        self._chk(self.lib.prv_score_views(self.handle, method, _ptr(slots), len(slots), camset.handle, _ptr(ids),
                                           len(ids), C.byref(opts), _ptr(gt), _ptr(rec), _ptr(records_dev),
                                           C.byref(st) if want_stats else None))
        return rec, st

    def rank(self, records, view_ids):
        records = np.ascontiguousarray(records, RECORD_DTYPE)
        ids = np.ascontiguousarray(view_ids, np.int32)
        order = np.zeros(len(ids), np.int32)
        self._chk(self.lib.prv_rank(_ptr(records), _ptr(ids), len(ids), _ptr(order)))
        return order

    def argmax(self, records, view_ids):
        records = np.ascontiguousarray(records, RECORD_DTYPE)
        ids = np.ascontiguousarray(view_ids, np.int32)
        return self.lib.prv_argmax(_ptr(records), _ptr(ids), len(ids))

    # -- stage hooks
    def model_layout(self, slot):
        """kernel-side layout of a loaded field and the render_queue64_kernel<F, NDENSE> instance it runs on"""
        out = L.ModelLayout()
        self._chk(self.lib.prv_debug_model_layout(self.handle, slot, C.byref(out)))
        return {k: getattr(out, k) for k, _ in out._fields_}

    def render_clock_ghz(self):
        """average shader clock of the render launches since the statistics were last cleared (prv_debug_render_clock)"""
        cyc, ticks, hz = C.c_uint64(), C.c_uint64(), C.c_double()
        self._chk(self.lib.prv_debug_render_clock(self.handle, C.byref(cyc), C.byref(ticks), C.byref(hz)))
        return cyc.value / (ticks.value / hz.value) / 1e9 if ticks.value else 0.0

    def debug_raygen(self, camset, view, width, height, spp_index=0):
        n = width * height
        o, d, t = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32)
        self._chk(self.lib.prv_debug_raygen(self.handle, camset.handle, view, width, height, spp_index, _ptr(o), _ptr(d),
                                            _ptr(t)))
        return o, d, t

    def debug_encode(self, slot, pos):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        feat = np.zeros((pos.shape[0], 32), np.uint16)
        self._chk(self.lib.prv_debug_encode(self.handle, slot, _ptr(pos), pos.shape[0], _ptr(feat)))
        return feat

    def debug_field(self, slot, pos, dirs):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros((pos.shape[0], 36), np.float32)
        occ = np.zeros(pos.shape[0], np.int32)
        self._chk(self.lib.prv_debug_field(self.handle, slot, _ptr(pos), _ptr(dirs), pos.shape[0], _ptr(out), _ptr(occ)))
        return out, occ


    # -- mesh extraction (include/prv.h, mesh section)
    def density_grid(self, slot, res, aabb=None, use_occupancy=False):
        """the field's sigma at every grid point -> torch float32 tensor (rz, ry, rx) on the context's device; point i on axis
        a at lo[a] + float32(i) * step[a] (engine frame, aabb = (lo, hi), default the unit cube)"""
        o = mesh_opts(res, aabb, use_occupancy=use_occupancy)
        out = self.torch.empty((o.res[2], o.res[1], o.res[0]), dtype=self.torch.float32, device=self.device)
        self._chk(self.lib.prv_density_grid(self.handle, slot, C.byref(o), _ptr(out)))
        return out

    def marching_cubes(self, slot, res=256, aabb=None, threshold=2.5, use_occupancy=False, colors=True):
        """marching cubes on the field's density grid -> Mesh (engine frame)"""
        o = mesh_opts(res, aabb, threshold, use_occupancy, colors)
        h = C.c_void_p()
        self._chk(self.lib.prv_marching_cubes(self.handle, slot, C.byref(o), C.byref(h)))
        return Mesh(self, h)

    def marching_cubes_grid(self, sigma, aabb=None, threshold=2.5, valid=None):
        """marching cubes on a caller's sigma grid (torch float32 (rz, ry, rx) on the device) -> Mesh without colours.  valid: a
        uint8 or bool device tensor of the same shape -- only cells whose eight corners are valid give triangles, and no vertex is
        left unused (prv_marching_cubes_grid_valid); None: every point is valid"""
        if sigma.dim() != 3 or sigma.dtype != self.torch.float32 or not sigma.is_cuda:
            raise ValueError("sigma must be a float32 (rz, ry, rx) device tensor")
        sigma = sigma.contiguous()
        rz, ry, rx = sigma.shape
        o = mesh_opts((rx, ry, rz), aabb, threshold, colors=False)
        h = C.c_void_p()
        if valid is None:
            self._chk(self.lib.prv_marching_cubes_grid(self.handle, _ptr(sigma), C.byref(o), C.byref(h)))
            return Mesh(self, h)
        if tuple(valid.shape) != tuple(sigma.shape) or valid.dtype not in (self.torch.uint8, self.torch.bool) or not valid.is_cuda:
            raise ValueError("valid must be a uint8 or bool device tensor of sigma's shape")
        valid = valid.to(self.torch.uint8).contiguous()
        self._chk(self.lib.prv_marching_cubes_grid_valid(self.handle, _ptr(sigma), _ptr(valid), C.byref(o), C.byref(h)))
        return Mesh(self, h)

    # -- depth-map fusion (include/prv.h, depth-map fusion section)
    def tsdf_volume(self, res=256, aabb=None, trunc=None, colors=True):
        """a truncated signed distance volume on the grid of `marching_cubes_grid` (prv_tsdf_create) -> TSDFVolume.  res = N or
        (rx, ry, rz); aabb = (lo, hi) in the engine frame (None: the unit cube); trunc: the truncation distance in engine units
        (None: three times the largest grid step, an option value, not a measured one)"""
        o = tsdf_opts(res, aabb, trunc, colors)
        h = C.c_void_p()
        self._chk(self.lib.prv_tsdf_create(self.handle, C.byref(o), C.byref(h)))
        return TSDFVolume(self, h, o)

    # -- geometric evaluation (include/prv.h, geometric evaluation section)
    def _points(self, xyz):
        """(n, 3) float32 on the context's device, from a torch tensor or anything numpy takes"""
        t = self.torch
        if not isinstance(xyz, t.Tensor):
            xyz = t.from_numpy(np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3)))
        return xyz.to(device=self.device, dtype=t.float32).reshape(-1, 3).contiguous()

    def nn_index(self, points, algorithm=L.NN_GRID):
        """a nearest-neighbour index over `points` ((n, 3), any frame) -> NNIndex"""
        pts = self._points(points)
        o = L.NNOpts()
        self.lib.prv_nn_default_opts(C.byref(o))
        o.algorithm = int(algorithm)
        h = C.c_void_p()
        self._chk(self.lib.prv_nn_index_create(self.handle, _ptr(pts), pts.shape[0], C.byref(o), C.byref(h)))
        return NNIndex(self, h)

    def geometry_metrics(self, rec, ref, tau, ref_index=None):
        """accuracy / completeness / Chamfer / F-score between two point sets of one frame -> dict of prv_geom_metrics' fields
        (distances and tau in that frame)"""
        a, b = self._points(rec), self._points(ref)
        out = L.GeomMetrics()
        if ref_index is not None:  # the caller's index of `ref`: the reference side is not indexed again
            self._chk(self.lib.prv_geometry_metrics_indexed(self.handle, _ptr(a), a.shape[0], ref_index.handle, _ptr(b), b.shape[0],
                                                            float(tau), C.byref(out)))
        else:
            self._chk(self.lib.prv_geometry_metrics(self.handle, _ptr(a), a.shape[0], _ptr(b), b.shape[0], float(tau), C.byref(out)))
        return {name: getattr(out, name) for name, _ in L.GeomMetrics._fields_}

    def coverage(self, points, camset, view_ids, width, height, point_size=1, depth_tol=0.02, want_depth=False, occluder=None):
        """which of `points` ((n, 3), ENGINE frame) each of the views sees (prv_coverage_create) -> Coverage; want_depth: its
        `.depth` is the views' nearest-depth buffers, float32 [n_views, h, w] on the device, 0 = empty.  occluder: a Mesh --
        its rasterised surface, not the points, is what occludes (prv_coverage_create_occluded; point_size is ignored)"""
        t = self.torch
        pts = self._points(points)
        ids = self._ids(camset, view_ids)
        o = L.CoverageOpts(int(point_size), float(depth_tol))
        depth = t.empty((len(ids), int(height), int(width)), dtype=t.float32, device=self.device) if want_depth else None
        h = C.c_void_p()
        xyz = _ptr(pts) if pts.shape[0] else None
        if occluder is not None:
            self._chk(self.lib.prv_coverage_create_occluded(self.handle, xyz, pts.shape[0], occluder.handle, camset.handle, _ptr(ids),
                                                            len(ids), int(width), int(height), C.byref(o), _ptr(depth), C.byref(h)))
        else:
            self._chk(self.lib.prv_coverage_create(self.handle, xyz, pts.shape[0], camset.handle, _ptr(ids), len(ids), int(width),
                                                   int(height), C.byref(o), _ptr(depth), C.byref(h)))
        return Coverage(self, h, depth)

    # -- a rasterised surface (include/prv.h, mesh depth and the mesh occluder)
    def mesh_from_arrays(self, vertices, triangles, colors=None):
        """a Mesh from host arrays in the ENGINE frame: vertices (n, 3) float32, triangles (m, 3) uint32 (prv_mesh_from_arrays);
        colors (n, 3) uint8, if given, become its vertex colours (Mesh.set_colors)"""
        v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
        tr = np.ascontiguousarray(np.asarray(triangles, np.uint32).reshape(-1, 3))
        h = C.c_void_p()
        self._chk(self.lib.prv_mesh_from_arrays(self.handle, _ptr(v) if len(v) else None, len(v), _ptr(tr) if len(tr) else None, len(tr),
                                                C.byref(h)))
        m = Mesh(self, h)
        if colors is not None:
            try:
                m.set_colors(colors)
            except Exception:
                m.close()
                raise
        return m

    def mesh_depth(self, mesh, camset, view_ids, width, height):
        """the nearest surface depth of `mesh` per pixel and view (prv_mesh_depth) -> float32 [n_views, h, w] on the device, 0 =
        no triangle; pinhole cameras only"""
        t = self.torch
        ids = self._ids(camset, view_ids)
        depth = t.empty((len(ids), int(height), int(width)), dtype=t.float32, device=self.device)
        self._chk(self.lib.prv_mesh_depth(self.handle, mesh.handle, camset.handle, _ptr(ids), len(ids), int(width), int(height), _ptr(depth)))
        return depth

    def mesh_render(self, mesh, camset, view_ids, width, height, flip180=False, want_depth=False, want_triangles=False):
        """colour images of a vertex-coloured `mesh` (prv_mesh_render) -> uint8 [n_views, h, w, 4] on the device: the nearest
        triangle's colours interpolated perspective-correctly, alpha 255; background and exactly-white pixels 255, 255, 255, 0;
        flip180 turns each image by 180 degrees as splat_points does.  With want_depth / want_triangles a tuple that also holds
        the float32 depth (0 = empty) and / or the int32 triangle-id plane (-1, i.e. 0xFFFFFFFF, = empty), both [n_views, h, w]
        and never flipped.  Pinhole cameras only"""
        t = self.torch
        ids = self._ids(camset, view_ids)
        shape = (len(ids), int(height), int(width))
        rgba = t.empty(shape + (4,), dtype=t.uint8, device=self.device)
        depth = t.empty(shape, dtype=t.float32, device=self.device) if want_depth else None
        tri = t.empty(shape, dtype=t.int32, device=self.device) if want_triangles else None
        self._chk(self.lib.prv_mesh_render(self.handle, mesh.handle, camset.handle, _ptr(ids), len(ids), int(width), int(height),
                                           int(bool(flip180)), _ptr(rgba), _ptr(depth), _ptr(tri)))
        out = (rgba,) + ((depth,) if want_depth else ()) + ((tri,) if want_triangles else ())
        return out if len(out) > 1 else rgba

    def raster_stats(self):
        """the last mesh_depth / mesh_render / mesh-occluded coverage call: (view, triangle) pairs rasterised, and those the large path took"""
        out = (C.c_uint64 * 2)()
        self._chk(self.lib.prv_debug_raster_stats(self.handle, out))
        return dict(pairs=int(out[0]), large=int(out[1]))

    def mesh_stage_ms(self):
        """milliseconds of the last extraction's stages: density grid, classify + scans, emit, colours"""
        ms = (C.c_float * 4)()
        self._chk(self.lib.prv_debug_mesh_stages(self.handle, ms))
        return dict(grid=ms[0], classify_scan=ms[1], emit=ms[2], colors=ms[3])


def mesh_opts(res=256, aabb=None, threshold=2.5, use_occupancy=False, colors=True):
    """prv_mesh_opts: res = N or (rx, ry, rz); aabb = (lo[3], hi[3]) in the engine frame (None: the unit cube)"""
    lib = L.load()
    o = L.MeshOpts()
    lib.prv_mesh_default_opts(C.byref(o))
    r = [int(res)] * 3 if np.isscalar(res) else [int(x) for x in res]
    if len(r) != 3:
        raise ValueError("res must be an int or three ints (x, y, z)")
    for a in range(3):
        o.res[a] = r[a]
    if aabb is not None:
        lo, hi = aabb
        for a in range(3):
            o.aabb_lo[a], o.aabb_hi[a] = float(lo[a]), float(hi[a])
    o.threshold = float(threshold)
    o.use_occupancy = int(bool(use_occupancy))
    o.colors = int(bool(colors))
    return o


def _mesh_file_error(rc):
    raise PrvError(rc, (L.load().prv_last_error(None) or b"").decode())


def write_mesh(path, vertices, triangles, normals=None, colors=None, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """prv_mesh_write_file: engine-frame host arrays -> .ply / .obj in the dataset frame (no GPU involved)"""
    lib = L.load()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    c = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    off = np.ascontiguousarray(offset, np.float64).reshape(3)
    rc = lib.prv_mesh_write_file(str(path).encode(), v.shape[0], _ptr(v), _ptr(n), _ptr(c), t.shape[0], _ptr(t), float(scale),
                                 _ptr(off))
    if rc != 0:
        _mesh_file_error(rc)


class Mesh(_Handle):
    """a marching-cubes mesh (engine frame) owned by the library; the arrays are host copies taken at construction:
    vertices / normals (n, 3) float32, colors (n, 3) uint8, triangles (m, 3) uint32 (counter-clockwise seen from outside)"""

    _destroy = "prv_mesh_destroy"

    def __init__(self, ctx, handle):
        super().__init__(ctx, handle)
        nv, nt = C.c_uint64(), C.c_uint64()
        ctx._chk(ctx.lib.prv_mesh_counts(handle, C.byref(nv), C.byref(nt)))
        self.vertices = np.zeros((nv.value, 3), np.float32)
        self.normals = np.zeros((nv.value, 3), np.float32)
        self.colors = np.zeros((nv.value, 3), np.uint8)
        self.triangles = np.zeros((nt.value, 3), np.uint32)
        ctx._chk(ctx.lib.prv_mesh_get(handle, _ptr(self.vertices), _ptr(self.normals), _ptr(self.colors), _ptr(self.triangles)))

    def counts(self):
        nv, nt = C.c_uint64(), C.c_uint64()
        rc = self.ctx.lib.prv_mesh_counts(self.handle, C.byref(nv), C.byref(nt))
        if rc != 0:
            _mesh_file_error(rc)
        return nv.value, nt.value

    def set_colors(self, rgb):
        """the mesh's vertex colours from a host array (n_vertices, 3) uint8 (prv_mesh_set_colors); refreshes self.colors"""
        rgb = np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1, 3))
        self._chk(self.ctx.lib.prv_mesh_set_colors(self.handle, _ptr(rgb) if len(rgb) else None, len(rgb)))
        self.colors = rgb.copy()

    def save(self, path, scale=0.33, offset=(0.5, 0.5, 0.5)):
        """.ply / .obj in the dataset frame: (cycle(e) - offset) / scale (prv_mesh_save)"""
        off = np.ascontiguousarray(offset, np.float64).reshape(3)
        rc = self.ctx.lib.prv_mesh_save(self.handle, str(path).encode(), float(scale), _ptr(off))
        if rc != 0:
            _mesh_file_error(rc)

    def sample(self, n, seed=0, want_triangles=False):
        """n area-weighted surface points (prv_mesh_sample: stratified, a pure function of (mesh, n, seed)) -> float32 (n, 3)
        device tensor in the engine frame; with want_triangles also the int32 (n,) triangle ids"""
        t = self.ctx.torch
        xyz = t.empty((int(n), 3), dtype=t.float32, device=self.ctx.device)
        tri = t.empty((int(n),), dtype=t.int32, device=self.ctx.device) if want_triangles else None
        rc = self.ctx.lib.prv_mesh_sample(self.handle, int(n), int(seed) & (2 ** 64 - 1), _ptr(xyz), _ptr(tri))
        if rc != 0:
            raise PrvError(rc, (self.ctx.lib.prv_last_error(self.ctx.handle if self.ctx.handle else None) or b"").decode())
        return (xyz, tri) if want_triangles else xyz

    def components(self):
        """the mesh's connected components (prv_mesh_components; labelled once, cached by the library) -> dict of numpy
        arrays: per component first_vertex uint32, n_vertices / n_triangles uint64, lo / hi (n, 3) float32 (engine frame);
        vertex_component / triangle_component uint32, one id per vertex / triangle"""
        lib = self.ctx.lib
        nc = C.c_uint64()
        self._chk(lib.prv_mesh_components(self.handle, C.byref(nc)))
        table = (L.MeshComponent * max(1, nc.value))()
        self._chk(lib.prv_mesh_component_info(self.handle, nc.value, table))
        t = np.frombuffer(table, dtype=np.dtype([("first_vertex", "<u4"), ("reserved", "<u4"), ("n_vertices", "<u8"), ("n_triangles", "<u8"),
                                                 ("lo", "<f4", (3,)), ("hi", "<f4", (3,))]))[:nc.value]
        out = {k: t[k].copy() for k in ("first_vertex", "n_vertices", "n_triangles", "lo", "hi")}
        out["vertex_component"] = np.zeros(len(self.vertices), np.uint32)
        out["triangle_component"] = np.zeros(len(self.triangles), np.uint32)
        self._chk(lib.prv_mesh_labels(self.handle, _ptr(out["vertex_component"]), _ptr(out["triangle_component"])))
        return out

    def component_rounds(self):
        """hook + compress rounds the labelling took (prv_debug_mesh_component_rounds)"""
        r = C.c_int()
        self._chk(self.ctx.lib.prv_debug_mesh_component_rounds(self.handle, C.byref(r)))
        return r.value

    def filter(self, min_triangles=0, keep_largest=0, min_diagonal=0.0):
        """whole components kept, vertex and triangle order preserved (prv_mesh_filter) -> a new Mesh: components with at
        least min_triangles triangles, of those the keep_largest with the most triangles (ties to the lower id), of those
        the ones whose box diagonal (engine units) is at least min_diagonal; 0 switches a rule off"""
        o = L.MeshFilterOpts()
        self.ctx.lib.prv_mesh_filter_default_opts(C.byref(o))
        o.min_triangles, o.keep_largest, o.min_diagonal = int(min_triangles), int(keep_largest), float(min_diagonal)
        h = C.c_void_p()
        self._chk(self.ctx.lib.prv_mesh_filter(self.handle, C.byref(o), C.byref(h)))
        return Mesh(self.ctx, h)


def tsdf_opts(res=256, aabb=None, trunc=None, colors=True):
    """prv_tsdf_opts: res and aabb as `mesh_opts`; trunc None: 3 * the largest grid step of this grid, in float32"""
    m = mesh_opts(res, aabb)
    o = L.TsdfOpts()
    L.load().prv_tsdf_default_opts(C.byref(o))
    for a in range(3):
        o.res[a], o.aabb_lo[a], o.aabb_hi[a] = m.res[a], m.aabb_lo[a], m.aabb_hi[a]
    if trunc is None:
        f = np.float32
        with np.errstate(all="ignore"):  # (a bad res or box is the library's to refuse)
            trunc = f(3) * max((f(m.aabb_hi[a]) - f(m.aabb_lo[a])) / f(max(m.res[a] - 1, 1)) for a in range(3))
    o.trunc = float(trunc)
    o.colors = int(bool(colors))
    return o


class TSDFVolume(_Handle):
    """a truncated signed distance volume owned by the library (prv_tsdf): depth images of views are fused into it, and its
    zero level comes out as a Mesh.  res = (rx, ry, rz), aabb = (lo, hi), trunc, colors: what it was made with"""
    _destroy = "prv_tsdf_destroy"

    def __init__(self, ctx, handle, opts):
        super().__init__(ctx, handle)
        self.res = tuple(int(x) for x in opts.res)
        self.aabb = (tuple(float(x) for x in opts.aabb_lo), tuple(float(x) for x in opts.aabb_hi))
        self.trunc, self.colors = float(opts.trunc), bool(opts.colors)

    def _plane(self, t, name, dtype, shape):
        torch = self.ctx.torch
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be a {dtype} device tensor of shape {shape}")
        return t.contiguous()

    def integrate(self, camset, view_ids, depth, weight=None, rgba8=None):
        """fuse the views' images (prv_tsdf_integrate), in list order: depth float32 [n, h, w] (z along the optical axis, engine
        units, unflipped; <= 0, Inf and NaN pixels are skipped), weight float32 [n, h, w] or None (1), rgba8 uint8 [n, h, w, 4]
        or None (no colour); device tensors, the size is the depth tensor's"""
        torch = self.ctx.torch
        ids = self.ctx._ids(camset, view_ids)
        if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
            raise ValueError("depth must be a float32 [n_views, h, w] device tensor")
        n, h, w = (int(x) for x in depth.shape)
        if n != len(ids):
            raise ValueError(f"{len(ids)} views but {n} depth images")
        depth = self._plane(depth, "depth", torch.float32, (n, h, w))
        weight = self._plane(weight, "weight", torch.float32, (n, h, w))
        rgba8 = self._plane(rgba8, "rgba8", torch.uint8, (n, h, w, 4))
        self._chk(self.ctx.lib.prv_tsdf_integrate(self.handle, camset.handle, _ptr(ids), n, w, h, _ptr(depth), _ptr(weight), _ptr(rgba8)))

    def info(self):
        """-> dict(points, observed (W > 0), inside (observed, D < 0), band (observed, |D| < 1))"""
        out = (C.c_uint64 * 4)()
        self._chk(self.ctx.lib.prv_tsdf_info(self.handle, out))
        return dict(points=int(out[0]), observed=int(out[1]), inside=int(out[2]), band=int(out[3]))

    def grid(self, min_weight=0.0):
        """-> (grid float32 (rz, ry, rx): -D, NaN where not valid; valid uint8 (rz, ry, rx): W > 0 and W >= min_weight), on the
        device (prv_tsdf_grid): what `Context.marching_cubes_grid(grid, aabb, 0.0, valid=valid)` takes"""
        torch = self.ctx.torch
        rx, ry, rz = self.res
        grid = torch.empty((rz, ry, rx), dtype=torch.float32, device=self.ctx.device)
        valid = torch.empty((rz, ry, rx), dtype=torch.uint8, device=self.ctx.device)
        self._chk(self.ctx.lib.prv_tsdf_grid(self.handle, float(min_weight), _ptr(grid), _ptr(valid)))
        return grid, valid

    def mesh(self, min_weight=0.0):
        """the zero level as a Mesh (prv_tsdf_mesh): only cells whose corners are all observed with at least min_weight, vertex
        colours from the nearest grid point if the volume keeps colours"""
        h = C.c_void_p()
        self._chk(self.ctx.lib.prv_tsdf_mesh(self.handle, float(min_weight), C.byref(h)))
        return Mesh(self.ctx, h)

    def state(self):
        """host copies of the state (prv_debug_tsdf_state, a test hook) -> dict(D, W, WC: (rz, ry, rx) float32, C: (3, rz, ry, rx))"""
        rx, ry, rz = self.res
        out = dict(D=np.zeros((rz, ry, rx), np.float32), W=np.zeros((rz, ry, rx), np.float32), WC=np.zeros((rz, ry, rx), np.float32),
                   C=np.zeros((3, rz, ry, rx), np.float32))
        self._chk(self.ctx.lib.prv_debug_tsdf_state(self.handle, _ptr(out["D"]), _ptr(out["W"]), _ptr(out["WC"]), _ptr(out["C"])))
        return out


class NNIndex(_Handle):
    """a nearest-neighbour index owned by the library (prv_nn_index)"""
    _destroy = "prv_nn_index_destroy"

    def query(self, points):
        """-> (d2 float32 (m,), ids int32 (m,)) device tensors: squared distance to and id of each point's nearest reference
        point (d2 = (dx*dx + dy*dy) + dz*dz in float32, ties to the smallest id)"""
        t = self.ctx.torch
        q = self.ctx._points(points)
        d2 = t.empty((q.shape[0],), dtype=t.float32, device=self.ctx.device)
        ids = t.empty((q.shape[0],), dtype=t.int32, device=self.ctx.device)
        self._chk(self.ctx.lib.prv_nn_query(self.handle, _ptr(q), q.shape[0], _ptr(d2), _ptr(ids)))
        return d2, ids

    def info(self):
        n, dims, capped = C.c_uint64(), (C.c_int32 * 3)(), C.c_int32()
        self._chk(self.ctx.lib.prv_nn_index_info(self.handle, C.byref(n), dims, C.byref(capped)))
        return dict(n=n.value, dims=tuple(dims), capped=bool(capped.value))

    def tests(self):
        """(query, reference) pairs whose distance the last query formed"""
        v = C.c_uint64()
        self._chk(self.ctx.lib.prv_debug_nn_tests(self.handle, C.byref(v)))
        return v.value


class Coverage(_Handle):
    """the visibility bit matrix of a cloud under a list of views, owned by the library (prv_coverage).  Views are named by
    their POSITION in the list the handle was made with"""

    _destroy = "prv_coverage_destroy"

    def __init__(self, ctx, handle, depth=None):
        super().__init__(ctx, handle)
        self.depth = depth

    def info(self):
        n, v, cov = C.c_uint64(), C.c_int(), C.c_uint64()
        self._chk(self.ctx.lib.prv_coverage_info(self.handle, C.byref(n), C.byref(v), C.byref(cov)))
        return dict(n_points=n.value, n_views=v.value, n_coverable=cov.value)

    def visible(self):
        """-> uint64 (n_views,): the points each view sees on its own"""
        out = np.zeros(self.info()["n_views"], np.uint64)
        self._chk(self.ctx.lib.prv_coverage_visible(self.handle, _ptr(out)))
        return out

    def bits(self, view):
        """-> uint64 (ceil(n_points / 64),): bit j of word w = point 64 w + j is visible in the view at position `view`"""
        out = np.zeros((self.info()["n_points"] + 63) // 64, np.uint64)
        self._chk(self.ctx.lib.prv_coverage_bits(self.handle, int(view), _ptr(out)))
        return out

    def curve(self, order, want_first_seen=False):
        """the points the views order[0..j] see together, j = 0..k-1 -> uint64 (k,); with want_first_seen also an int32 device
        tensor (n_points,) holding uint32 bit patterns: the first j whose view sees the point, 0xFFFFFFFF = never"""
        order = np.ascontiguousarray(order, np.int32).ravel()
        out = np.zeros(len(order), np.uint64)
        first = None
        if want_first_seen:
            t = self.ctx.torch
            first = t.empty((self.info()["n_points"],), dtype=t.int32, device=self.ctx.device)
        self._chk(self.ctx.lib.prv_coverage_curve(self.handle, _ptr(order), len(order), _ptr(out),
                                                  _ptr(first) if first is not None and first.numel() else None))
        return (out, first) if want_first_seen else out

    def greedy(self, k):
        """k greedy rounds -> (chosen positions int32 (k,), cumulative covered counts uint64 (k,))"""
        k = int(k)
        chosen, covered = np.zeros(max(k, 0), np.int32), np.zeros(max(k, 0), np.uint64)
        self._chk(self.ctx.lib.prv_coverage_greedy(self.handle, k, _ptr(chosen), _ptr(covered)))
        return chosen, covered


def write_image_depth(path, image, scale):
    """run.py:307 `write_image_depth(outname, image, ref_transforms["scale"])`: a single-channel 16-bit PNG of channel 0 of
    `image` (a Depth-mode Testbed.render; a 2-D array is taken as it is), uint16(clip(round(z / scale * 1000), 0, 65535)):
    millimetres of the dataset unit, which a reader with depth_scale 0.001 (the reference's DefaultConfiguration.yaml:50)
    takes back to dataset units.  round is numpy's (halves to even).  The depth is written as rendered: premultiplied by
    opacity, with no un-premultiply and no opacity threshold, so partially transparent pixels read nearer than the surface.
    ASSUMED: upstream's write_image_depth lives in the unvendored scripts/common.py."""
    from PIL import Image

    z = np.asarray(image, np.float64)
    if z.ndim == 3:
        z = z[..., 0]
    mm = np.clip(np.round(np.nan_to_num(z) / float(scale) * 1000.0), 0, 65535).astype(np.uint16)
    Image.fromarray(mm).save(path)  # uint16 -> mode I;16


def engine_to_dataset(xyz, scale, offset):
    """engine-frame positions -> the dataset (transforms.json) frame: q = (e2, e0, e1), (q - offset) / scale"""
    e = np.asarray(xyz, np.float64).reshape(-1, 3)
    return (e[:, [2, 0, 1]] - np.asarray(offset, np.float64)) / float(scale)


GEOMETRY_FIELDS = tuple(name for name, _ in L.GeomMetrics._fields_)


def write_geometry_metrics(path, metrics):
    """a `*_geometry.txt` metrics file: one `name<TAB>value` line per field of prv_geom_metrics in struct order, in the style
    of the PSNR / SSIM metrics file (run.py:273-277); the doubles with 17 significant digits, so the file round-trips"""
    with open(path, "w") as f:
        for k in GEOMETRY_FIELDS:
            f.write(f"{k}\t{int(metrics[k])}\n" if k.startswith("n_") else f"{k}\t{float(metrics[k]):.17g}\n")


def read_geometry_metrics(path):
    out = {}
    with open(path) as f:
        for line in f:
            k, v = line.rstrip("\n").split("\t")
            out[k] = int(v) if k.startswith("n_") else float(v)
    return out


def dataset_to_engine(xyz, scale, offset):
    """the inverse of engine_to_dataset: q = p * scale + offset, e = (q1, q2, q0)"""
    q = np.asarray(xyz, np.float64).reshape(-1, 3) * float(scale) + np.asarray(offset, np.float64)
    return q[:, [1, 2, 0]]


class Comm(_Handle):
    """the ranks of one job as the C ABI sees them (include/prv.h, "several GPUs"): RCCL on device buffers, or the
    host-staged socket transport for ranks that share a GPU"""

    _destroy = "prv_comm_destroy"

    def __init__(self, ctx, rank, world, transport=None, rendezvous=None):
        super().__init__(ctx, C.c_void_p())
        ctx._chk(ctx.lib.prv_comm_create(ctx.handle, int(rank), int(world), transport.encode() if transport else None,
                                         rendezvous.encode() if rendezvous else None, C.byref(self.handle)))
        self.rank, self.world = int(rank), int(world)

    @property
    def transport(self):
        return self.ctx.lib.prv_comm_transport(self.handle).decode()

    @property
    def library(self):
        """{"path", "version", "found"}: the librccl file this communicator's calls land in (empty for "socket")"""
        path, how, ver = C.create_string_buffer(1024), C.create_string_buffer(128), C.c_int(0)
        self.ctx._chk(self.ctx.lib.prv_comm_library(self.handle, path, len(path), C.byref(ver), how, len(how)))
        return {"path": path.value.decode(), "version": int(ver.value), "found": how.value.decode()}

    def all_gather(self, send):
        """send: device tensor -> device uint8 tensor of world blocks in rank order"""
        t = self.ctx.torch
        send = send.contiguous()
        nbytes = send.numel() * send.element_size()
        out = t.empty(self.world * nbytes, dtype=t.uint8, device=send.device)
        self.ctx._chk(self.ctx.lib.prv_comm_all_gather(self.handle, _ptr(send), nbytes, _ptr(out)))
        self.ctx.synchronize()
        return out

    def barrier(self):
        self.ctx._chk(self.ctx.lib.prv_comm_barrier(self.handle))

    def score_views(self, method, slots, camset, n_views, opts, gt_shard=None, interleaved=True, want_stats=False):
        """the sharded scoring round -> (records[n_views] in view order, identical on every rank; local stats).  Methods as
        Context.score_views; gt_shard: SCORE_PSNR_COVERAGE only"""
        slots = np.ascontiguousarray(slots, np.int32)
        rec = np.zeros(int(n_views), RECORD_DTYPE)
        st = L.Stats()
        self.ctx._chk(self.ctx.lib.prv_score_views_sharded(self.ctx.handle, self.handle, method, _ptr(slots), len(slots),
                                                           camset.handle, int(n_views), int(bool(interleaved)), C.byref(opts),
                                                           _ptr(gt_shard), _ptr(rec), C.byref(st) if want_stats else None))
        return rec, st

    def exchange_models(self, n_members, desc):
        """member e trained in slot e of rank e % world -> slot e of every rank (device to device)"""
        self.ctx._chk(self.ctx.lib.prv_model_exchange(self.ctx.handle, self.handle, int(n_members), C.byref(desc)))


def shard_views(n_views, rank, world, interleaved=False):
    """prv_shard_views -> (ids, per_rank)"""
    lib = L.load()
    per = -(-int(n_views) // int(world)) if world > 0 else 0
    ids = np.zeros(max(1, per), np.int32)
    n = C.c_int()
    per = lib.prv_shard_views(int(n_views), int(rank), int(world), int(bool(interleaved)), _ptr(ids), C.byref(n))
    if per < 0:
        raise PrvError(per, "prv_shard_views")
    return ids[: n.value].copy(), per


def rank_host(records, view_ids):
    """ranking without a context (pure host entry point of the C ABI)"""
    lib = L.load()
    records = np.ascontiguousarray(records, RECORD_DTYPE)
    ids = np.ascontiguousarray(view_ids, np.int32)
    order = np.zeros(len(ids), np.int32)
    rc = lib.prv_rank(_ptr(records), _ptr(ids), len(ids), _ptr(order))
    if rc != 0:
        raise PrvError(rc, "prv_rank")
    return order


def train_opts(**kw):
    """prv_train_default_opts with overrides.  n_samples is a parameter of the sampling rule (include/prv.h): given without
    step_mode it selects PRV_STEP_FIXED_S (n_samples uniform samples per ray); step_mode given without it gets that rule's
    default (128 samples / 1024 steps)."""
    o = L.TrainOpts()
    rc = L.load().prv_train_default_opts(C.byref(o))
    if rc != 0:
        raise PrvError(rc, "prv_train_default_opts")
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown training option {k}")
        setattr(o, k, v)
    if "step_mode" in kw and "n_samples" not in kw:
        o.n_samples = L.NGP_MAX_STEPS if kw["step_mode"] == L.STEP_NGP else 128
    if "n_samples" in kw and "step_mode" not in kw:
        o.step_mode = L.STEP_FIXED_S
    if "step_mode" not in kw and max(o.patch_w, 1) * max(o.patch_h, 1) > 1:  # pixel patches are an option of the fixed rule
        o.step_mode = L.STEP_FIXED_S
        if "n_samples" not in kw:
            o.n_samples = 128
    return o


class Trainer(_Handle):
    """the in-process training step on one model slot (include/prv.h, training section)"""

    _destroy = "prv_train_destroy"

    def __init__(self, ctx, slot, camset, images_u8, opts=None):
        t = ctx.torch
        super().__init__(ctx, None)
        self.slot, self.camset = slot, camset
        self.images = images_u8.to(device=ctx.device, dtype=t.uint8).contiguous()  # kept alive here
        n, h, w, ch = self.images.shape
        if ch != 4 or n != len(camset):
            raise ValueError("images must be [n_views, h, w, 4], one per dataset camera")
        self.opts = opts if opts is not None else train_opts()
        self.handle = C.c_void_p()
        ctx._chk(ctx.lib.prv_train_create(ctx.handle, slot, camset.handle, _ptr(self.images), w, h, C.byref(self.opts),
                                          C.byref(self.handle)))

    def steps(self, n):
        losses = np.zeros(int(n), np.float32)
        self.ctx._chk(self.ctx.lib.prv_train_steps(self.handle, int(n), _ptr(losses)))
        return losses

    def info(self):
        s, u, n = C.c_uint32(), C.c_uint64(), C.c_uint64()
        self.ctx.lib.prv_train_info(self.handle, C.byref(s), C.byref(u), C.byref(n))
        return {"steps": s.value, "samples_last": u.value, "table_scalars": n.value,
                "active_rays": self.ctx.lib.prv_train_active_rays(self.handle)}

    def gradients(self):
        n = self.info()["table_scalars"]
        tg, mg, loss = np.zeros(n, np.float32), np.zeros(L.MLP_HALFS, np.float32), C.c_float()
        self.ctx._chk(self.ctx.lib.prv_train_gradients(self.handle, _ptr(tg), _ptr(mg), C.byref(loss)))
        return loss.value, tg, mg

    def master(self):
        n = self.info()["table_scalars"]
        tw, mw = np.zeros(n, np.float32), np.zeros(L.MLP_HALFS, np.float32)
        self.ctx._chk(self.ctx.lib.prv_train_master(self.handle, _ptr(tw), _ptr(mw)))
        return tw, mw

    def refresh_occupancy(self):
        self.ctx._chk(self.ctx.lib.prv_train_refresh_occupancy(self.handle))


def train_many(trainers, n):
    """n steps of every trainer side by side (prv_train_steps_multi) -> losses [n_trainers, n]"""
    ctx = trainers[0].ctx
    arr = (C.c_void_p * len(trainers))(*[t.handle for t in trainers])
    losses = np.zeros((len(trainers), int(n)), np.float32)
    ctx._chk(ctx.lib.prv_train_steps_multi(arr, len(trainers), int(n), _ptr(losses)))
    return losses


class _NerfSettings:
    """stands in for testbed.nerf (run.py:140,145,235)"""

    def __init__(self):
        self.render_min_transmittance = 0.01  # engine default; run.py:235 sets 1e-4 for evaluation
        self.render_with_lens_distortion = False
        self.sharpen = 0.0
        self.samples_per_ray = 0  # not a pyngp attribute: 0 = the engine's own stepping (dt = sqrt(3)/1024), N > 0 = N uniform samples per ray
        self.training = _Training()


class _FrameMeta:
    def __init__(self, w, h):
        self.resolution = (w, h)


class _Dataset:
    """testbed.nerf.training.dataset (run.py:240-241): n_images, metadata[i].resolution"""

    def __init__(self):
        self.n_images = 0
        self.metadata = []


class _Training:
    def __init__(self):
        self.dataset = _Dataset()


class Testbed:
    """The slice of pyngp.Testbed that run.py uses on the render path.

    run.py:90   testbed = ngp.Testbed()
    run.py:94   testbed.background_color = [0,0,0,1]
    run.py:109  testbed.load_training_data(scene)       -> scale/offset/intrinsics of the json
    run.py:127  testbed.load_snapshot(...)              -> load_model(...) / synthetic_model(...)
    run.py:231  testbed.snap_to_pixel_centers = True
    run.py:285  testbed.fov_axis = 0 ; testbed.fov = camera_angle_x * 180 / pi
    run.py:296  testbed.set_nerf_camera_matrix(M[:-1,:])
    run.py:304  image = testbed.render(w, h, spp, True)  -> float32 HxWx4, linear
    run.py:287  testbed.render_mode = ngp.Depth         -> render() returns (z, z, z, alpha) (prv_render_depth)
    """

    def __init__(self, device=0):
        self.ctx = Context(device)
        self.background_color = [0.0, 0.0, 0.0, 1.0]
        self.fov_axis = 0
        self.fov = 50.625
        self.snap_to_pixel_centers = False
        self.shall_train = False
        self.exposure = 0.0
        self.nerf = _NerfSettings()
        self.scale = 0.33
        self.offset = [0.5, 0.5, 0.5]
        self._matrix = np.eye(4)[:3]
        self._slot = 0
        self._have_model = False
        self.render_ground_truth = False
        self.render_mode = RenderMode.Shade
        self.steps_per_frame = 16  # ASSUMED: upstream trains a batch of steps per frame() call
        self.train_options = None  # TrainOpts override
        self._trainer = None
        self._last_loss = 0.0
        self._dataset_cams = None
        self._dataset_path = None
        self._training_view = None

    def load_training_data(self, path):
        with open(path) as f:
            meta = json.load(f)
        self.scale = float(meta.get("scale", 0.33))
        self.offset = [float(x) for x in meta.get("offset", [0.5, 0.5, 0.5])]
        if "camera_angle_x" in meta:
            self.fov_axis, self.fov = 0, meta["camera_angle_x"] * 180.0 / math.pi
        self.training_meta = meta
        self._drop_trainer()
        if self._dataset_cams is not None:
            self._dataset_cams.close()
            self._dataset_cams = None
        ds = self.nerf.training.dataset
        ds.n_images, ds.metadata = 0, []
        if meta.get("frames") and "w" in meta and "h" in meta:  # the dataset's own cameras (run.py:238-242)
            self._dataset_cams = self.ctx.cameras_from_dataset_json(path)
            self._dataset_path = str(path)
            ds.n_images = len(self._dataset_cams)
            ds.metadata = [_FrameMeta(int(meta["w"]), int(meta["h"])) for _ in range(ds.n_images)]

    def reset_network(self, desc, seed=0x1234):
        """a new network to train (what a fresh pyngp.Testbed holds, run.py:90)"""
        self.ctx.fresh_model(self._slot, desc, seed)
        self._have_model = True
        self._drop_trainer()

    def _drop_trainer(self):
        if self._trainer is not None:
            self._trainer.close()
            self._trainer = None

    @property
    def training_step(self):  # run.py:191
        return self._trainer.info()["steps"] if self._trainer is not None else 0

    @property
    def loss(self):  # run.py:206
        return self._last_loss

    def frame(self):
        """one iteration of `while testbed.frame()` (run.py:187): a batch of optimiser steps when shall_train"""
        if self.shall_train:
            if not self._have_model:
                raise PrvError(L.PRV_E_STATE, "no network: call reset_network(desc) or load a snapshot first")
            if self._dataset_cams is None:
                raise PrvError(L.PRV_E_STATE, "no training data loaded")
            if self._trainer is None:
                from .compat_server import load_dataset_bytes

                self._trainer = Trainer(self.ctx, self._slot, self._dataset_cams,
                                        load_dataset_bytes(self.ctx, self._dataset_path), self.train_options)
            self._last_loss = float(self._trainer.steps(self.steps_per_frame)[-1])
        return True

    def set_camera_to_training_view(self, i):  # run.py:242
        if self._dataset_cams is None or not 0 <= int(i) < len(self._dataset_cams):
            raise PrvError(L.PRV_E_INVALID, "no such training view")
        self._training_view = int(i)

    def load_model(self, desc, table, mlp, occ):
        self.ctx.load_model(self._slot, desc, table, mlp, occ)
        self._have_model = True
        self._drop_trainer()

    def synthetic_model(self, desc, seed):
        self.ctx.synthetic_model(self._slot, desc, seed)
        self._have_model = True
        self._drop_trainer()

    def load_snapshot(self, path):  # run.py:127
        """instant-ngp's own snapshots (.ingp / .msgpack) or this build's .prvf"""
        if str(path).lower().endswith((".ingp", ".msgpack")):
            self.ctx.load_ingp(self._slot, path)
        else:
            self.ctx.load_model_file(self._slot, path)
        self._have_model = True
        self._drop_trainer()

    def save_snapshot(self, path, include_optimizer_state=False):  # run.py:211
        if str(path).lower().endswith((".ingp", ".msgpack")):
            self.ctx.save_ingp(self._slot, path)
        else:
            self.ctx.save_model(self._slot, path)

    def set_nerf_camera_matrix(self, m):
        m = np.asarray(m, np.float64)
        if m.shape != (3, 4):
            raise ValueError("set_nerf_camera_matrix expects a 3x4 matrix")
        self._matrix = m
        self._training_view = None

    def render(self, width, height, spp=1, linear=True):
        if not self._have_model:
            raise PrvError(L.PRV_E_STATE, "no model loaded")
        if not linear:
            raise NotImplementedError("only linear=True is used on the reference path (run.py:245,247,304)")
        if self.fov_axis != 0:
            raise NotImplementedError("fov_axis must be 0 (run.py:285)")
        eff_spp = 1 if self.snap_to_pixel_centers else int(spp)
        opts = engine_render_opts(width, height, self.nerf.samples_per_ray, eff_spp, self.nerf.render_min_transmittance)
        if self.render_mode == RenderMode.Depth:
            return self._render_depth(width, height, opts)
        if self._training_view is not None:  # dataset camera: own intrinsics + lens (run.py:242-247)
            if self.render_ground_truth:
                img = self._ground_truth(self._training_view, width, height)
            else:
                img, _ = self.ctx.render(self._slot, self._dataset_cams, [self._training_view], opts, want_stats=False)
                img = img[0]
        else:
            tm = np.vstack([self._matrix, [0, 0, 0, 1]])
            cams = self.ctx.cameras_from_matrices(tm, self.fov * math.pi / 180.0, width, height, self.scale, self.offset)
            img, _ = self.ctx.render(self._slot, cams, None, opts, want_stats=False)
            img = img[0]
            cams.close()
        bg = self.ctx.torch.tensor(self.background_color, dtype=img.dtype, device=img.device)
        img = img + (1.0 - img[..., 3:4]) * bg  # composite over the background colour
        return img.cpu().numpy()

    def _render_depth(self, width, height, opts):
        """Depth mode: (h, w, 4) float32, r = g = b = z (premultiplied z-depth, engine units; prv_render_depth), a = opacity;
        the background colour is not composited"""
        if self._training_view is not None:
            if self.render_ground_truth:
                raise NotImplementedError("render_ground_truth has no depth image")
            rgba, depth, _ = self.ctx.render_depth(self._slot, self._dataset_cams, [self._training_view], opts, want_stats=False)
        else:
            tm = np.vstack([self._matrix, [0, 0, 0, 1]])
            cams = self.ctx.cameras_from_matrices(tm, self.fov * math.pi / 180.0, width, height, self.scale, self.offset)
            rgba, depth, _ = self.ctx.render_depth(self._slot, cams, None, opts, want_stats=False)
            cams.close()
        z = depth[0]
        return self.ctx.torch.stack([z, z, z, rgba[0][..., 3]], dim=-1).cpu().numpy()

    # ASSUMED: pyngp's signatures (upstream testbed.compute_marching_cubes_mesh / compute_and_save_marching_cubes_mesh are
    # not in the reference tree; run.py:282 passes (filename, [res, res, res])).  resolution = (x, y, z) grid points; aabb =
    # (lo, hi) in the engine frame (None: the unit cube, upstream's render_aabb); thresh = the sigma iso-level.
    def compute_marching_cubes_mesh(self, resolution=(256, 256, 256), aabb=None, thresh=2.5):
        """-> {"V": positions, "N": normals, "C": colours in [0, 1], "F": triangles}, in the dataset frame"""
        if not self._have_model:
            raise PrvError(L.PRV_E_STATE, "no model loaded")
        m = self.ctx.marching_cubes(self._slot, resolution, aabb, thresh)
        try:
            return {"V": engine_to_dataset(m.vertices, self.scale, self.offset).astype(np.float32),
                    "N": m.normals[:, [2, 0, 1]].copy(), "C": m.colors.astype(np.float32) / 255.0,
                    "F": m.triangles.astype(np.int32)}
        finally:
            m.close()

    def _without_floaters(self, m, keep_largest, min_triangles):
        """m, or with a rule set the filtered mesh (m is closed then)"""
        if not keep_largest and not min_triangles:
            return m
        try:
            return m.filter(min_triangles=min_triangles, keep_largest=keep_largest)
        finally:
            m.close()

    def compute_and_save_marching_cubes_mesh(self, filename, resolution=(256, 256, 256), aabb=None, thresh=2.5, keep_largest=0,
                                             min_triangles=0):  # run.py:282
        """keep_largest / min_triangles (this build's own; 0: off): drop density floaters before saving (Mesh.filter)"""
        if not self._have_model:
            raise PrvError(L.PRV_E_STATE, "no model loaded")
        m = self._without_floaters(self.ctx.marching_cubes(self._slot, resolution, aabb, thresh), keep_largest, min_triangles)
        try:
            m.save(filename, self.scale, self.offset)
        finally:
            m.close()

    TSDF_VIEW_BATCH = 16  # views rendered and fused per batch by compute_tsdf_mesh (the batches change no byte)

    def compute_tsdf_mesh(self, camset, view_ids, width, height, resolution=(256, 256, 256), aabb=None, trunc=None, level=0.5,
                          min_weight=0.0, keep_largest=0, min_triangles=0):
        """the surface the views `view_ids` of `camset` (None: all) SEE in the current model, by depth-map fusion (this build's
        own; include/prv.h, depth-map fusion): each view is rendered at width x height, one sample per pixel, under the Testbed's
        stepping rule -- `render_surface` for the first-crossing depth at opacity `level` (weight = hit, 0 or 1 at one sample per
        pixel) and `render_rgba8` for the colour -- fused into a volume of `resolution` points over `aabb` (engine frame, None:
        the unit cube) with truncation `trunc` (None: three grid steps), and the zero level is meshed; keep_largest /
        min_triangles: the floater filter of compute_and_save_marching_cubes_mesh.  -> Mesh, engine frame (close it)"""
        if not self._have_model:
            raise PrvError(L.PRV_E_STATE, "no model loaded")
        ids = self.ctx._ids(camset, view_ids)
        opts = engine_render_opts(width, height, self.nerf.samples_per_ray, 1, self.nerf.render_min_transmittance)
        with self.ctx.tsdf_volume(resolution, aabb, trunc, colors=True) as vol:
            for i in range(0, len(ids), self.TSDF_VIEW_BATCH):
                batch = ids[i:i + self.TSDF_VIEW_BATCH]
                _, _, depth, hit, _ = self.ctx.render_surface(self._slot, camset, batch, opts, level, want_stats=False)
                rgba8, _ = self.ctx.render_rgba8(self._slot, camset, batch, opts, want_stats=False)
                vol.integrate(camset, batch, depth, weight=hit, rgba8=rgba8)
            return self._without_floaters(vol.mesh(min_weight), keep_largest, min_triangles)

    def compute_and_save_tsdf_mesh(self, filename, camset, view_ids, width, height, resolution=(256, 256, 256), aabb=None, trunc=None,
                                   level=0.5, min_weight=0.0, keep_largest=0, min_triangles=0):
        """compute_tsdf_mesh, saved as compute_and_save_marching_cubes_mesh saves (.ply / .obj, dataset frame)"""
        m = self.compute_tsdf_mesh(camset, view_ids, width, height, resolution, aabb, trunc, level, min_weight, keep_largest, min_triangles)
        try:
            m.save(filename, self.scale, self.offset)
        finally:
            m.close()

    def compute_geometry_metrics(self, reference_points, resolution=(256, 256, 256), n_samples=1 << 20, tau=None, thresh=2.5, seed=0,
                                 keep_largest=0, min_triangles=0, surface="density", tsdf=None):
        """mesh the current model (marching cubes at `resolution`, iso-level `thresh`), sample n_samples surface points and
        compare them with reference_points ((n, 3), dataset frame) -> dict of prv_geom_metrics' fields in DATASET units.
        tau (dataset units) defaults to 1 % of the reference's largest extent.  keep_largest / min_triangles (0: off): the
        mesh is filtered first (Mesh.filter), so floaters do not enter accuracy and hausdorff_rec.
        surface = "tsdf": the mesh is compute_tsdf_mesh's at `resolution` instead; tsdf = dict(camset=, view_ids=, width=, height=)
        and optionally trunc, level, min_weight, aabb (thresh is not used)."""
        if not self._have_model:
            raise PrvError(L.PRV_E_STATE, "no model loaded")
        if surface not in ("density", "tsdf"):
            raise ValueError('surface must be "density" or "tsdf"')
        if surface == "tsdf" and (not tsdf or any(k not in tsdf for k in ("camset", "width", "height"))):
            raise ValueError('surface="tsdf" needs tsdf=dict(camset=, view_ids=, width=, height=, ...)')
        ref = np.asarray(reference_points, np.float64).reshape(-1, 3)
        if tau is None:
            tau = 0.01 * float((ref.max(axis=0) - ref.min(axis=0)).max())
        if surface == "tsdf":
            kw = dict(tsdf)
            m = self.compute_tsdf_mesh(kw.pop("camset"), kw.pop("view_ids", None), kw.pop("width"), kw.pop("height"), resolution,
                                       keep_largest=keep_largest, min_triangles=min_triangles, **kw)
        else:
            m = self._without_floaters(self.ctx.marching_cubes(self._slot, resolution, None, thresh, colors=False), keep_largest, min_triangles)
        try:
            rec = m.sample(n_samples, seed)
        finally:
            m.close()
        out = self.ctx.geometry_metrics(rec, dataset_to_engine(ref, self.scale, self.offset).astype(np.float32), float(tau) * self.scale)
        for k in ("accuracy", "completeness", "chamfer", "hausdorff_rec", "hausdorff_ref"):
            out[k] /= self.scale
        for k in ("accuracy_sq", "completeness_sq"):
            out[k] /= self.scale ** 2
        return out

    def compute_coverage(self, reference_points, camset, chosen, width=None, height=None, point_size=1, depth_tol=0.02, occluder=None):
        """how much of a reference surface the views `chosen` (camera ids of `camset`, in the order they were taken) see, against
        the greedy choice of as many views out of the WHOLE camset.  reference_points: (n, 3), dataset frame; the size defaults
        to the camset's.  Needs no model: nothing is trained or rendered.  occluder: a Mesh (ENGINE frame, as the library makes
        them) whose rasterised surface occludes, not the points.
        -> dict(n_points, n_coverable, covered[k] cumulative, greedy_covered[k], greedy_chosen[k] camera ids)"""
        ref = np.asarray(reference_points, np.float64).reshape(-1, 3)
        w, h = camset.size
        chosen = [int(v) for v in chosen]
        with self.ctx.coverage(dataset_to_engine(ref, self.scale, self.offset).astype(np.float32), camset, None,
                               int(width or w), int(height or h), point_size, depth_tol, occluder=occluder) as cov:
            info = cov.info()
            out = dict(n_points=info["n_points"], n_coverable=info["n_coverable"], covered=[], greedy_covered=[], greedy_chosen=[])
            if chosen:
                out["covered"] = [int(c) for c in cov.curve(chosen)]
                g, gc = cov.greedy(min(len(chosen), info["n_views"]))
                out["greedy_chosen"], out["greedy_covered"] = [int(v) for v in g], [int(c) for c in gc]
        return out

    def _ground_truth(self, i, width, height):
        """render_ground_truth (run.py:241-244): the dataset image of view i, linear premultiplied RGBA"""
        from .compat_server import load_reference_images

        if getattr(self, "_gt_cache_path", None) != self._dataset_path:
            self._gt_cache = load_reference_images(self.ctx, self._dataset_path)
            self._gt_cache_path = self._dataset_path
        img = self._gt_cache[i]
        if tuple(img.shape[:2]) != (height, width):
            raise NotImplementedError("ground-truth images are only served at their own resolution (run.py:240-244)")
        return img
