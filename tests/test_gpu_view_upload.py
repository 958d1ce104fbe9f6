"""Every C ABI call that takes a camera set and a view list sends its cameras through one pinned staging block into one device
buffer (stage_views / send_views in prv_api.cpp, PinnedStage in prv_buffer.hpp), and no call waits for the stream any more
before it returns.  Here the calls follow each other without a synchronise in between, each with a view list of its own, and
every output must be, byte for byte, what the same call gives alone on a fresh context: the next call's cameras must not reach
the staging or the device buffer before the previous call's kernels have read theirs."""
import numpy as np
import pytest

from nerf_prv_amd import api
from tests import util
from tests.test_gpu_raster import box_mesh, sphere

pytestmark = pytest.mark.gpu

W, H = 16, 12
N_CAMS = 8
LISTS = ([5], [0, 3, 6], [7, 1, 4, 2, 6])  # three view lists of the set: 1, 3 and 5 views
CENTRE = np.array([0.5, 0.5, 0.5], np.float32)
CONSUMERS = ["mesh_depth", "first_hit", "splat", "coverage", "select"]


class Env:
    """a context with the smallest synthetic field in slot 0 and the inputs of the five consumers"""

    def __init__(self, oracle):
        self.ctx = ctx = api.Context(0)
        t = ctx.torch
        ctx.synthetic_model(0, api.field_desc(**util.SMALL), util.SEED_A)
        tms, self.scale, self.offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(N_CAMS))
        self.cams = ctx.cameras_from_matrices(tms, util.FOV_X, W, H, self.scale, self.offset)
        self.mesh = ctx.mesh_from_arrays(*box_mesh(CENTRE - 0.25, CENTRE + 0.25))
        rng = np.random.default_rng(5)
        self.points = sphere(rng, 200, 0.3)  # engine frame; the cameras stand 1.5 from its centre
        self.world = ((self.points.astype(np.float64) - np.asarray(self.offset, np.float64)) / self.scale).astype(np.float32)
        self.rgb = rng.integers(0, 256, (200, 3), dtype=np.uint8)
        # constant planes: every pixel fully opaque, one bit of entropy, located 1.4 along the axis (inside the cube)
        self.planes = [t.full((5, H, W), v, dtype=t.float32, device=ctx.device) for v in (1.0, 1.0, 1.4)]
        self.handles = []

    def call(self, name, ids, w=W, h=H):
        """starts the consumer and returns what it handed back, unread"""
        ctx, n = self.ctx, len(ids)
        if name == "mesh_depth":
            return ctx.mesh_depth(self.mesh, self.cams, ids, w, h)
        if name == "first_hit":
            return ctx.first_hit(0, self.cams, ids, w, h)
        if name == "splat":
            return ctx.splat_points(self.world, self.rgb, self.scale, self.offset, self.cams, ids, w, h, point_size=3)
        if name == "coverage":
            self.handles.append(ctx.coverage(self.points, self.cams, ids, w, h, point_size=2, want_depth=True))
            return self.handles[-1]
        chosen, gains, vox, q = ctx.select_from_images(self.cams, ids, *[p[:n].contiguous() for p in self.planes],
                                                       api.select_opts(k=min(2, n), grid_res=16), want_words=True)
        return chosen, gains, vox, q

    def read(self, name, raw):
        """the bytes of a finished call's output (the context has been synchronised)"""
        if name == "coverage":
            n = raw.info()["n_views"]
            return b"".join([raw.visible().tobytes(), raw.depth.cpu().numpy().tobytes()] + [raw.bits(v).tobytes() for v in range(n)])
        if name == "select":
            return b"".join(x.tobytes() if isinstance(x, np.ndarray) else x.cpu().numpy().tobytes() for x in raw)
        return raw.cpu().numpy().tobytes()

    def close(self):
        for h in self.handles:
            h.close()
        self.mesh.close()
        self.cams.close()
        self.ctx.close()


_alone = {}


def alone(oracle, name, ids, w=W, h=H):
    """the call on a fresh context, a synchronise before and after; computed once per (consumer, list, size)"""
    key = (name, tuple(ids), w, h)
    if key not in _alone:
        env = Env(oracle)
        try:
            env.ctx.synchronize()
            raw = env.call(name, ids, w, h)
            env.ctx.synchronize()
            _alone[key] = env.read(name, raw)
        finally:
            env.close()
    return _alone[key]


@pytest.fixture(scope="module")
def env(oracle):
    e = Env(oracle)
    yield e
    e.close()


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_interleaved_consumers_each_see_their_own_views(env, oracle, order, shift):
    names = CONSUMERS if order == "forward" else CONSUMERS[::-1]
    ids = {name: LISTS[(i + shift) % 3] for i, name in enumerate(CONSUMERS)}  # neighbours never share a list
    raw = [(name, env.call(name, ids[name])) for name in names]  # no synchronise in between
    env.ctx.synchronize()
    got = {name: env.read(name, r) for name, r in raw}
    for name in CONSUMERS:
        want = alone(oracle, name, ids[name])
        assert got[name] == want, (name, ids[name], order)
        assert len(set(want)) > 1  # (not a blank output)
    # what is compared depends on the list: another list of the same length gives other bytes
    assert alone(oracle, "first_hit", [5]) != alone(oracle, "first_hit", [2])


def test_the_staging_grows_while_the_previous_upload_is_in_flight(oracle):
    # A view is one CamDev and one int of the upload (prv_device.hpp: CamDev = c2w[12] + fx, fy, cx, cy + lens[4] floats +
    # cull[4] ints = 24 words = 96 bytes; + 4 = 100 bytes), and the staging starts at 8192 bytes: 81 views fit (8100), 82 do
    # not (8200).  first_hit waits for nothing, so the 82-view call finds the 2-view upload in flight when it must grow
    cam_bytes = 4 * (12 + 4 + 4 + 4)
    n_big = 8192 // (cam_bytes + 4) + 1
    assert cam_bytes == 96 and n_big == 82 and (n_big - 1) * (cam_bytes + 4) <= 8192 < n_big * (cam_bytes + 4)
    lists = ([1, 6], [(3 * i + 1) % N_CAMS for i in range(n_big)], [4, 2])
    e = Env(oracle)
    try:
        raw = [e.call("first_hit", ids, 8, 6) for ids in lists]
        e.ctx.synchronize()
        got = [e.read("first_hit", r) for r in raw]
    finally:
        e.close()
    for ids, g in zip(lists, got):
        assert g == alone(oracle, "first_hit", ids, 8, 6), len(ids)
    assert got[0] != got[2] and len(set(got[1])) > 1


def test_the_method_5_score_reads_the_cameras_of_its_own_render(env, oracle):
    opts = api.render_opts(W, H, 64, 1, 1e-4)
    ids = LISTS[1]
    gt_host = np.random.default_rng(9).random((len(ids), H, W, 4), dtype=np.float32)

    def score(e, foreign):
        gt = e.ctx.torch.from_numpy(gt_host).to(e.ctx.device)
        if foreign:
            e.call("first_hit", LISTS[2])  # another five cameras go through the staging and the device buffer first
        rec, _ = e.ctx.score_views(api.L.SCORE_PSNR_COVERAGE, [0], e.cams, ids, opts, gt=gt)
        return rec

    fresh = Env(oracle)
    try:
        want = score(fresh, False)
    finally:
        fresh.close()
    got = score(env, True)
    assert got.tobytes() == want.tobytes()
    assert np.isfinite(want["score"]).all() and len(set(want["score"].tolist())) == len(ids)
