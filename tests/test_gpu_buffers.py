"""Device memory the library holds (prv_debug_live_bytes) is back where it was after the smallest object of every family
has lived and died on a context of its own -- handles first or context first -- and does not move across a refused call.
The session's shared context keeps its grow-only workspaces and stays out of the balance."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded, the order api.Context keeps: one HIP runtime per process, torch's)

from nerf_prv_amd import api
from tests import instances, util

pytestmark = pytest.mark.gpu
L = api.L
FIELD = instances.MATRIX["F4_finer_than_table"].kw  # the smallest tables of the matrix
W = H = 16


def held():
    return int(L.load().prv_debug_live_bytes())


def lifecycle(c, oracle):
    """the smallest object of every family -> (handles in creation order, {name: call on an inert handle})"""
    t = c.torch
    for slot, seed in ((0, util.SEED_A), (1, util.SEED_B)):
        c.synthetic_model(slot, api.field_desc(**FIELD), seed)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(2))
    cams = c.cameras_from_matrices(tms, util.FOV_X, W, H, scale, offset)
    for spp in (1, 2):
        img, _ = c.render(0, cams, None, api.render_opts(W, H, 32, spp, 1e-4))
        assert tuple(img.shape[:3]) == (2, H, W)
    mesh = c.marching_cubes(0, res=8)
    mesh.components()
    kept = mesh.filter(keep_largest=1)
    pts = np.random.default_rng(5).random((64, 3), dtype=np.float32)
    index = c.nn_index(pts)
    d2, ids = index.query(pts[:8])
    assert bool((d2 == 0).all()) and ids.cpu().numpy().tolist() == list(range(8))
    cov = c.coverage(pts, cams, None, W, H)
    cov_mesh = c.coverage(pts, cams, None, W, H, occluder=mesh)
    assert cov.info()["n_points"] == cov_mesh.info()["n_points"] == 64
    imgs = t.zeros((2, 8, 8, 4), dtype=t.uint8)
    opts = api.train_opts(n_rays=8, n_samples=8)
    first = api.Trainer(c, 0, cams, imgs, opts)
    assert np.isfinite(first.steps(1)).all()
    parked_from = held()
    first.close()  # its buffers stay parked with the context ...
    trainer = api.Trainer(c, 0, cams, imgs, opts)
    assert held() == parked_from  # ... and the next trainer of the same shape takes every one of them back
    assert np.isfinite(trainer.steps(1)).all()
    comm = api.Comm(c, 0, 1, transport="socket")
    rec, _ = comm.score_views(L.SCORE_ENSEMBLE_RGB, [0, 1], cams, 2, api.render_opts(W, H, 32, 1, 1e-4))
    assert len(rec) == 2
    inert = {"mesh": (mesh.counts, L.PRV_E_STATE), "filtered mesh": (kept.components, L.PRV_E_STATE), "index": (index.info, L.PRV_E_STATE),
             "coverage": (cov.info, L.PRV_E_STATE), "occluded coverage": (lambda: cov_mesh.greedy(1), L.PRV_E_STATE),
             "trainer": (lambda: trainer.steps(1), L.PRV_E_INVALID), "communicator": (comm.barrier, L.PRV_E_INVALID)}
    return [cams, mesh, kept, index, cov, cov_mesh, trainer, comm], inert


def test_handles_destroyed_before_their_context_leave_nothing(oracle):
    start = held()
    c = api.Context(0)
    handles, _ = lifecycle(c, oracle)
    assert held() > start
    for h in handles:
        h.close()
    c.close()
    assert held() == start


def test_a_context_destroyed_first_leaves_inert_handles_and_nothing_else(oracle):
    start = held()
    c = api.Context(0)
    handles, inert = lifecycle(c, oracle)
    c.close()
    assert held() == start  # the context's end freed what its handles held
    for name, (call, code) in inert.items():
        with pytest.raises(api.PrvError) as e:
            call()
        assert e.value.code == code, name
        if code == L.PRV_E_STATE:
            assert "context has been destroyed" in str(e.value), name
    for h in handles:
        h.close()
    assert held() == start


def test_a_trainer_built_from_parked_buffers_equals_one_built_from_fresh_memory(oracle):
    """A destroyed trainer's buffers wait in its context for the next trainer, which takes them by size: whatever has to start
    at zero is zeroed when a trainer is created, wherever its memory comes from.  Context A runs a patch trainer on slot 0 first
    (its slot_of, tile_live, ray_loss, ... are parked with their last contents), then a deterministic trainer on slot 1, whose
    tab_gq, block_tot and tile_live come out of that pool; context B runs the deterministic trainer alone, on fresh
    allocations.  Deterministic training is reproducible bit for bit, so the two must agree in every bit."""
    d = api.field_desc(**FIELD)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(4))
    pixels = np.random.default_rng(11).integers(0, 256, (4, H, W, 4), dtype=np.uint8)
    shape = dict(n_rays=256, n_samples=24, step_mode=L.STEP_FIXED_S)

    def run(parked_first):
        start = held()
        c = api.Context(0)
        for slot in (0, 1):
            c.fresh_model(slot, d, util.SEED_A)
        cams = c.cameras_from_matrices(tms, util.FOV_X, W, H, scale, offset)
        imgs = c.torch.from_numpy(pixels)
        if parked_first:
            first = api.Trainer(c, 0, cams, imgs, api.train_opts(patch_w=2, patch_h=2, **shape))
            assert np.isfinite(first.steps(2)).all()
            first.close()
        tr = api.Trainer(c, 1, cams, imgs, api.train_opts(deterministic=1, occ_every=4, **shape))
        losses = tr.steps(4)
        got = [losses, *tr.master(), *c.export_model(1, d), np.uint64(tr.info()["samples_last"])]
        assert np.isfinite(losses).all() and tr.info()["samples_last"] > 0
        tr.close()
        cams.close()
        c.close()
        assert held() == start
        return [np.ascontiguousarray(a).tobytes() for a in got]

    from_pool, fresh = run(True), run(False)
    for name, a, b in zip(("losses", "master table", "master MLP", "fp16 table", "fp16 MLP", "occupancy", "samples_last"), from_pool, fresh):
        assert a == b, name


def test_a_refused_call_holds_nothing_afterwards(oracle):
    """ordinary error returns that come after an allocation can have happened, as the suites of their families make them"""
    start = held()
    c = api.Context(0)
    t = c.torch
    c.synthetic_model(0, api.field_desc(**FIELD), util.SEED_A)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(2))
    cams = c.cameras_from_matrices(tms, util.FOV_X, W, H, scale, offset)
    intr = dict(fl_x=60.0, fl_y=58.0, cx=41.0, cy=21.5, w=80, h=45, k1=0.12, k2=-0.05, p1=0.01, p2=-0.008)
    lens = c.cameras_from_matrices_intr(tms[[1]], intr, scale, offset)
    pts = np.random.default_rng(6).random((64, 3), dtype=np.float32)
    flat = c.mesh_from_arrays([[0.2, 0.2, 0.2], [0.4, 0.4, 0.4], [0.6, 0.6, 0.6]], [[0, 1, 2]])  # one triangle, no area
    imgs = t.zeros((2, 8, 8, 4), dtype=t.uint8)
    nan = pts.copy()
    nan[3, 1] = np.nan
    refused = [("a sample of a mesh without area", lambda: flat.sample(16), L.PRV_E_STATE, "no area"),
               ("an occluder with a lens camera", lambda: c.coverage(pts, lens, None, W, H, occluder=flat), L.PRV_E_INVALID, "lens"),
               ("a view id out of range", lambda: c.coverage(pts, cams, [0, 2], W, H), L.PRV_E_INVALID, "out of range"),
               ("an index over a non-finite point", lambda: c.nn_index(nan), L.PRV_E_INVALID, "non-finite"),
               ("a trainer with a negative learning rate", lambda: api.Trainer(c, 0, cams, imgs, api.train_opts(n_rays=8, n_samples=8, lr=-1e-3)),
                L.PRV_E_INVALID, "optimiser"),
               ("a trainer on an empty slot", lambda: api.Trainer(c, 3, cams, imgs, api.train_opts(n_rays=8, n_samples=8)), L.PRV_E_STATE, "empty")]
    for name, call, code, text in refused:
        before = held()
        with pytest.raises(api.PrvError) as e:
            call()
        assert e.value.code == code and text in str(e.value), name
        assert held() == before, name
    for h in (flat, lens, cams):
        h.close()
    c.close()
    assert held() == start
