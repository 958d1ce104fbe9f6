"""prv_train_opts.deterministic = 1 leaves what tests/golden/train_deterministic.json holds, bit for bit: the order of the sample
list decides every sum behind it (tiles, fixed-point table gradient, dW slots), so losses, masters, the exported model and the
budget's ray counts are EQUAL to the recorded run or the list order has changed.  The golden was recorded on the MI355X from the
trainer whose ray blocks appended in block order one after another; a trainer that orders them any other way (per-block counts,
a scan, the append) must reproduce it.  Cases: the shapes where blocks lie beyond the step's ray budget, where a block is partly
filled, where the blocks outnumber the scan's threads, where whole blocks list nothing, patches, and two trainers side by side."""
import hashlib
import json
import os

import numpy as np
import pytest

from nerf_prv_amd import api
from tests import train_cases as tc
from tests.test_gpu_train import scene, start  # noqa: F401  (scene: the module's fixture, F4 and F2)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_deterministic.json")
NGP = dict(step_mode=api.L.STEP_NGP, n_samples=1024)

# name -> (options on top of deterministic = 1, steps)
CASES = {
    "fixed_200": (dict(n_rays=200, occ_every=4, occ_sigma_thresh=0.3), 12),  # test_deterministic_training_is_bit_reproducible's shape
    # starts at 8 active rays of 300 and grows: most blocks lie beyond the budget, which moves every step
    "ngp_budget": (dict(NGP, n_rays=300, target_samples=8192, occ_every=2, occ_sigma_thresh=2.5), 6),
    "ngp_1_ray": (dict(NGP, n_rays=1), 3),  # one partly filled block
    "ngp_3_rays": (dict(NGP, n_rays=3), 3),
    "fixed_4097": (dict(n_rays=4097, n_samples=16, target_samples=0), 3),  # 1025 blocks, the last one holds one ray
    "patch_2x2": (dict(n_rays=203, patch_w=2, patch_h=2), 4),  # 203: no multiple of the patch size
    "patch_4x4": (dict(n_rays=203, patch_w=4, patch_h=4), 4),
}


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _digest(ctx, tr, slot, desc, losses, grads=None):
    info = tr.info()
    d = {"losses": _sha(losses), "master": _sha(*tr.master()), "export": _sha(*ctx.export_model(slot, desc)),
         "samples_last": int(info["samples_last"]), "active_rays": int(info["active_rays"])}
    if grads is not None:  # the loss and the gradients of the first batch, listed by prv_train_gradients' own ray launch
        d["gradients"] = _sha(np.float32(grads[0]), grads[1], grads[2])
    return d


def _check(key, got):
    want = json.load(open(GOLD))[key]
    assert got == want, key


@pytest.mark.parametrize("name", list(CASES))
def test_a_deterministic_run_is_the_recorded_one(ctx, oracle, scene, request, name):
    opts, n_steps = CASES[name]
    f, otr, gtr = start(ctx, oracle, scene, deterministic=1, **opts)
    grads = gtr.gradients()
    losses = gtr.steps(n_steps)
    got = _digest(ctx, gtr, 3, api.field_desc(**scene[0]), losses, grads)
    gtr.close()
    assert got["samples_last"] > 0
    _check(f"{name}/F{scene[0]['n_features']}", got)


def test_blocks_that_list_nothing_between_blocks_that_do(ctx, oracle):
    """graze5 under the engine's marcher (tests/train_cases.py): about eight of the 64 rays hit the cube, through a quarter-occupied
    grid -- whole blocks list zero samples between blocks that list some"""
    ds = tc.awkward_datasets(oracle)["graze5"]
    _, params = tc.awkward_field(oracle, "graze5")
    imgs = tc.awkward_images("graze5", len(ds["tms"]))
    desc = api.field_desc(**tc.TINY)
    ctx.load_model(3, desc, *params)
    cams = ctx.cameras_from_matrices_intr(ds["tms"], ds["intr"], ds["scale"], ds["offset"])
    gtr = api.Trainer(ctx, 3, cams, ctx.torch.from_numpy(imgs), api.train_opts(n_rays=64, occ_every=0, seed=ds["seed"], deterministic=1, **NGP))
    grads = gtr.gradients()
    losses = gtr.steps(3)
    got = _digest(ctx, gtr, 3, desc, losses, grads)
    gtr.close()
    cams.close()
    assert 0 < got["samples_last"] < 64 * 100
    _check("graze5_ngp", got)


def test_two_deterministic_trainers_side_by_side(ctx, oracle, scene, monkeypatch):
    """prv_train_steps_multi: each of two deterministic trainers on slots of their own gives, bit for bit, what it gives alone --
    on the same backward grid.  A trainer alone launches two backward blocks per CU, trainers side by side one each
    (prv_train_api.inc: bwd_blocks), and the f32 dW sums follow the grid (a block sums its own tiles, the reduction walks the
    blocks' slots): recorded without this, `alone` and `together` had the same sample counts and (F = 4) the same losses but
    other masters.  That is the backward pass, not the list order: PRV_TRAIN_BWD_BLOCKS pins the grid to one block per CU for
    both."""
    monkeypatch.setenv("PRV_TRAIN_BWD_BLOCKS", str(ctx.torch.cuda.get_device_properties(0).multi_processor_count))
    kw, ocams, cams, imgs = scene
    d = api.field_desc(**dict(kw, table_amp=1e-4))
    u8 = ctx.torch.from_numpy(imgs)

    def member(e):
        ctx.fresh_model(e, d, 500 + e)
        return api.Trainer(ctx, e, cams, u8, api.train_opts(n_rays=256, n_samples=24, seed=900 + e, occ_every=4, occ_sigma_thresh=0.1, deterministic=1))

    alone = []
    for e in range(2):
        tr = member(e)
        alone.append(_digest(ctx, tr, e, d, tr.steps(6)))
        tr.close()
    trs = [member(e) for e in range(2)]
    losses = api.train_many(trs, 6)
    together = [_digest(ctx, tr, e, d, losses[e]) for e, tr in enumerate(trs)]
    for tr in trs:
        tr.close()
    assert together == alone and alone[0] != alone[1]
    _check(f"multi/F{kw['n_features']}", alone)
