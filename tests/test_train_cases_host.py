"""The inputs of tests/test_gpu_train_edges.py (tests/train_cases.py) exercise what they claim: shown with the CPU oracle alone, before a
GPU is involved.  These are conditions on the inputs, not measurements of the code under test: the seeds in train_cases.py were
chosen until the oracle met them.  CPU only."""
import numpy as np
import pytest

from tests import train_cases as tc


def _trainer(oracle, params, kw, ds, imgs, **opts):
    f = oracle.OracleField(oracle.desc(**kw), params=params)
    return oracle.OracleTrainer(f, oracle.train_opts(**opts), tc.oracle_cameras(oracle, ds), imgs)


def _awkward_batch(oracle, name, **rule):
    ds = tc.awkward_datasets(oracle)[name]
    _, params = tc.awkward_field(oracle, name, dense="step_mode" not in rule)
    tr = _trainer(oracle, params, tc.TINY, ds, tc.awkward_images(name, len(ds["tms"])), n_rays=64, occ_every=0, seed=ds["seed"], **rule)
    tr.loss_only()
    return tr.samples_last


def test_awkward_datasets_are_what_their_names_say(oracle):
    sets = tc.awkward_datasets(oracle)
    assert list(sets) == tc.AWKWARD and len(sets["mixed"]["tms"]) == len(tc.AWKWARD) - 1
    assert sum("k1" in sets[n]["intr"] for n in tc.AWKWARD[:-1]) == 6  # the lens on half of them, pinhole on the rest
    for name in ("inside", "inside_off_centre"):
        origins = [np.array(c.c2w).reshape(3, 4)[:, 3] for c in tc.oracle_cameras(oracle, sets[name])]
        assert any(np.all(o > 0.0) and np.all(o < 1.0) for o in origins), name  # strictly inside the unit cube
    assert all(np.array_equal(np.array(c.c2w).reshape(3, 4)[:, 3], [0.5, 0.5, 0.5]) for c in tc.oracle_cameras(oracle, sets["inside"]))
    assert not np.array_equal(np.array(tc.oracle_cameras(oracle, sets["inside_off_centre"])[0].c2w).reshape(3, 4)[:, 3], [0.5, 0.5, 0.5])
    # axis: the middle pixel's ray has two zero components, and the trainer's 64-ray batch of step 0 holds that pixel
    _, d, _ = oracle.raygen(tc.oracle_cameras(oracle, sets["axis"])[0], tc.W, tc.H)
    assert np.sum(d[7 * tc.W + 12] == 0.0) == 2
    u24, seed = oracle.lib().orc_rng_u24, sets["axis"]["seed"]
    assert (12, 7) in [((u24(seed, 1, j) * tc.W) >> 24, (u24(seed, 2, j) * tc.H) >> 24) for j in range(64)]


@pytest.mark.parametrize("name", tc.AWKWARD)
def test_awkward_batches_list_samples(oracle, name):
    """64 rays: `away` lists nothing; every other set lists more than 200 samples under the engine's marcher, under the fixed rule and
    under both patch shapes, and `far` more than 50.  One exception, stated: of `graze5`'s 64 rays about eight hit the cube at all, which
    24 samples each cannot bring to 200 in any grid -- there the floor is 100 (four rays' worth)"""
    counts = {"ngp": _awkward_batch(oracle, name, **tc.RULES["ngp"]), "fixed_s": _awkward_batch(oracle, name, **tc.RULES["fixed_s"])}
    for pw, ph in tc.PATCHES:
        counts[f"{pw}x{ph}"] = _awkward_batch(oracle, name, n_samples=24, patch_w=pw, patch_h=ph)
    if name == "away":
        assert set(counts.values()) == {0}
        return
    assert counts["ngp"] > 200, (name, counts)
    floor = 100 if name == "graze5" else 200
    assert all(n > floor for k, n in counts.items() if k != "ngp"), (name, counts)
    assert name != "far" or min(counts.values()) > 50


def test_random_cases_cover_what_they_claim(oracle):
    cases = [tc.random_ngp_case(i) for i in range(tc.N_RANDOM)]
    assert len(cases) == 16 and all(c["opts"]["step_mode"] == oracle.STEP_NGP and c["opts"]["occ_every"] == 0 for c in cases)
    assert all(c["opts"].get("deterministic", 0) == 0 and c["opts"].get("patch_w", 0) == 0 for c in cases)
    zero = capped = long_rays = one_cell = 0
    for c in cases:
        params, ds, imgs = tc.realise(oracle, c)
        tr = _trainer(oracle, params, c["field"], ds, imgs, **c["opts"])
        tr.loss_only()
        n, active = tr.samples_last, tr.active_rays
        assert n <= 1.2 * tc.SAMPLE_BUDGET, (c["id"], n)  # "about": the CPU side of a case stays at a few seconds
        zero += n == 0
        one_cell += c["occupancy"] == "cell" and c["field"]["occ_res"] > 1 and n >= 200
        long_rays += n > 128 * active  # the mean of the rays' listed samples: SOME ray has more than 128 live steps (two mask words)
        if n and c["opts"]["n_samples"] < oracle.NGP_MAX_STEPS:
            # the same rays under the full cap: more samples means that the case's own cap cut a ray
            more = _trainer(oracle, params, c["field"], ds, imgs, **dict(c["opts"], n_samples=oracle.NGP_MAX_STEPS, n_rays=active, target_samples=0))
            more.loss_only()
            assert more.active_rays == active and more.samples_last >= n
            capped += more.samples_last > n
    assert zero <= 2
    assert sum(c["field"]["occ_res"] % 4 != 0 for c in cases) >= 3  # no coarse grid
    assert capped >= 2 and long_rays >= 2
    assert {c["occupancy"] for c in cases} == {"all", "sparse", "cell"}
    assert one_cell >= 1  # a single occupied cell that a few hundred samples fall into: the mode is not only empty batches
    assert {c["opts"]["n_samples"] for c in cases} == set(tc.STEP_CAPS) == {1, 63, 64, 65, 200, 1023, 1024}  # every cap, 65 and 1023 included
    assert {c["field"]["occ_res"] for c in cases} == set(tc.OCC_RES) == {1, 3, 4, 8, 12, 17, 20, 32}
    assert len({c["camera"]["kind"] for c in cases}) >= 4 and any(c["camera"]["kind"] == "hemisphere" for c in cases)


@pytest.mark.parametrize("occ_res,F", sorted({(R, F) for R, F, _ in tc.refresh_cases()}))
def test_refresh_threshold_sits_in_an_empty_band(oracle, occ_res, F):
    """between 20 % and 80 % of the cells on, and no cell's density within a relative 1e-4 of the threshold: GPU and oracle then
    have to agree on EVERY bit (they agree on sigma to about 1e-6, tests/test_gpu_train.py)"""
    f, _ = tc.refresh_field(oracle, occ_res, F)
    sigma = tc.cell_sigma(oracle, f)
    assert sigma.shape == (occ_res ** 3,) and np.all(sigma > 0)
    thresh = tc.place_threshold(sigma)
    assert thresh == float(np.float32(thresh))
    assert 0.2 <= np.mean(sigma > np.float32(thresh)) <= 0.8
    assert not tc.in_band(sigma, thresh, tc.BAND).any()


def test_refresh_cases_select_both_kernels_and_both_instances():
    cases = tc.refresh_cases()
    assert len(cases) == 20 and {c[0] for c in cases} == {3, 12, 17, 20, 32} and {c[1] for c in cases} == {4, 2} and {c[2] for c in cases} == {None, "0"}
    assert {R ** 3 % 32 != 0 for R, _, _ in cases} == {True, False}  # a partial last word and whole words


def test_the_oracle_ema_accessor(oracle):
    f, _ = tc.refresh_field(oracle, 3, 4)
    ds = tc.awkward_datasets(oracle)["axis"]
    tr = oracle.OracleTrainer(f, oracle.train_opts(n_rays=1, n_samples=1, occ_every=0, occ_decay=0.5, occ_sigma_thresh=1e9), tc.oracle_cameras(oracle, ds),
                              np.zeros((1, tc.H, tc.W, 4), np.uint8))
    assert tr.ema().shape == (27,) and not tr.ema().any()  # starts at 0
    tr.refresh_occupancy()
    first = tr.ema()
    assert np.all(first > 0)
    first[:] = 0  # a copy: writing to it changes nothing
    tr.refresh_occupancy()
    assert np.all(tr.ema() > 0) and np.array_equal(tr.ema(), tc.cell_sigma(oracle, f))  # max(sigma / 2, sigma) = sigma


def test_ema_case_holds_cells_on_by_the_decay_alone(oracle):
    """12 steps with a refresh every second one while the densities fall: cells whose EMA is above the threshold although their
    current density is below it -- what the decayed maximum exists for"""
    params, ds, imgs, opts = tc.ema_case(oracle)
    tr = _trainer(oracle, params, tc.EMA_CASE["field"], ds, imgs, **opts)
    for _ in range(tc.EMA_CASE["steps"]):
        tr.step()
    ema, sigma = tr.ema(), tc.cell_sigma(oracle, tr.field())
    thresh = np.float32(opts["occ_sigma_thresh"])
    held = (ema > thresh) & (sigma < thresh)
    assert held.sum() >= 20
    assert np.array_equal(tc.bits_of(tr.params()[2], len(ema)), ema > thresh)
    assert 0.05 < np.mean(ema > thresh) < 0.95
