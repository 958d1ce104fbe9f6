"""The image-space kernels (prv_kernels.hip: quantize_kernel and spp_reduce_kernel's byte branch, score_psnr_kernel, the three
ssim kernels, the two ensemble-score passes, score_finalize_kernel) against tests/image_ref.py, the float64 statement of what
they compute, on the input families of tests/image_cases.py and at the launch shapes where the kernels change path: one /
several / the 64-block cap of score_blocks(), the second 64-view block of the finalize kernels, the 512-addend chunks of the
sequential sum, a single SSIM window, the 4096-block grid-stride cap of the quantise kernel.  Bars: bytes equal outside the
band image_ref derives and within 1 inside it; PSNR within the per-case bound derived there; SSIM within image_ref.SSIM_TOL;
EnsembleRGBDensity bit for bit, EnsembleRGB within n_terms 2^-52 |term|max; rankings identical.  tests/test_image_ref_host.py
holds the oracle's float32 twin to the same bars without a GPU.

Image-level entry points only; the cull-rectangle test renders with model slot 28 (slots of this file: 28..29)."""
import functools
import math

import numpy as np
import pytest

from nerf_prv_amd import api
from tests import image_cases as cases
from tests import image_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

SLOT = 28  # slots of this file: 28..29
f32 = np.float32
FAMILIES = cases.quantize_families()
BG = cases.BACKGROUNDS[3]  # (0.5, 0, 1, 1): every term of the composite is live


def dev(ctx, a):
    return ctx.torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def assert_bytes(got, q, name, boundary=False):
    """got (n, 4) uint8 against image_ref's Quantized: within 1 everywhere, equal outside the band"""
    diff = np.abs(got.astype(int) - q.byte.astype(int))
    stray = (diff != 0) & ~q.in_band
    print(f"{name}: {int((diff != 0).sum())} of {diff.size} bytes differ, {int(q.in_band.sum())} in band, {int(stray.sum())} outside it")
    assert diff.max() <= 1, (name, np.argwhere(diff > 1)[:5])
    if not boundary:
        assert not stray.any(), (name, np.argwhere(stray)[:5], q.y[stray][:5], q.band[stray][:5])


# ------------------------------------------------------------------ quantisation

@pytest.mark.parametrize("name", list(FAMILIES))
def test_quantize_family(ctx, oracle, name):
    px, bg = FAMILIES[name]
    got = ctx.quantize_rgba8(dev(ctx, px), bg).cpu().numpy()
    twin = oracle.quantize_rgba8(px, bg)
    assert_bytes(got, ref.quantize_exact(px, bg), name, boundary=name.startswith("boundary"))
    # no powf on the way to the alpha byte: the same IEEE operations on both sides
    assert np.array_equal(got[:, 3], twin[:, 3]), name
    if name.startswith("nonfinite"):
        assert np.array_equal(got, twin), name  # prv.h's clamp rule (NaN -> 0); beyond it the twin's bytes are the contract


@functools.lru_cache(maxsize=None)
def _sized(n):
    a, b = cases.random_pair(0x51 + n, 1, 1, n, 0.3)
    px = np.concatenate([a[0, 0, : (n + 1) // 2], b[0, 0, : n // 2]])
    return px, ref.quantize_exact(px, BG)


@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 1])
def test_quantize_sizes(ctx, n):
    """one thread, a partial block, two blocks, and one pixel past what 4096 blocks cover in one stride"""
    px, q = _sized(n)
    got = ctx.quantize_rgba8(dev(ctx, px), BG).cpu().numpy()
    assert got.shape == (n, 4)
    assert_bytes(got, q, f"n={n}")
    assert q.in_band.mean() < 0.01


@pytest.fixture(scope="module")
def scene(ctx, oracle):
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    return tms, scale, offset


def test_render_bytes_at_spp3_follow_the_same_rule(ctx, scene):
    """spp_reduce_kernel's byte branch: the bytes of a 3-sub-sample render are quantize_rgba8 of its floats, and those are
    within the band of the float64 bytes"""
    tms, scale, offset = scene
    w, h = 40, 24
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    opts = api.render_opts(w, h, 32, 3, 1e-4, background=BG)
    u8, _ = ctx.render_rgba8(SLOT, cs, None, opts)
    img, _ = ctx.render(SLOT, cs, None, opts)
    assert np.array_equal(u8.cpu().numpy(), ctx.quantize_rgba8(img, BG).cpu().numpy())
    px = img.cpu().numpy().reshape(-1, 4)
    assert (px[:, 3] > 0.5).sum() > 100 and (px[:, 3] == 0).sum() > 100  # object and background both in view
    assert_bytes(u8.cpu().numpy().reshape(-1, 4), ref.quantize_exact(px, BG), "spp3")
    cs.close()


# ------------------------------------------------------------------ PSNR / coverage

def assert_psnr_record(rec, a, b, bg, weight, oracle, tag):
    want = ref.psnr_coverage(a, b, bg, weight)
    print(f"{tag}: psnr {rec['psnr']:.6f} ref {want.psnr:.6f} |d| {abs(rec['psnr'] - want.psnr):.2e} bound {want.psnr_tol:.2e}; eps_max {want.eps_max:.2e}")
    assert math.isfinite(want.psnr_tol) and want.psnr_tol < 0.05, tag  # the bound says something about this case
    assert abs(float(rec["psnr"]) - want.psnr) <= want.psnr_tol + abs(want.psnr) * 2.0 ** -24, tag
    assert abs(float(rec["score"]) - want.score) <= want.score_tol, tag
    assert abs(float(rec["coverage"]) - want.coverage) <= want.coverage_tol, tag
    s, p, c = oracle.score_view(a, b, bg, weight)  # the twin, at the bars of test_gpu_sweep.py
    assert rec["score"] == pytest.approx(s, rel=1e-6) and rec["psnr"] == pytest.approx(p, rel=1e-5) and rec["coverage"] == pytest.approx(c, rel=1e-5)
    return want


@pytest.fixture
def weights(ctx):
    def set_weight(w):
        ctx.set_coverage_weight(w)
    yield set_weight
    ctx.set_coverage_weight(1.0)


@pytest.mark.parametrize("npix", [1, 4096, 4097, 8193, 262144 + 1])
def test_psnr_pixel_counts(ctx, oracle, weights, npix):
    """one block up to 4096 pixels, two from 4097, three from 8193, the 64-block cap past 262144; two different views"""
    a, b = cases.random_pair(0xB10C + npix, 2, 1, npix, 0.05)
    b[1] = np.clip(a[1] + (b[1] - a[1]) * 4, 0, 1)  # the second view is noisier: a different record
    ta, tb = dev(ctx, a), dev(ctx, b)
    for weight in (0.0, 2.5):
        weights(weight)
        rec = ctx.score_psnr_images(ta, tb, BG)
        wants = [assert_psnr_record(rec[v], a[v], b[v], BG, weight, oracle, f"npix={npix} w={weight} view {v}") for v in range(2)]
        if npix > 1:
            assert wants[0].psnr > wants[1].psnr + 3 and rec["psnr"][0] > rec["psnr"][1] + 3


@functools.lru_cache(maxsize=None)
def _views65():
    """65 views of 5 x 5, every one at its own noise level"""
    a, b = cases.random_pair(0x65, 65, 5, 5, 0.05)
    for v in range(65):
        b[v] = np.clip(a[v] + (b[v] - a[v]) * f32(0.1 + 0.1 * v), 0, 1)
    return a, b


def test_psnr_65_views(ctx, oracle):
    """score_finalize_kernel runs 64 views per block: view 64 is the second block's only thread"""
    a, b = _views65()
    rec = ctx.score_psnr_images(dev(ctx, a), dev(ctx, b), BG)
    for v in range(65):
        assert_psnr_record(rec[v], a[v], b[v], BG, 1.0, oracle, f"view {v}")
    assert len(set(rec["psnr"].tolist())) == 65


def test_psnr_families(ctx, oracle):
    for name, (a, b, bg) in cases.image_families().items():
        if a.shape[0] * a.shape[1] > 10000:
            continue  # launch shapes are test_psnr_pixel_counts' business
        rec = ctx.score_psnr_images(dev(ctx, a[None]), dev(ctx, b[None]), bg)
        assert_psnr_record(rec[0], a, b, bg, 1.0, oracle, name)


def test_psnr_pixel_on_the_knee(ctx, oracle, weights):
    """ONE pixel whose three channels are exactly the knee 0.0031308f against a ground truth 2^-10 below it: the pixel belongs
    to the linear piece (x <= knee).  The two pieces differ by 2e-6 at the knee, the difference of the pair is 4e-5: taking the
    power piece moves the PSNR by 0.4 dB, the bound here is below 0.01 dB"""
    weights(0.0)
    k = cases.KNEE
    a = np.array([[[[k, k, k, 1.0]]]], f32)
    b = np.array([[[[k * f32(1 - 2.0 ** -10)] * 3 + [1.0]]]], f32)
    rec = ctx.score_psnr_images(dev(ctx, a), dev(ctx, b), (0, 0, 0, 0))
    want = assert_psnr_record(rec[0], a[0], b[0], (0, 0, 0, 0), 0.0, oracle, "knee pixel")
    assert want.psnr_tol < 0.01
    assert want.mse == pytest.approx((ref.K_LIN * float(k) * 2.0 ** -10) ** 2, rel=1e-3)


def test_identical_images_rank_last_among_numbers(ctx, oracle):
    """mse = 0 exactly (the same operations on the same bits): psnr +inf, score -inf; prv_rank orders -inf after every number
    and before a NaN.  (A NaN COLOUR is clamped to 0 like any other; a NaN alpha reaches the coverage sums: score NaN.)"""
    a, b = cases.random_pair(0x1D, 4, 9, 7, 0.05)
    b[0], b[2] = a[0], a[2]
    a[3, 4, 3, 3] = np.nan
    rec = ctx.score_psnr_images(dev(ctx, a), dev(ctx, b), BG)
    for v in (0, 2):
        assert rec["psnr"][v] == np.inf and rec["score"][v] == -np.inf
        assert ref.psnr_coverage(a[v], b[v], BG).psnr == math.inf
    assert math.isfinite(rec["score"][1]) and math.isnan(rec["score"][3]) and math.isnan(rec["coverage"][3]) and math.isfinite(rec["psnr"][3])
    ids = np.arange(4)
    assert ctx.rank(rec, ids).tolist() == [1, 0, 2, 3] == oracle.rank(rec["score"], ids).tolist()
    assert ctx.argmax(rec, ids) == 1


# ------------------------------------------------------------------ SSIM

def _const(h, w, rgb, a=1.0):
    img = np.empty((h, w, 4), f32)
    img[..., :3], img[..., 3] = rgb, a
    return img


@pytest.mark.parametrize("shape", cases.SSIM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ssim_shapes(ctx, shape):
    """one window (5x5), one row / one column of windows, ow * oh not a multiple of 256 (69x61: 65 x 57), several blocks
    (260x260: 256 x 256 windows of 66564 pixels = 17 blocks); every noise scale and background"""
    h, w = shape
    groups = {}
    for name, (a, b, bg) in cases.image_families().items():
        if a.shape[:2] == (h, w) and name.startswith("noise"):
            groups.setdefault(bg, []).append((name, a, b))
    assert len(groups) >= 3
    for bg, items in groups.items():
        a, b = np.stack([i[1] for i in items]), np.stack([i[2] for i in items])
        ps, ss = ctx.evaluate_images(dev(ctx, a), dev(ctx, b), bg)
        for v, (name, _, _) in enumerate(items):
            want = ref.ssim(a[v], b[v], bg)
            print(f"{name}: ssim {ss[v]:.9f} ref {want:.9f} |d| {abs(ss[v] - want):.2e}")
            assert abs(ss[v] - want) <= ref.SSIM_TOL, name
            p = ref.psnr_coverage(a[v], b[v], bg, 0.0)
            assert abs(ps[v] - p.psnr) <= p.psnr_tol, name


def test_ssim_pixel_families(ctx):
    for name, (a, b, bg) in cases.image_families().items():
        if name.startswith("noise"):
            continue
        _, ss = ctx.evaluate_images(dev(ctx, a[None]), dev(ctx, b[None]), bg)
        want = ref.ssim(a, b, bg)
        print(f"{name}: ssim {ss[0]:.9f} ref {want:.9f} |d| {abs(ss[0] - want):.2e}")
        assert abs(ss[0] - want) <= ref.SSIM_TOL, name


def test_ssim_65_views(ctx):
    """ssim_finalize_kernel's second block; every view against its own reference"""
    a, b = _views65()
    ps, ss = ctx.evaluate_images(dev(ctx, a), dev(ctx, b), BG)
    for v in range(65):
        assert abs(ss[v] - ref.ssim(a[v], b[v], BG)) <= ref.SSIM_TOL, v
        p = ref.psnr_coverage(a[v], b[v], BG, 0.0)
        assert abs(ps[v] - p.psnr) <= p.psnr_tol, v
    assert len(set(ss.tolist())) == 65


def test_ssim_known_answers(ctx):
    a, _ = cases.random_pair(1, 3, 9, 11, 0.05)
    for bg in cases.BACKGROUNDS:
        ps, ss = ctx.evaluate_images(dev(ctx, a), dev(ctx, a.copy()), bg)
        assert (ss == 1.0).all() and (ps == np.inf).all()  # sAB, sA and sB are the same bits: (2 s + c2) / (s + s + c2) = 1
    black, white = _const(7, 8, 0.0), _const(7, 8, 1.0)
    ps, ss = ctx.evaluate_images(dev(ctx, black[None]), dev(ctx, white[None]), (0, 0, 0, 0))
    assert abs(ps[0]) < 1e-5 and 0 < ss[0] < 1.1e-4 and abs(ss[0] - ref.ssim(black, white, (0, 0, 0, 0))) <= ref.SSIM_TOL
    for ga, gb in ((0.25, 0.5), (0.0, 0.1), (1.0, 0.9)):
        A, B = _const(8, 6, ga), _const(8, 6, gb)
        la, lb = ref.luminance(A, (0, 0, 0, 1))[0, 0], ref.luminance(B, (0, 0, 0, 1))[0, 0]
        _, ss = ctx.evaluate_images(dev(ctx, A[None]), dev(ctx, B[None]), (0, 0, 0, 1))
        assert abs(ss[0] - (2 * la * lb + ref.C1) / (la * la + lb * lb + ref.C1)) <= ref.SSIM_TOL
    # the hand-computed window of tests/test_image_ref_host.py
    A, B = _const(5, 5, 0.0), _const(5, 5, 0.0)
    A[2, 2, :3] = B[2, 2, :3] = B[0, 0, :3] = 1.0
    _, ss = ctx.evaluate_images(dev(ctx, A[None]), dev(ctx, B[None]), (0, 0, 0, 0))
    assert abs(ss[0] - 0.9047821560737367) <= ref.SSIM_TOL and abs(ref.ssim(A, B, (0, 0, 0, 0)) - 0.9047821560737367) < 1e-12


@pytest.mark.parametrize("shape", [(4, 9), (9, 4)])
def test_ssim_refuses_images_without_a_window(ctx, shape):
    a = np.zeros((1,) + shape + (4,), f32)
    with pytest.raises(api.PrvError) as e:
        ctx.evaluate_images(dev(ctx, a), dev(ctx, a), (0, 0, 0, 0))
    assert e.value.code == api.L.PRV_E_INVALID


# ------------------------------------------------------------------ ensemble sums

@pytest.mark.parametrize("E", [1, 2, 8])
@pytest.mark.parametrize("method", [2, 3])
def test_ensemble_chunk_boundaries(ctx, oracle, method, E):
    """the sequential sum's 512-addend chunks: n_terms on, one before and one after a boundary (see image_cases.ENSEMBLE_NPIX
    for how K = 3 and K = 2 reach them), one member (the ABI accepts it), all addends negative, all addends gated to 0"""
    fn = ref.ensemble_rgb if method == 2 else ref.ensemble_rgbdensity
    for npix in cases.ENSEMBLE_NPIX[method]:
        views = [cases.members(npix * 8 + E, E, npix, mode) for mode in cases.ENSEMBLE_MODES]
        imgs = [np.stack([views[v][e] for v in range(len(views))]) for e in range(E)]  # member e: (views, npix, 4)
        rec = ctx.score_ensemble_images(method, [dev(ctx, i) for i in imgs])
        want = np.array([fn(v) for v in views])
        for v, mode in enumerate(cases.ENSEMBLE_MODES):
            if method == 3:
                assert rec["score"][v] == want[v], (npix, mode)
            else:
                assert abs(rec["score"][v] - want[v]) <= ref.ensemble_rgb_bound(views[v]), (npix, mode, rec["score"][v], want[v])
                if mode == "gated" or E == 1:
                    assert rec["score"][v] == 0.0
                elif mode == "negative":
                    assert rec["score"][v] < 0
        assert (rec["psnr"] == 0).all() and (rec["coverage"] == 0).all()
        ids = np.arange(len(views))
        assert ctx.rank(rec, ids).tolist() == oracle.rank(want, ids).tolist(), (npix, rec["score"], want)


# ------------------------------------------------------------------ the cull rectangle of the fused PSNR round

def occupied_box(occ, R):
    """the box the library culls against: the occupied cells' bounding box, one cell of margin (prv_field_plan.hpp: summarize_occupancy)"""
    bits = np.unpackbits(occ.view(np.uint8), bitorder="little")[: R ** 3].reshape(R, R, R)  # z, y, x
    lo, hi = np.zeros(3), np.zeros(3)
    for a, axis in enumerate((2, 1, 0)):
        idx = np.nonzero(bits.any(axis=tuple(i for i in range(3) if i != axis)))[0]
        lo[a], hi[a] = f32(f32(idx.min() - 1) / f32(R)), f32(f32(idx.max() + 2) / f32(R))
    return lo, hi


def cull_rectangle(c2w, intr, lo, hi, W, H):
    """[x0, x1) x [y0, y1): the bounding rectangle of the grown box's eight projected corners, two pixels of margin, clamped to
    the image (prv_device.hpp, CamDev::cull); None when a corner is not in front of the camera"""
    c2w = np.asarray(c2w, np.float64).reshape(3, 4)
    o, Mi = c2w[:, 3], np.linalg.inv(c2w[:, :3])
    grow = 1e-3 + 1e-5 * np.abs(o - 0.5).max() + 1e-4
    us, vs = [], []
    for k in range(8):
        c = Mi @ (np.array([hi[a] + grow if (k >> a) & 1 else lo[a] - grow for a in range(3)]) - o)
        if not c[2] > 1e-3:
            return None
        us.append(intr[0] * c[0] / c[2] + intr[2])
        vs.append(intr[1] * c[1] / c[2] + intr[3])
    clamp = lambda v, lo_, hi_: max(lo_, min(hi_, v))
    return (clamp(math.floor(min(us)) - 2, 0, W), clamp(math.floor(min(vs)) - 2, 0, H),
            clamp(math.ceil(max(us)) + 3, 1, W), clamp(math.ceil(max(vs)) + 3, 0, H))


def test_psnr_round_ignores_what_lies_outside_the_cull_rectangle(ctx, oracle, scene):
    """prv_score_views (method 5, 1 spp) renders only the 16 x 16 tiles that meet a view's cull rectangle into a scratch image
    and score_psnr_kernel takes every pixel outside the rectangle as (0, 0, 0, 0) WITHOUT reading it.  With a ground truth that
    is non-zero everywhere and a scratch image that still holds another view's pixels there, both must hold: the records are
    byte-equal to scoring the full render, and within bound of image_ref on the render.  Cameras: those of
    test_march_rejection_on_awkward_cameras (tests/test_gpu_parity.py) whose rectangle is a proper sub-rectangle, and one more
    whose rectangle ends on a tile edge (x1 = 48): column 48 is then in a tile the round does not render, so only the
    rectangle test keeps the stale pixels out"""
    w, h, S = 64, 48, 48
    _, _, occ = ctx.export_model(SLOT, api.field_desc(**util.SMALL))
    lo, hi = occupied_box(occ, util.SMALL["occ_res"])

    def tm(t):
        m = np.eye(4)
        m[:3, 3] = t
        return m

    sc, off = 5.0, np.array([0.5, 0.5, 0.5])
    cams = [("axis", tm([0, 0, 0.3]), util.FOV_X), ("far", tm([0, 0, 60.0]), 0.02), ("graze3", tm([0.12, 0.06, 0.3]), 0.6),
            ("tile edge", tm([0.005, 0.01, 0.5]), 0.9)]
    opts = api.render_opts(w, h, S, 1, 1e-4, background=BG)
    inside = ctx.cameras_from_matrices(tm([0, 0, 0])[None], util.FOV_X, w, h, sc, off)  # in the object: every pixel is lit
    full, _ = ctx.render(SLOT, inside, None, opts)
    assert float(full[0, :, :, 3].min()) > 0.05
    gt = np.random.default_rng(0xC011).random((1, h, w, 4)).astype(f32) * f32(0.9) + f32(0.05)
    tgt = dev(ctx, gt)
    for name, m, fov in cams:
        cs = ctx.cameras_from_matrices(m[None], fov, w, h, sc, off)
        c2w, intr = cs.get(0)
        x0, y0, x1, y1 = cull_rectangle(c2w, intr, lo, hi, w, h)
        assert 0 < x1 - x0 < w and 0 < y1 - y0 <= h and (x0 > 0 or x1 < w), (name, x0, y0, x1, y1)  # proper
        if name == "tile edge":
            assert (x0, y0, x1, y1) == (17, 8, 48, 41)
        ctx.score_views(api.L.SCORE_PSNR_COVERAGE, [SLOT], inside, None, opts, gt=tgt)  # the scratch image: lit everywhere
        rec, _ = ctx.score_views(api.L.SCORE_PSNR_COVERAGE, [SLOT], cs, None, opts, gt=tgt)
        img, _ = ctx.render(SLOT, cs, None, opts)
        assert rec.tobytes() == ctx.score_psnr_images(img, tgt, BG).tobytes(), name
        px = img.cpu().numpy()
        outside = np.ones((h, w), bool)
        outside[y0:y1, x0:x1] = False
        assert not px[0][outside].any() and px[0][~outside][:, 3].max() > 0.5, name  # the rectangle holds the object
        assert_psnr_record(rec[0], px[0], gt[0], BG, 1.0, oracle, name)
        cs.close()
    inside.close()
