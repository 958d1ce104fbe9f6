"""Depth images without a GPU: the C ABI's new entry point is declared, exported and bound; api.write_image_depth's
byte rule; the flag-file server routes `--screenshot_depth` to the depth render (a stub context stands in for the GPU)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_depth_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prv.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+prv_render_depth\s*\(([^;]*)\)\s*;", text)
    assert m, "prv_render_depth is not declared in prv.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert n_args == 9
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "nerf_prv_amd", "libprv_hip.so")], text=True)
    assert "prv_render_depth" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    from nerf_prv_amd import _lib

    res, args = _lib.SIGNATURES["prv_render_depth"]
    assert len(args) == n_args
    assert _lib.load().prv_render_depth.argtypes is not None


def test_render_mode_names():
    from nerf_prv_amd import api

    assert int(api.RenderMode.Shade) == 0 and int(api.RenderMode.Depth) == 1
    assert api.Depth is api.RenderMode.Depth and api.Shade is api.RenderMode.Shade


def _read16(path):
    from PIL import Image

    im = Image.open(path)
    assert im.mode == "I;16"
    return np.asarray(im).astype(np.int64)


def test_write_image_depth_known_answers(tmp_path):
    from nerf_prv_amd import api

    scale = 0.25
    # z in engine units -> round(z / scale * 1000) millimetres of the dataset unit
    z = np.array([[0.0, 0.25, 0.5, 1.0],
                  [0.0000625, 0.0001875, 0.000125, -0.1],  # .5 cases: 0.25 -> 0, 0.75 -> 1, 0.5 -> 0 (halves to even)
                  [16.38375, 16.4, 100.0, 0.001]],  # 65535 exactly, then clipped; 4
                 np.float32)
    img = np.zeros(z.shape + (4,), np.float32)
    img[..., 0] = z
    img[..., 1] = 7.0  # channels other than 0 are ignored
    img[..., 2] = -3.0
    img[..., 3] = 0.5
    p = str(tmp_path / "d.png")
    api.write_image_depth(p, img, scale)
    got = _read16(p)
    want = np.clip(np.round(z.astype(np.float64) / scale * 1000.0), 0, 65535).astype(np.int64)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[0], [0, 1000, 2000, 4000])
    assert got[1, 3] == 0 and got[2, 1] == 65535 and got[2, 2] == 65535 and got[2, 3] == 4
    assert got[2, 0] == 65535
    # exact halves (values chosen exact in binary): 2.5 -> 2, 3.5 -> 4
    api.write_image_depth(p, np.array([[2.5, 3.5, 0.5, 1.5]], np.float64) / 1000.0, 1.0)
    np.testing.assert_array_equal(_read16(p), [[2, 4, 0, 2]])
    # a 2-D image is the depth itself
    api.write_image_depth(p, np.array([[0.1, 0.2]], np.float32), 0.1)
    np.testing.assert_array_equal(_read16(p), [[1000, 2000]])


class _StubCams:
    closed = False

    def close(self):
        self.closed = True


class _StubCtx:
    """cameras_from_json + render_depth / render_rgba8 on CPU tensors"""

    def __init__(self, n, h, w):
        import torch

        self.torch = torch
        self.n, self.h, self.w = n, h, w
        self.depth_calls, self.rgba8_calls = [], []
        self.depth = torch.arange(n * h * w, dtype=torch.float32).reshape(n, h, w) * 0.01

    def cameras_from_json(self, path):
        return _StubCams()

    def render_depth(self, slot, cams, view_ids, opts, out=None, out_depth=None, want_stats=True):
        self.depth_calls.append((slot, opts.width, opts.height, opts.spp))
        return self.torch.zeros((self.n, self.h, self.w, 4)), self.depth.clone(), None

    def render_rgba8(self, slot, cams, view_ids, opts, out=None, want_stats=True):
        self.rgba8_calls.append(slot)
        return self.torch.zeros((self.n, self.h, self.w, 4), dtype=self.torch.uint8), None


def _request(tmp_path, flags):
    frames = [{"file_path": "./images/view_0"}, {"file_path": "./images/view_1.png"}, {"file_path": "view_2"}]
    tj = tmp_path / "shots.json"
    tj.write_text(json.dumps({"w": 5, "h": 3, "scale": 0.5, "frames": frames}))
    line = f"os.system('python run.py --screenshot_transforms {tj} --screenshot_dir {tmp_path / 'out'} {flags}')"
    return line


@pytest.mark.parametrize("depth", [True, False])
def test_server_routes_screenshot_depth(tmp_path, depth):
    from nerf_prv_amd import api, compat_server

    line = _request(tmp_path, "--screenshot_depth --n_steps 0" if depth else "--n_steps 0")
    args = compat_server.parse_command(line)
    assert ("screenshot_depth" in args["flags"]) == depth
    ctx = _StubCtx(3, 3, 5)
    srv = compat_server.CompatServer(str(tmp_path), ctx, load_model=lambda scene, c: 7, screenshot_spp=4)
    if depth:
        srv.serve_one(args)
        assert ctx.depth_calls == [(7, 5, 3, 4)] and ctx.rgba8_calls == []
        names = sorted(os.listdir(tmp_path / "out"))
        assert names == ["view_0.png", "view_1.png", "view_2.png"]
        for i, name in enumerate(["view_0.png", "view_1.png", "view_2.png"]):
            got = _read16(str(tmp_path / "out" / name))
            want = np.clip(np.round(ctx.depth[i].numpy().astype(np.float64) / 0.5 * 1000.0), 0, 65535)
            np.testing.assert_array_equal(got, want)
            ref = str(tmp_path / "ref.png")
            api.write_image_depth(ref, ctx.depth[i].numpy(), 0.5)
            np.testing.assert_array_equal(got, _read16(ref))
    else:
        srv.serve_one(args)
        assert ctx.depth_calls == [] and ctx.rgba8_calls == [7]
        from PIL import Image

        assert Image.open(str(tmp_path / "out" / "view_0.png")).mode == "RGBA"
