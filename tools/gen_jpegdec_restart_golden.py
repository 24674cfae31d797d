"""Writes tests/golden/jpegdec_restart_cases.npz: the restart-interval files of tests/jpegdec_restart_cases.py as Pillow (libjpeg-turbo) writes them
(restart_marker_blocks / restart_marker_rows) and the gray pixels Pillow decodes them to -- for colour files Image.draft('L', size), as in
tools/gen_jpegdec_golden.py.  Restart markers do not change the pixels: files of one picture that differ in their markers alone share one pixel array.  Needs
Pillow; the tests that read the fixture do not.
    python tools/gen_jpegdec_restart_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import jpegdec_cases as J  # noqa: E402
from tests import jpegdec_restart_cases as R  # noqa: E402
from gen_jpegdec_golden import pillow_file, pillow_gray  # noqa: E402


def build() -> dict:
    out = {}
    for name, (w, h, content, save, n_int, shared) in R.SPECS.items():
        img = J.make_image(content, w, h)
        data = pillow_file(img, **save)
        out["jpg_" + name] = np.frombuffer(data, np.uint8)
        pix = pillow_gray(data)
        assert pix.shape == (h, w)
        plain = {k: v for k, v in save.items() if not k.startswith("restart_marker")}
        assert np.array_equal(pix, pillow_gray(pillow_file(img, **plain))), name                # the markers change no pixel
        key = "pix_" + (shared or name)
        assert key not in out or np.array_equal(out[key], pix), name
        out[key] = pix
        assert b"\xff\xdd" in data[:700] and len(R.markers(data)) == n_int - 1, (name, len(R.markers(data)))
    for k in range(R.CAM_FRAMES):
        plain, rows = pillow_file(R.cam_image(k), **R.CAM_SAVE[k]), pillow_file(R.cam_image(k), restart_marker_rows=1, **R.CAM_SAVE[k])
        assert np.array_equal(pillow_gray(plain), pillow_gray(rows)) and len(R.markers(rows)) == R.CAM_H // 8 - 1 and b"\xff\xdd" not in plain[:700]
        assert max(len(plain), len(rows)) <= R.CAM_W * R.CAM_H // 2
        out[f"jpg_cam_plain_{k}"], out[f"jpg_cam_rows_{k}"] = np.frombuffer(plain, np.uint8), np.frombuffer(rows, np.uint8)
    return out


if __name__ == "__main__":
    data = build()
    np.savez_compressed(R.GOLDEN, **data)
    print(f"{R.GOLDEN}: {len(R.SPECS)} files, {sum(v.size for k, v in data.items() if k.startswith('jpg_'))} file bytes, {os.path.getsize(R.GOLDEN)} bytes")
