"""Writes tests/golden/jpeg_cases.npz: the small input images of tests/jpeg_cases.py and Pillow's (libjpeg-turbo) complete files for them at every quality --
what csrc/jpeg_plan.h and csrc/jpeg.hip must reproduce byte for byte.  Needs Pillow; the tests that read the fixture on a GPU box do not.
    python tools/gen_jpeg_golden.py
Checked while generating (and asserted again by tests/test_jpeg_plan_cpu.py): at least one file's scan holds a stuffed FF 00 pair and one a ZRL symbol."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpeg_cases as J  # noqa: E402


def pillow_file(gray: np.ndarray, quality: int) -> bytes:
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(gray, np.uint8), "L").save(b, "JPEG", quality=quality)      # Pillow's defaults: baseline, JDCT_ISLOW, standard tables
    return b.getvalue()


def build() -> dict:
    out = {}
    for name, imgs in J.image_sets().items():
        assert imgs.shape[1] <= 48 and imgs.shape[2] <= 64
        out["img_" + name] = imgs
        for q in J.QUALITIES:
            for i, g in enumerate(imgs):
                out[f"jpg_{name}_q{q}_{i}"] = np.frombuffer(pillow_file(g, q), np.uint8)
    return out


if __name__ == "__main__":
    data = build()
    stuffed = zrl = 0
    for k, v in data.items():
        if k.startswith("jpg_"):
            h, w = data["img_" + k[4:k.rindex("_q")]].shape[1:]
            syms, st = J.scan_symbols(v.tobytes(), w, h)
            stuffed += st > 0
            zrl += 0xF0 in syms
    assert stuffed > 0 and zrl > 0, (stuffed, zrl)
    os.makedirs(os.path.dirname(J.GOLDEN), exist_ok=True)
    np.savez_compressed(J.GOLDEN, **data)
    print(f"{J.GOLDEN}: {sum(k.startswith('img_') for k in data)} image sets, {sum(k.startswith('jpg_') for k in data)} files, "
          f"{stuffed} with a stuffed FF 00, {zrl} with ZRL, {os.path.getsize(J.GOLDEN)} bytes")
