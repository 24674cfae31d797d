"""Writes tests/golden/jpegdec_cases.npz: the JPEG files of tests/jpegdec_cases.py as Pillow (libjpeg-turbo) writes them and the gray pixels Pillow decodes them
to -- for colour files Image.draft('L', size), libjpeg's JCS_GRAYSCALE: the first component alone -- which csrc/jpeg_dec_plan.h and csrc/jpeg_dec.hip must
reproduce pixel for pixel.  Needs Pillow; the tests that read the fixture on a GPU box do not.
    python tools/gen_jpegdec_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpegdec_cases as J  # noqa: E402


def pillow_file(img: np.ndarray, **save) -> bytes:
    b = io.BytesIO()
    Image.fromarray(img, "L" if img.ndim == 2 else "RGB").save(b, "JPEG", **save)
    return b.getvalue()


def pillow_gray(data: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    if im.mode != "L":
        im.draft("L", im.size)
    im.load()
    assert im.mode == "L", im.mode
    return np.asarray(im).copy()


def build() -> dict:
    out = {}
    for name, (w, h, content, save, cls) in J.SPECS.items():
        data = pillow_file(J.make_image(content, w, h), **save)
        out["jpg_" + name] = np.frombuffer(data, np.uint8)
        pix = pillow_gray(data)
        assert pix.shape == (h, w)
        out["pix_" + name] = pix
        assert (b"\xff\xc2" in data[:700]) == (cls == J.UNSUPPORTED), name
        assert (b"\xff\xdd" in data[:700]) == (cls == J.HOST), name
    return out


if __name__ == "__main__":
    data = build()
    os.makedirs(os.path.dirname(J.GOLDEN), exist_ok=True)
    np.savez_compressed(J.GOLDEN, **data)
    print(f"{J.GOLDEN}: {len(J.SPECS)} files, {sum(v.size for k, v in data.items() if k.startswith('jpg_'))} file bytes, {os.path.getsize(J.GOLDEN)} bytes")
