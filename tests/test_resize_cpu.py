"""CPU checks of the resize spec (csrc/resize_plan.h; OpenCV 3.4's INTER_LINEAR resize of a CV_8UC1 image restated, parity with OpenCV itself unpinned):
(1) the numpy restatement tests/resize_ref.py against torch's float64 bilinear interpolation (align_corners=False, the same source coordinates) -- every pixel
within 1 grey level: the fixed-point path rounds coefficients to 1/2048 and drops bits twice, the restatement alone measured 0.79; the area-2x mode against the
rounded 2 x 2 mean, the copy mode against identity; (2) the plan header, compiled with g++ into tests/cpp/resize_plan_pin.cpp: mode and all four tables equal the
restatement's, for every source size 2..160 against the destination sizes {8, 64, 96, 128} on both axes and for the size pairs of the camera formats, and the bytes
the pin program computes from those tables equal the restatement's images."""
import os
import subprocess

import numpy as np
import pytest

from omni_swarm_amd import synth
from tests import resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (w, h) -> (W, H): the camera formats at the networks' size, small odd shapes, an upscale whose borders clamp on both sides, the exact 2x
PAIRS = [((752, 480), (600, 480)), ((640, 480), (600, 480)), ((1280, 720), (600, 480)), ((750, 600), (600, 480)), ((95, 61), (64, 48)), ((37, 29), (96, 64)),
         ((128, 96), (64, 48)), ((188, 120), (128, 96)), ((130, 96), (128, 96))]
DST = (8, 64, 96, 128)


image = R.edge_frame


@pytest.mark.parametrize("src,dst", PAIRS)
def test_restatement_against_float64_bilinear(src, dst):
    import torch
    import torch.nn.functional as F
    (w, h), (W, H) = src, dst
    g = image(11, h, w)
    got = R.resize(g, W, H).astype(np.float64)
    if R.plan(w, h, W, H)["mode"] == R.AREA2:
        s = g.astype(np.int64)
        ref = np.floor((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]) / 4.0 + 0.5)
        assert np.array_equal(got, ref)
        return
    ref = F.interpolate(torch.from_numpy(g.astype(np.float64))[None, None], size=(H, W), mode="bilinear", align_corners=False)[0, 0].numpy()
    err = np.abs(got - ref).max()
    print(f"{w}x{h} -> {W}x{H}: max |restatement - float64 bilinear| = {err:.3f} grey levels")
    assert err <= 1.0


def test_copy_is_identity():
    g = image(12, 48, 64)
    assert R.plan(64, 48, 64, 48)["mode"] == R.COPY and np.array_equal(R.resize(g, 64, 48), g)
    # one axis 1:1 and the other not: linear, and the 1:1 axis still copies (its coefficients are (2048, 0) at every index)
    p = R.plan(64, 61, 64, 48)
    assert p["mode"] == R.LINEAR and np.array_equal(p["xofs"], np.arange(64)) and (p["ialpha"] == (2048, 0)).all()


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resize_plan") / "resize_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "resize_plan_pin.cpp")])
    return exe


def test_plan_header_equals_the_restatement(pin):
    cases = [(n, n, d, d) for n in range(2, 161) for d in DST] + [(w, h, W, H) for (w, h), (W, H) in PAIRS] + [(64, 48, 64, 48), (16, 200, 8, 100)]
    raw = subprocess.run([pin, "plans"], input="".join("%d %d %d %d\n" % c for c in cases).encode(), capture_output=True, check=True).stdout
    at, seen = 0, {"lo": 0, "hi": 0, R.COPY: 0, R.AREA2: 0, R.LINEAR: 0}
    for (w, h, W, H) in cases:
        def take(dtype, n):
            nonlocal at
            a = np.frombuffer(raw, dtype, n, at)
            at += a.nbytes
            return a
        mode, xofs, ialpha, yofs, ibeta = int(take(np.int32, 1)[0]), take(np.int32, W), take(np.int16, 2 * W).reshape(W, 2), take(np.int32, H), take(np.int16, 2 * H).reshape(H, 2)
        p = R.plan(w, h, W, H)
        assert mode == p["mode"], (w, h, W, H)
        for n, a in (("xofs", xofs), ("ialpha", ialpha), ("yofs", yofs), ("ibeta", ibeta)):
            assert np.array_equal(a, p[n]), (w, h, W, H, n)
        assert xofs.min() >= 0 and xofs.max() <= w - 1 and (ialpha.astype(int).sum(1) == 2048).all() and (ibeta.astype(int).sum(1) == 2048).all()
        seen[mode] += 1
        # the first / last destination column clamps: the source coordinate falls outside the row and the tap gets the whole weight
        seen["lo"] += int((0.5 * w / W - 0.5) < 0 and tuple(ialpha[0]) == (2048, 0) and xofs[0] == 0 and mode == R.LINEAR)
        seen["hi"] += int(((W - 0.5) * w / W - 0.5) >= w - 1 and tuple(ialpha[-1]) == (2048, 0) and xofs[-1] == w - 1 and mode == R.LINEAR)
    assert at == len(raw)
    assert seen["lo"] > 100 and seen["hi"] > 100 and seen[R.COPY] >= 5 and seen[R.AREA2] >= 4 and seen[R.LINEAR] > 600, seen


@pytest.mark.parametrize("src,dst", [((95, 61), (64, 48)), ((37, 29), (96, 64)), ((128, 96), (64, 48)), ((64, 48), (64, 48)), ((130, 96), (128, 96))])
def test_bytes_from_the_plans_tables_equal_the_restatement(pin, src, dst):
    (w, h), (W, H) = src, dst
    g = image(13, h, w)
    out = subprocess.run([pin, "resize", str(w), str(h), str(W), str(H)], input=g.tobytes(), capture_output=True, check=True).stdout
    assert np.array_equal(np.frombuffer(out, np.uint8).reshape(H, W), R.resize(g, W, H))
