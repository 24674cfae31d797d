"""CPU gate of the lens model (csrc/camera_plan.h: camodocal's PINHOLE with distortion and MEI, what csrc/landmarks.hip lifts with one key point per lane) built
with g++ into tests/cpp/camera_plan_pin.cpp -- once plainly and once under -fsanitize=address,undefined:

  1  the build's lift equals a Python restatement of the specification (tests/camera_cases.py lift_py: float64 scalars, the same expressions, math.sqrt),
     BIT FOR BIT, over a pixel grid and over the gate cases' key points, for every camera;
  2  `zero` (a model whose coefficients are 0) and `ideal` give the bits of the earlier lm::lift and of landmark_plan_pin's `plan` mode on the seven gate cases;
  3  project(lift(pixel)) returns the pixel: within 1e-4 px for `mild` and `mei` (the formula points the right way; rounding is ~1e-6); for `euroc` the eight
     rounds do not converge at the picture's border -- the figure is printed, not bounded;
  4  the host functions with the model's lift (fill_image_descriptor + fill_stereo_landmarks) equal landmarks_host with the camera, bit for bit.  Conditions on
     the CPU build: every camera's cases keep and drop matches, no tied eigenvalue, no NaN, every lifted float finite.  Landmarks: landmark_cases' zero-disparity
     matches (kind "infinity") triangulate to +-inf in its four-direction cases under the ideal pinhole already; those key points, and only those, may hold inf
     here too (compared by their bits like everything else);
  5  a camera whose rounds diverge: flags, counts, isnan / isinf masks and every finite value's bits equal;
  6  the camodocal file reader, the scaling rule, Config's refusals;
  7  the new symbols are exported, the ABI version and sizeof(omni_stereo_model) are unchanged.
camodocal itself is not vendored: parity with it is UNPINNED (the header says so)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import camera_cases as K
from tests import landmark_cases as L

ALL = ("ideal", "zero", "mild", "barrel", "euroc", "mei")


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return K.build_pin(tmp_path_factory.mktemp("camera_plan"))


@pytest.fixture(scope="module")
def pin_san(tmp_path_factory):
    return K.build_pin(tmp_path_factory.mktemp("camera_plan_san"), sanitize=True)


def grid(step=4.0):
    """pixels over landmark_cases' range, every other row shifted by a quarter pixel (key points are whole pixels; the lift takes any float)"""
    x0, x1, y0, y1 = K.PIXEL_RANGE
    xs, ys = np.meshgrid(np.arange(x0, x1 + 1, step), np.arange(y0, y1 + 1, step))
    xs = xs + 0.25 * (np.arange(xs.shape[0])[:, None] % 2)
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)


@pytest.fixture(scope="module")
def runs(omni, pin):
    """per gated camera: the seven cases, the header's output, the host functions' output -- computed once"""
    out = {}
    for name in K.GATED:
        cases = K.gate_cases(omni, name)
        out[name] = (cases, K.run_pin(pin, "plan", cases), K.run_pin(pin, "host", cases))
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", ALL)
def test_lift_equals_the_python_restatement_bit_for_bit(omni, pin, name):
    pts = grid()
    kps = np.concatenate([c["kps_xy"][i, :int(c["n_kps"][i])] for c in K.gate_cases(omni, name) for i in range(c["kps_xy"].shape[0])])
    pts = np.concatenate([pts, kps[::3]])
    got = K.run_points(pin, "lift", name, pts, omni)
    ref = np.array([K.lift_py(name, x, y) for x, y in pts], np.float64)
    differ = int((bits(got) != bits(ref)).any(1).sum())
    print(f"{name}: {len(pts)} pixels ({len(kps[::3])} key points of the gate cases), {differ} differ from the restatement; all finite: {bool(np.isfinite(got).all())}")
    assert np.isfinite(got).all()
    assert differ == 0


def test_zero_and_ideal_have_the_bits_of_the_earlier_lift(omni, pin):
    pts = grid(2.0)
    old = K.run_points(pin, "lmlift", "ideal", pts, omni)
    ref = np.stack([(pts[:, 0].astype(np.float64) - L.CX) / L.FX, (pts[:, 1].astype(np.float64) - L.CY) / L.FY], 1)
    assert np.array_equal(bits(old), bits(ref))
    for name in ("ideal", "zero"):
        assert np.array_equal(bits(K.run_points(pin, "lift", name, pts, omni)), bits(old)), name
    # ... and the whole stage: landmark_plan_pin's `plan` mode (the earlier signatures) on the seven gate cases
    cases = L.gate_cases(omni)
    old_plan = L.run_pin(L.build_pin(os.path.dirname(pin)), "plan", cases)
    for name in ("ideal", "zero"):
        mine = K.gate_cases(omni, name)
        assert all(np.array_equal(a["kps_xy"], b["kps_xy"]) for a, b in zip(cases, mine))
        for mode in ("plan", "host"):
            for i, (a, b) in enumerate(zip(K.run_pin(pin, mode, mine), old_plan)):
                assert L.same_bits(a, b) == [] and int(a["ties"][0]) == int(b["ties"][0]) == 0, (name, mode, i)


@pytest.mark.parametrize("name", ("mild", "mei", "euroc"))
def test_project_of_lift_returns_the_pixel(omni, pin, name):
    """the restatement points the right way: the forward model undoes the lift.  `mild` and `mei` to 1e-4 px (rounding alone is ~1e-6: the bound checks the
    formula).  `euroc`: the eight rounds have not converged at the border -- measured 0.083 px at worst over the range; printed, not bounded."""
    pts = grid()
    rays = K.run_points(pin, "lift", name, pts, omni)
    back = K.run_points(pin, "project", name, np.concatenate([rays, np.ones((len(rays), 1))], 1), omni)
    err = np.abs(back - pts.astype(np.float64)).max(1)
    print(f"{name}: project(lift(pixel)) - pixel over {len(pts)} pixels: worst {err.max():.3g} px, median {np.median(err):.3g} px")
    assert np.isfinite(back).all()
    assert np.allclose(back, K.project_np(name, np.concatenate([rays, np.ones((len(rays), 1))], 1)), rtol=0, atol=1e-9)      # the numpy forward model the cases are made with
    if name != "euroc":
        assert err.max() < 1e-4


@pytest.mark.parametrize("name", K.GATED)
def test_host_functions_with_the_models_lift_equal_the_header(runs, name):
    cases, plan, host = runs[name]
    kept = dropped = 0
    for i, (c, a, b) in enumerate(zip(cases, plan, host)):
        print(f"{name} case {i}: {c['n_pairs']} pairs x {c['max_num']}, count_3d header {a['count_3d'].tolist()} host {b['count_3d'].tolist()}, ties {int(a['ties'][0])} / {int(b['ties'][0])}")
        # the conditions, on the CPU build alone: finite outputs, no tied eigenvalue
        # (non-finite output: none in the lifted floats; no NaN anywhere; among the landmarks only the +-inf that landmark_cases' zero-disparity matches -- its
        # kind "infinity", parallel rays -- give under the ideal pinhole too, at exactly those key points)
        assert np.isfinite(b["norm2d"]).all() and not np.isnan(b["landmarks_3d"]).any(), i
        assert not (~np.isfinite(b["landmarks_3d"]).all(-1) & ~K.infinity_keypoints(c)).any(), i
        assert int(b["ties"][0]) == 0 and int(a["ties"][0]) == 0, i
        assert L.same_bits(a, b) == [], i
        live = sum(int(c["n_matches"][p]) for p in range(c["n_pairs"]) if c["n_kps"][p] > c["model"].accept_min_3d_pts)
        kept += int(b["count_3d"].sum())
        dropped += live - int(b["count_3d"].sum())
    print(f"{name}: kept {kept}, dropped {dropped}")
    assert kept >= 1 and dropped >= 1
    # the lifted floats differ from the ideal pinhole's: the camera is in the path
    ideal = np.stack([(cases[3]["kps_xy"][..., 0].astype(np.float64) - cases[3]["model"].cx) / cases[3]["model"].fx,
                      (cases[3]["kps_xy"][..., 1].astype(np.float64) - cases[3]["model"].cy) / cases[3]["model"].fy], -1).astype(np.float32)
    n0 = int(cases[3]["n_kps"][0])
    assert not np.array_equal(plan[3]["norm2d"][0, :n0], ideal[0, :n0])


@pytest.mark.parametrize("name", ("mild", "mei"))
def test_good_matches_stay_good_under_the_camera(runs, name):
    """the cases are true under their camera: untouched matches are mostly kept, reversed disparity never"""
    cases, plan, _ = runs[name]
    kept = {k: [0, 0] for k in L.KINDS}
    for c, a in zip(cases, plan):
        for p in range(c["n_pairs"]):
            if c["n_kps"][p] <= c["model"].accept_min_3d_pts:
                continue
            for i in range(int(c["n_matches"][p])):
                k = int(c["kind"][p, i])
                if k >= 0:
                    kept[L.KINDS[k]][int(a["landmarks_flag"][p, c["match_up"][p, i]])] += 1
    print(name, "dropped / kept per kind:", kept)
    assert kept["good"][1] > 300 and kept["good"][1] > 4 * kept["good"][0]
    assert kept["behind"][0] > 20 and kept["behind"][1] == 0


def test_a_camera_that_diverges(omni, pin):
    bad, n_grid = K.diverging_pixels(pin)
    print(f"the diverging camera's lift is not finite at {len(bad)} of {n_grid} grid pixels")
    cases = K.diverging_cases(omni, pin)
    plan, host = K.run_pin(pin, "plan", cases), K.run_pin(pin, "host", cases)
    for i, (a, b) in enumerate(zip(plan, host)):
        nonfinite = int((~np.isfinite(a["norm2d"])).sum())
        print(f"case {i}: {nonfinite} non-finite lifted floats, {int((~np.isfinite(a['landmarks_3d'])).sum())} non-finite landmark floats, count_3d {a['count_3d'].tolist()}")
        assert nonfinite > 20                                                     # not vacuous: inf / NaN do flow through the stage
        assert K.same_where_finite(a, b) == [], i
    assert sum(int(a["count_3d"].sum()) for a in plan) > 50


def test_the_sanitized_build_agrees_and_runs_clean(omni, pin, pin_san, runs):
    """-fsanitize=address,undefined on the stand-alone program: lifts, whole stages on both paths (one gate shape per camera and the diverging camera), the
    file reader and the Config checks -- the same bytes as the plain build, nothing reported"""
    pts = grid(8.0)
    for name in ALL:
        assert np.array_equal(bits(K.run_points(pin_san, "lift", name, pts, omni)), bits(K.run_points(pin, "lift", name, pts, omni)))
    for name in K.GATED:
        cases, plan, host = runs[name]
        for mode, ref in (("plan", plan), ("host", host)):
            (a,) = K.run_pin(pin_san, mode, [cases[6]])
            assert L.same_bits(a, ref[6]) == []
    div = K.diverging_cases(omni, pin)[:1]
    assert K.same_where_finite(K.run_pin(pin_san, "plan", div)[0], K.run_pin(pin_san, "host", div)[0]) == []
    r = subprocess.run([pin_san, "config"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.stdout, r.stderr[-3000:])
    r = subprocess.run([pin_san, "yaml", "400", "208"], input=PINHOLE_YAML, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stdout.startswith("ERROR") and r.stderr == "", (r.stdout, r.stderr[-3000:])


# ---- the camodocal file --------------------------------------------------------------------------------------------------------------------------------------
PINHOLE_YAML = """%YAML:1.0
---
model_type: PINHOLE
camera_name: camera
image_width: 640
image_height: 480
distortion_parameters:
   k1: -2.917e-01
   k2: 8.228e-02
   p1: 5.333e-05
   p2: -1.578e-04
projection_parameters:
   fx: 4.616e+02
   fy: 4.603e+02
   cx: 3.630e+02
   cy: 2.481e+02
"""
MEI_YAML = """%YAML:1.0
---
model_type: MEI
camera_name: cam0    # the up camera
image_width: 1280
image_height: 1024
mirror_parameters:
   xi: 1.2
distortion_parameters: {k1: -0.05, k2: 0.01, p1: 1e-3, p2: -1e-3}
projection_parameters:
   gamma1: 620.0
   gamma2: 621.5
   u0: 640.25
   v0: 511.75
"""


def yaml_line(pin, text, w, h):
    r = subprocess.run([pin, "yaml", str(w), str(h)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


def parse(line):
    model, file_k, size, cfg_k = (part.split() for part in line.split("|"))
    return [int(model[0])] + [float(v) for v in model[1:]], [float(v) for v in file_k], [int(v) for v in size], [float(v) for v in cfg_k]


def test_camodocal_file_reader_and_the_scaling_rule(pin):
    model, file_k, size, cfg_k = parse(yaml_line(pin, PINHOLE_YAML, 640, 480))
    assert model == [0, -0.2917, 0.08228, 5.333e-05, -1.578e-04, 0.0] and file_k == [461.6, 460.3, 363.0, 248.1] and size == [640, 480]
    assert cfg_k == file_k                                                       # the networks' size is the file's: as it is
    # networks of another size: fx cx by width / image_width, fy cy by height / image_height; the coefficients stay
    model2, file_k2, _, cfg_k2 = parse(yaml_line(pin, PINHOLE_YAML, 400, 208))
    assert model2 == model and file_k2 == file_k
    assert cfg_k2 == [461.6 * (400 / 640), 460.3 * (208 / 480), 363.0 * (400 / 640), 248.1 * (208 / 480)]
    model, file_k, size, cfg_k = parse(yaml_line(pin, MEI_YAML, 1280, 1024))
    assert model == [1, -0.05, 0.01, 1e-3, -1e-3, 1.2] and file_k == cfg_k == [620.0, 621.5, 640.25, 511.75] and size == [1280, 1024]
    # refused by name; a missing entry is named; MEI needs its mirror parameter
    for other in ("KANNALA_BRANDT", "SCARAMUZZA"):
        line = yaml_line(pin, PINHOLE_YAML.replace("PINHOLE", other), 640, 480)
        assert line.startswith("ERROR") and other in line and "not supported" in line
    assert "no distortion_parameters.k2" in yaml_line(pin, PINHOLE_YAML.replace("   k2: 8.228e-02\n", ""), 640, 480)
    assert "no mirror_parameters.xi" in yaml_line(pin, MEI_YAML.replace("   xi: 1.2\n", ""), 1280, 1024)
    assert "xi > 0" in yaml_line(pin, MEI_YAML.replace("xi: 1.2", "xi: 0.0"), 1280, 1024)
    assert "not a number" in yaml_line(pin, PINHOLE_YAML.replace("-2.917e-01", "abc"), 640, 480)


def test_config_refusals(pin):
    r = subprocess.run([pin, "config"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.stdout, r.stderr)


def test_python_reads_the_same_file(omni):
    from omni_swarm_amd import pipeline
    got = pipeline.camera_from_yaml(MEI_YAML, 640, 512)
    assert got["type"] == "MEI" and got["xi"] == 1.2 and got["k1"] == -0.05 and got["p2"] == -1e-3
    assert got["intrinsics"] == [310.0, 310.75, 320.125, 255.875] and got["image_size"] == (1280, 1024)
    with pytest.raises(omni.capi.OmniError, match="KANNALA_BRANDT"):
        pipeline.camera_from_yaml(PINHOLE_YAML.replace("PINHOLE", "KANNALA_BRANDT"))


# ---- the boundaries ------------------------------------------------------------------------------------------------------------------------------------------
NEW = {"omni_landmarks_enqueue_dev_camera", "omni_cam_set_camera_model", "omni_camera_lift_host", "omni_camera_project_host"}


def test_new_symbols_are_exported_and_the_abi_is_unchanged(omni):
    c = omni.capi
    Lb = c.lib()
    hdr = open(os.path.join(L.ROOT, "include", "omni_hip.h")).read()
    assert NEW <= set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", hdr)) and NEW <= set(c.SYMBOLS) and all(hasattr(Lb, s) for s in NEW)
    assert "#define OMNI_ABI_VERSION 2 " in hdr and Lb.omni_abi_version() == 2 and c.ABI_VERSION == 2
    assert ctypes.sizeof(c.StereoModel) == 5 * 8 + 2 * 4 + 2 * c.STEREO_MAX_DIRS * 7 * 8                  # as before: the lens is a struct of its own
    assert ctypes.sizeof(c.CameraModel) == 8 + 5 * 8
    assert "typedef struct omni_camera_model { int type; double k1, k2, p1, p2, xi; } omni_camera_model;" in hdr
    assert (c.CAMERA_PINHOLE, c.CAMERA_MEI) == (0, 1) and "#define OMNI_CAMERA_PINHOLE 0" in hdr and "#define OMNI_CAMERA_MEI 1" in hdr


def test_camera_host_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(L.ROOT, "include", "omni_host_camera.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", "-I", os.path.join(L.ROOT, "include"), hdr_path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(L.ROOT, "omni-swarm_amd", "lib", "libomni_host_camera.so")
    assert os.path.exists(lib), "libomni_host_camera.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    from omni_swarm_amd import pipeline
    assert set(pipeline.CAMERA_SYMBOLS) == declared
    Lc = pipeline.camera_lib()
    assert Lc.omni_pipeline_set_camera_model(None, None, None) == 1 and b"null pipeline" in Lc.omni_camera_last_error()


def test_the_lens_arithmetic_is_stated_once():
    """camera_plan.h is plain C++ for both compilers; landmark_plan.h, the kernel and the host path only call it"""
    pkg = os.path.join(L.ROOT, "omni-swarm_amd")
    plan = open(os.path.join(pkg, "csrc", "camera_plan.h")).read()
    code = re.sub(r"//.*", "", plan)
    for word in ("hip/", "common.h", "std::", "<vector>", "<functional>", "<algorithm>"):
        assert word not in code, word
    assert "#pragma clang fp contract(off)" in plan and "UNPINNED" in plan
    for f in (os.path.join("csrc", "landmark_plan.h"), os.path.join("csrc", "landmarks.hip"), os.path.join("host", "camera_model.hpp"), os.path.join("host", "keyframe_pipeline.hpp")):
        text = re.sub(r"//.*", "", open(os.path.join(pkg, f)).read())
        assert "rho2" not in text and "k1 *" not in text, f
