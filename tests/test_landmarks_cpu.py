"""CPU gate of the stereo-landmark arithmetic (csrc/landmark_plan.h, what csrc/landmarks.hip runs one match per lane): built with g++ into
tests/cpp/landmark_plan_pin.cpp and compared with the host functions it restates -- omni::fill_image_descriptor's lifted floats, omni::fill_stereo_landmarks,
geom::stereo_landmarks -- on the seeded inputs of tests/landmark_cases.py: flags, counts and the BITS of every float.  The header takes the arg-min of the
diagonal where the host sorts the eigenvalues: equal where the smallest one is unique, so both programs count tied smallest eigenvalues and the count must be 0."""
import numpy as np
import pytest

from tests import landmark_cases as L


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return L.build_pin(tmp_path_factory.mktemp("landmark_plan"))


@pytest.fixture(scope="module")
def runs(omni, pin):
    cases = L.gate_cases(omni)
    return cases, L.run_pin(pin, "plan", cases), L.run_pin(pin, "host", cases)


def test_header_equals_the_host_functions_bit_for_bit(runs):
    cases, plan, host = runs
    for i, (c, a, b) in enumerate(zip(cases, plan, host)):
        print(f"case {i}: {c['n_pairs']} pairs x {c['max_num']}, count_3d header {a['count_3d'].tolist()} host {b['count_3d'].tolist()}, ties {int(a['ties'][0])} / {int(b['ties'][0])}")
        assert L.same_bits(a, b) == [], i
        assert int(b["ties"][0]) == 0 and int(a["ties"][0]) == 0, i          # the host code alone first: the inputs are inside what the arg-min form covers
    assert sum(int(a["count_3d"].sum()) for a in plan) > 500                   # not vacuous


def test_injected_matches_fall_on_the_expected_side(runs):
    """the injected kinds are all there and land where the geometry says: reversed disparity (behind the up camera) gives no landmark; matches moved across
    the epipolar line are kept at 1 pixel and dropped at 15 (triangle_thres = 0.006 is about 4 pixels at f = 300); most untouched ones (+- 1 pixel of noise
    per image) are kept.  Zero disparity (the point at infinity) is kept or dropped as the literal comparisons decide -- the first test holds that to the host's
    bits; here it only has to occur."""
    cases, plan, _ = runs
    kept = {k: [0, 0] for k in L.KINDS}
    by_offset = {}
    for c, a in zip(cases, plan):
        P = c["n_pairs"]
        for p in range(P):
            if c["n_kps"][p] <= c["model"].accept_min_3d_pts:
                continue
            for i in range(int(c["n_matches"][p])):
                k = int(c["kind"][p, i])
                if k < 0:
                    continue
                f = int(a["landmarks_flag"][p, c["match_up"][p, i]])
                assert f == int(a["landmarks_flag"][P + p, c["match_down"][p, i]])
                kept[L.KINDS[k]][f] += 1
                if k == 3:
                    by_offset.setdefault(int(c["offset"][p, i]), [0, 0])[f] += 1
    print("dropped / kept per kind:", kept, "per offset in pixels:", dict(sorted(by_offset.items())))
    assert kept["good"][1] > 300 and kept["good"][1] > 4 * kept["good"][0]
    assert sum(kept["infinity"]) > 20 and kept["behind"][0] > 20 and kept["behind"][1] == 0
    assert kept["offset"][0] > 20 and kept["offset"][1] > 20                  # residuals on both sides of triangle_thres
    assert by_offset[1][1] > 0 and by_offset[15][1] == 0


def test_accept_rule_and_untouched_entries(runs):
    """nothing unless the up image has MORE than accept_min_3d_pts key points (its lifted points are still there); zeros behind the last key point; a landmark
    exactly where the flag is set; indices outside the images never written through"""
    cases, plan, _ = runs
    at_min = above_min = 0
    for c, a in zip(cases, plan):
        P, M, amin = c["n_pairs"], c["max_num"], c["model"].accept_min_3d_pts
        for img in range(2 * P):
            n = int(c["n_kps"][img])
            assert not a["norm2d"][img, n:].any() and not a["landmarks_3d"][img, n:].any() and not a["landmarks_flag"][img, n:].any()
            ref = np.stack([(c["kps_xy"][img, :n, 0].astype(np.float64) - L.CX) / L.FX, (c["kps_xy"][img, :n, 1].astype(np.float64) - L.CY) / L.FY], 1).astype(np.float32)
            assert np.array_equal(a["norm2d"][img, :n], ref)
            flagged = a["landmarks_flag"][img].astype(bool)
            assert not a["landmarks_3d"][img][~flagged].any() and np.abs(a["landmarks_3d"][img][flagged]).sum(1).all()
        for p in range(P):
            assert int(a["count_3d"][p]) == int(a["landmarks_flag"][p].sum()) == int(a["landmarks_flag"][P + p].sum())
            if c["n_kps"][p] == amin and c["n_matches"][p] > 0:
                at_min += 1
                assert a["count_3d"][p] == 0
            if c["n_kps"][p] == amin + 1 and c["n_matches"][p] > 0:
                above_min += int(a["count_3d"][p] > 0)
    assert at_min >= 3 and above_min >= 2


def test_points_are_the_scene_points(omni, pin):
    """sanity of the whole chain against the generator's geometry: kept landmarks of untouched matches, moved into the up camera, project to the up pixel"""
    c = L.make_case(omni, 11, 4, 2, 100, 3, [(100, 100)] * 8, [100] * 8)
    (a,) = L.run_pin(pin, "plan", [c])
    up7, _ = L.rig(4)
    worst = 0.0
    for p in range(8):
        pose = c["poses"][p // 4]
        Rw, tw = L.quat_R(pose[3:]), pose[:3]
        Rc, tc = L.quat_R(up7[p % 4, 3:]), up7[p % 4, :3]
        for i in range(100):
            iu = c["match_up"][p, i]
            if c["kind"][p, i] != 0 or not a["landmarks_flag"][p, iu]:
                continue
            cam = Rc.T @ (Rw.T @ (a["landmarks_3d"][p, iu].astype(np.float64) - tw) - tc)
            px = np.array([cam[0] / cam[2] * L.FX + L.CX, cam[1] / cam[2] * L.FY + L.CY])
            worst = max(worst, float(np.abs(px - c["kps_xy"][p, iu]).max()))
            assert cam[2] > 0.5
    print(f"largest reprojection error of a kept landmark in its up image: {worst:.2f} pixels")
    assert worst < 3.0            # +- 1 pixel of noise per image, shared between the two views by the least-squares point
