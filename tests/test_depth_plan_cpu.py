"""CPU gate of the depth-landmark arithmetic (csrc/depth_plan.h, what csrc/depth_landmarks.hip runs one key-point slot per lane): built with g++ (ASan + UBSan)
into tests/cpp/depth_plan_pin.cpp and compared with the host functions it restates -- omni::fill_image_descriptor's lifted floats and
omni::fill_depth_landmarks with omni::CameraModel::lift -- on the seeded inputs of tests/depth_cases.py: flags, counts and the BITS of every float."""
import numpy as np
import pytest

from tests import depth_cases as D


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return D.build_pin(tmp_path_factory.mktemp("depth_plan"))


@pytest.fixture(scope="module")
def runs(omni, pin):
    cases = D.gate_cases(omni)
    return cases, D.run_pin(pin, "plan", cases), D.run_pin(pin, "host", cases)


def test_header_equals_the_host_functions_bit_for_bit(runs):
    cases, plan, host = runs
    for i, (c, a, b) in enumerate(zip(cases, plan, host)):
        print(f"case {i} ({c['lens']}): {c['n_images']} images x {c['max_num']}, count_3d header {a['count_3d'].tolist()} host {b['count_3d'].tolist()}")
        assert D.same_bits(a, b) == [], i
    assert sum(int(a["count_3d"].sum()) for a in plan) > 500                   # not vacuous


def test_gate_rounding_and_depth_window(runs):
    """the listed special points and depth values land where the specification says (case 0's image 2 is too small to see them all: case 1, image 0)"""
    cases, plan, _ = runs
    c, a = cases[1], plan[1]
    sp = {p: k for k, p in enumerate(D.SPECIAL_POINTS)}
    flag, kps, depth = a["landmarks_flag"][0], c["kps_xy"][0], c["depth"][0]

    def dep(px, py):
        return int(depth[py, px])

    def expect(px, py):
        return int(dep(px, py) / 1000.0 > D.NEAR and dep(px, py) / 1000.0 < D.FAR)
    assert flag[sp[(2.5, 3.5)]] == expect(2, 4) and flag[sp[(3.5, 2.5)]] == expect(4, 2)          # half to even, both ways
    for p in ((640.0, 10.0), (640.4, 10.0), (-0.25, 5.0), (10.0, 480.0), (10.0, 480.4), (10.0, -0.25), (639.5, 479.5)):
        assert flag[sp[p]] == 0, p                                                                  # outside this depth image, or dropped by the gate
    assert flag[sp[(638.5, 478.5)]] == expect(638, 478) and flag[sp[(0.5, 0.5)]] == expect(0, 0) and flag[sp[(639.0, 479.0)]] == expect(639, 479)
    # every listed depth value was read by some live key point, and accepted exactly when strictly inside the window
    seen = {}
    for k in range(int(c["n_kps"][0])):
        x, y = kps[k]
        if 0 <= x <= 640 and 0 <= y <= 480 and np.rint(np.float64(x)) < 640 and np.rint(np.float64(y)) < 480:
            v = dep(int(np.rint(np.float64(x))), int(np.rint(np.float64(y))))
            assert flag[k] == int(v / 1000.0 > D.NEAR and v / 1000.0 < D.FAR), (k, v)
            seen.setdefault(v, flag[k])
        else:
            assert flag[k] == 0, k
    print("depth value -> accepted:", {v: int(seen[v]) for v in D.DEPTH_VALUES})
    assert [int(seen[v]) for v in D.DEPTH_VALUES] == [0, 0, 0, 1, 1, 0, 0]


def test_accept_rule_missing_frame_and_untouched_slots(runs):
    cases, plan, _ = runs
    for c, a in zip(cases, plan):
        amin, M = c["model"].accept_min_3d_pts, c["max_num"]
        for i in range(c["n_images"]):
            n = min(max(int(c["n_kps"][i]), 0), M)
            assert not a["norm2d"][i, n:].any() and not a["landmarks_3d"][i, n:].any() and not a["landmarks_flag"][i, n:].any()
            assert int(a["count_3d"][i]) == int(a["landmarks_flag"][i].sum())
            flagged = a["landmarks_flag"][i].astype(bool)
            assert not a["landmarks_3d"][i][~flagged].any()
            if n <= amin or not c["have"][i]:
                assert a["count_3d"][i] == 0
            if n:
                assert a["norm2d"][i, :n].any()                                                      # the lifted floats are there either way
    a0 = plan[0]
    assert a0["count_3d"][1] == 0 and a0["count_3d"][2] > 0                                         # accept_min key points: nothing; one more: landmarks
    assert plan[1]["count_3d"][1] == 0 and plan[1]["count_3d"][2] > 0                               # no depth frame; a raw count above max_num runs as max_num
    assert plan[2]["count_3d"].min() > 0                                                            # the 64 x 48 depth image still gives some


def test_points_are_the_scene_points(omni, pin):
    """sanity of the chain against geometry stated independently: an ideal pinhole, a plane of constant depth -> the landmark, moved back into the camera, is
    (x_n * d, y_n * d, d)"""
    c = D.make_case(omni, "ideal", 21, 100, 640, 480, 640, [100, 100, 100], [1, 1, 1])
    c["depth"][:] = 2500
    (a,) = D.run_pin(pin, "plan", [c])
    from tests import landmark_cases as L
    ext = np.array(list(c["model"].extrinsic))
    Re, te = L.quat_R(ext[3:]), ext[:3]
    worst, n_seen = 0.0, 0
    for i in range(3):
        Rw, tw = L.quat_R(c["poses"][i, 3:]), c["poses"][i, :3]
        for k in np.flatnonzero(a["landmarks_flag"][i]):
            cam = Re.T @ (Rw.T @ (a["landmarks_3d"][i, k].astype(np.float64) - tw) - te)
            x, y = c["kps_xy"][i, k].astype(np.float64)
            want = np.array([(x - CCX) / CFX * 2.5, (y - CCY) / CFY * 2.5, 2.5])
            worst = max(worst, float(np.abs(cam - want).max()))
            n_seen += 1
    print(f"{n_seen} landmarks, largest deviation from the plane's point {worst:.2e} m")
    assert n_seen > 200 and worst < 1e-5              # float32 landmarks a few metres from the origin: ~5e-7 m per coordinate


from tests import camera_cases as _CC  # noqa: E402

CFX, CFY, CCX, CCY = _CC.intrinsics("ideal")
