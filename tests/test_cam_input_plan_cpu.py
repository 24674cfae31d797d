"""Where a key-frame unit's input bytes go, without a GPU: csrc/cam_input.h's plan() as a g++ program of its own under -fsanitize=address,undefined
(tests/cpp/cam_input_pin.cpp) against an independent restatement of the rules in Python, every field of every plan, over a grid of all ten omni_cam_enqueue_*
entries' arrival forms: cams 1 and 2 where the form allows, 1 and 3 key frames, source frames 40 x 24 with stride 40 and 48, networks 16 x 8 (network-size forms:
stride 16 and 20), 1 and 2 directions for fisheye, host parts [3] and [2, 1], files with and without a resize.

The step-order properties hold for every form but one: omni_cam_enqueue_dev has no FENCE.  It has none today -- nothing of it runs in front of the networks, and a
FENCE would make its MobileNetVLAD stream wait for its SuperPoint stream, which no caller of it sees today -- so its step list is pinned as [UNIT] alone."""
import itertools
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")

DEV, HOST, FILES = 0, 1, 2                                         # csrc/cam_input.h FORM_*
NONE, FLATTEN, RESIZE = 0, 1, 2                                    # PRE_*
CALLER, GRAY, RAW = 0, 1, 2                                        # AT_*
UPLOAD, DECODE_ALL, STATUS_DOWN, PRE, FENCE, UNIT = range(6)
W, H, SW, SH, N_CAP = 16, 8, 40, 24, 8


def case(entry, form, pre, cams, frames, stride, dirs=1, parts=None, mask=1, src=None):
    """parts: per camera the frames of each part (None: the entry hands over one buffer per camera).  mask = 1 everywhere: the plan, not the entry, must take it
    off the resize and plain file paths"""
    sw, sh = src or ((W, H) if pre == NONE else (SW, SH))
    return dict(entry=entry, form=form, pre=pre, cams=cams, n=frames * dirs, W=W, H=H, n_cap=N_CAP, src_w=(sw, sw), src_h=(sh, sh), stride=stride, frames=frames,
                first_view=1 if pre == FLATTEN else 0, dirs=dirs, mask=mask, parts=parts)


def splits(frames):
    return [[3], [2, 1]] if frames == 3 else [[1]]


def grid():
    out = []
    for frames in (1, 3):
        for cams, stride in itertools.product((1, 2), (16, 20)):
            out.append(case("dev", DEV, NONE, cams, frames, stride))
            out.append(case("host", HOST, NONE, cams, frames, stride))
        for cams, up, down in itertools.product((1, 2), splits(frames), splits(frames)):
            out.append(case("host_parts", HOST, NONE, cams, frames, W, parts=(up, down if cams == 2 else [])))
        for stride, dirs in itertools.product((40, 48), (1, 2)):
            out.append(case("fisheye_dev", DEV, FLATTEN, 2, frames, stride, dirs))
            out.append(case("fisheye_host", HOST, FLATTEN, 2, frames, stride, dirs))
        for dirs in (1, 2):
            out.append(case("fisheye_jpeg_host", FILES, FLATTEN, 2, frames, SW, dirs))
        for stride in (40, 48):
            out.append(case("raw_dev", DEV, RESIZE, 2, frames, stride))
            out.append(case("raw_host", HOST, RESIZE, 2, frames, stride))
            for left, right in itertools.product(splits(frames), splits(frames)):
                out.append(case("raw_host_parts", HOST, RESIZE, 2, frames, stride, parts=(left, right)))
        for cams in (1, 2):
            out.append(case("jpeg_host", FILES, RESIZE, cams, frames, SW))
            out.append(case("jpeg_host", FILES, NONE, cams, frames, W))
    return out


def raw_bytes(c, cam, f):
    return (f * c["src_h"][cam] - 1) * c["stride"] + c["src_w"][cam]                             # the last row may end at its width


def expect(c):
    """the rules of the header's comment, restated from scratch: -> the dict run_pin returns"""
    form, pre, cams, n, frames = c["form"], c["pre"], c["cams"], c["n"], c["frames"]
    half = n * W * H
    e = dict(gray_bytes=0, raw_bytes=0, gray_cam1=half, raw_cam1=0, stage=RAW if pre != NONE else GRAY, parts=[[], []], dec_images=0, dec_stride=0, dec_w=0, dec_h=0,
             dec_max=0, dec_cap=0, pre_src=CALLER if form == DEV else RAW, pre_stride=c["stride"], unit_src=GRAY, unit_stride=W, unit_mask=c["mask"])
    if form == DEV and pre == NONE:                                                               # the dev entry: the caller's buffer, nothing in front of the unit
        e.update(unit_src=CALLER, unit_stride=c["stride"], steps=[(UNIT, 0)])
        return e
    e["gray_bytes"] = cams * half
    if pre == RESIZE or (form == FILES and pre == NONE):
        e["unit_mask"] = 0
    steps = []
    if form == FILES:                                                                             # packed frames, one decode
        sw, sh = c["src_w"][0], c["src_h"][0]
        e.update(dec_images=cams * frames, dec_stride=sw, pre_stride=sw, dec_w=sw, dec_h=sh, dec_cap=max(sw * sh // 2, 1024),
                 dec_max=2 * (N_CAP // c["dirs"]) if pre == FLATTEN else cams * N_CAP)
        if pre != NONE:
            e.update(raw_bytes=cams * frames * sw * sh, raw_cam1=frames * sw * sh)
        steps += [(DECODE_ALL, 0), (STATUS_DOWN, 0)]
    elif form == HOST and pre != NONE:                                                            # the pixel paths through d_raw
        e["raw_cam1"] = -(-raw_bytes(c, 0, frames) // 256) * 256
        e["raw_bytes"] = e["raw_cam1"] + raw_bytes(c, 1, frames)
    if form == HOST:
        for cam in range(cams):
            before = 0
            for k in (c["parts"][cam] if c["parts"] else [frames]):
                if pre != NONE:
                    e["parts"][cam].append(((e["raw_cam1"] if cam else 0) + before * c["stride"] * c["src_h"][cam], raw_bytes(c, cam, k), 0))
                else:                                                                             # straight into the input block, packed; 2-D when the rows are not
                    e["parts"][cam].append((cam * half + before * W * H, k * W * H, k * H if c["stride"] != W else 0))
                before += k
    for cam in range(cams):
        steps += [(UPLOAD, cam)] * (form == HOST) + [(PRE, cam)] * (pre != NONE) + [(FENCE, 0)] * (cam == 0)
    e["steps"] = steps + [(UNIT, 0)]
    return e


def build_pin(tmp) -> str:
    exe = os.path.join(str(tmp), "cam_input_pin_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "cam_input_pin.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_pin(exe, cases, tmp) -> list:
    """-> per case None (plan() said no) or every field of the plan"""
    fin, fout = os.path.join(str(tmp), "cases.bin"), os.path.join(str(tmp), "plans.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            parts = c["parts"] or ([1], [1])
            f.write(struct.pack("19i", c["form"], c["pre"], c["cams"], c["n"], c["W"], c["H"], c["n_cap"], *c["src_w"], *c["src_h"], c["stride"], c["frames"], c["first_view"],
                                c["dirs"], c["mask"], len(parts[0]), len(parts[1]), int(c["parts"] is not None)))
            if c["parts"] is not None:
                f.write(struct.pack(f"{len(parts[0]) + len(parts[1])}i", *parts[0], *parts[1]))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    d = open(fout, "rb").read()
    v, p, out = struct.unpack(f"{len(d) // 8}q", d), 0, []

    def take(k):
        nonlocal p
        p += k
        return v[p - k:p]
    for _ in cases:
        if not take(1)[0]:
            out.append(None)
            continue
        e = dict(zip(("gray_bytes", "raw_bytes", "gray_cam1", "raw_cam1", "stage"), take(5)))
        n0, n1 = take(2)
        e["parts"] = [[tuple(take(3)) for _ in range(k)] for k in (n0, n1)]
        e.update(zip(("dec_images", "dec_stride", "dec_w", "dec_h", "dec_max", "dec_cap", "pre_src", "pre_stride", "unit_src", "unit_stride", "unit_mask"), take(11)))
        e["steps"] = [tuple(take(2)) for _ in range(take(1)[0])]
        out.append(e)
    assert p == len(v)
    return out


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return build_pin(tmp_path_factory.mktemp("cam_input_pin"))


@pytest.fixture(scope="module")
def plans(pin, tmp_path_factory):
    cases = grid()
    return cases, run_pin(pin, cases, tmp_path_factory.mktemp("cam_input_grid"))


def test_every_field_of_every_plan_equals_the_restatement(plans):
    cases, got = plans
    assert {c["entry"] for c in cases} == {"dev", "host", "host_parts", "fisheye_dev", "fisheye_host", "fisheye_jpeg_host", "raw_dev", "raw_host", "raw_host_parts", "jpeg_host"}
    for c, g in zip(cases, got):
        want = expect(c)
        assert g is not None, c
        assert set(g) == set(want), c
        for key in want:
            assert g[key] == want[key], (key, c, g[key], want[key])


def test_the_worked_example_of_raw_stereo_host_parts(pin, tmp_path):
    packed, padded = run_pin(pin, [case("raw_host_parts", HOST, RESIZE, 2, 3, stride, parts=([2, 1], [2, 1]), mask=0) for stride in (40, 48)], tmp_path)
    assert packed["parts"][0] == [(0, 1920, 0), (1920, 960, 0)]
    assert packed["raw_cam1"] == 3072 and packed["raw_bytes"] == 5952
    assert packed["parts"][1] == [(3072, 1920, 0), (3072 + 1920, 960, 0)]
    assert (3 * 24 - 1) * 48 + 40 == 3448                                                         # the raw bytes of 3 frames at stride 48
    assert padded["raw_cam1"] == 3584 and padded["raw_bytes"] == 7032
    assert sum(padded["parts"][0][-1][:2]) == 3448                                                # the last part ends where the camera's raw bytes end
    for g in (packed, padded):
        assert g["gray_bytes"] == 2 * 3 * W * H and g["unit_mask"] == 0
        assert g["steps"] == [(UPLOAD, 0), (PRE, 0), (FENCE, 0), (UPLOAD, 1), (PRE, 1), (UNIT, 0)]


def test_step_order(plans):
    cases, got = plans
    for c, g in zip(cases, got):
        kinds = [k for k, _ in g["steps"]]
        assert kinds[-1] == UNIT and kinds.count(UNIT) == 1, c
        if c["entry"] == "dev":                                                                   # (the module's docstring)
            assert g["steps"] == [(UNIT, 0)] and g["gray_bytes"] == 0 == g["raw_bytes"], c
            continue
        assert kinds.count(FENCE) == 1, c
        fence = kinds.index(FENCE)
        assert all(cam == 0 for _, cam in g["steps"][:fence]), c                                  # nothing of the second camera in front of it
        assert all(cam == 1 for k, cam in g["steps"][fence + 1:] if k in (UPLOAD, PRE)), c        # nothing of the first camera behind it
        assert all(k not in (DECODE_ALL, STATUS_DOWN) for k in kinds[fence:]), c
        if c["form"] == FILES:
            assert kinds[:2] == [DECODE_ALL, STATUS_DOWN], c                                      # in front of the first PRE
        assert kinds.count(UPLOAD) == (c["cams"] if c["form"] == HOST else 0) and kinds.count(PRE) == (c["cams"] if c["pre"] != NONE else 0), c


def test_the_cameras_byte_ranges_do_not_overlap_and_end_inside_the_planned_size(plans):
    cases, got = plans
    seen = 0
    for c, g in zip(cases, got):
        if c["form"] != HOST:
            continue
        size = g["raw_bytes"] if g["stage"] == RAW else g["gray_bytes"]
        spans = []
        for cam in range(c["cams"]):
            assert g["parts"][cam], c
            lo, hi = min(d for d, _, _ in g["parts"][cam]), max(d + b for d, b, _ in g["parts"][cam])
            parts = sorted(g["parts"][cam])
            assert all(a[0] + a[1] <= b[0] for a, b in zip(parts, parts[1:])), c                   # a camera's own parts do not overlap either
            spans.append((lo, hi))
            assert 0 <= lo < hi <= size, (c, lo, hi, size)
            if c["pre"] != NONE:                                                                   # what the pre-processing reads of this camera lies in what was planned
                start = g["raw_cam1"] if cam else 0
                assert lo == start and hi == start + raw_bytes(c, cam, c["frames"]) <= size, c
        if c["cams"] == 2:
            assert spans[0][1] <= spans[1][0], (c, spans)
            seen += 1
    assert seen >= 20


def test_what_is_not_a_unit_is_refused_not_planned(pin, tmp_path):
    """parts that do not add up, an empty part, more parts than a handle holds, no frames: plan() says no and the executor enqueues nothing"""
    bad = [case("raw_host_parts", HOST, RESIZE, 2, 3, 40, parts=([2, 2], [3])), case("host_parts", HOST, NONE, 2, 3, W, parts=([3], [2, 0, 1])),
           case("host_parts", HOST, NONE, 1, 3, W, parts=([1] * 65, [])), case("host", HOST, NONE, 2, 0, W), case("jpeg_host", FILES, NONE, 2, 65, W)]
    assert run_pin(pin, bad, tmp_path) == [None] * len(bad)


def test_the_header_is_plain_cpp():
    code = "\n".join(line.split("//")[0] for line in open(os.path.join(PKG, "csrc", "cam_input.h")).read().splitlines())
    for word in ("hip", "common.h", "omni_cam", "<vector>", "std::"):
        assert word not in code, word
