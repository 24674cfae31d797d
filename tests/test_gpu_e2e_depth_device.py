"""CameraConfig::PINHOLE_DEPTH end to end with KeyframePipeline::Config::device_depth_landmarks off and on: the scene of tests/test_gpu_e2e_depth.py (imported:
8 places in front of a stepped wall, each visited twice) through the C++ key-frame pipeline, by run() and by push_keyframe + flush, with the ideal lens and a
distorted one.  Off is the host path that test holds to the oracle chain; on must give the same hits, candidates and LoopEdges and, for every key frame of the
database, the same message fields (landmarks_2d, landmarks_2d_norm, landmarks_3d, landmarks_flag) bit for bit.  With the switch on the caller overwrites its
depth buffer right after every push_keyframe returns.

Also here, because they need a live pipeline: the switch's round trip through libomni_host_depth.so and its refusal for camera configurations 0 and 1."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import test_gpu_e2e_depth as E

pytestmark = pytest.mark.gpu
MB = 4
LENSES = {"ideal": None, "distorted": dict(type="PINHOLE", k1=-0.05, k2=0.01, p1=1e-3, p2=-1e-3)}
FIELDS = ("landmarks_2d", "landmarks_2d_norm", "landmarks_3d", "landmarks_flag")


@pytest.fixture(scope="module")
def scene(omni, ctx, tmp_path_factory):
    from omni_swarm_amd import weights
    c = omni.capi
    comp, mean = synth.pca()
    files = weights.write_pipeline_files(str(tmp_path_factory.mktemp("depth_device")), S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), c.VLAD_KINDS)
    plan = E.schedule()
    frames = [synth.depth_keyframe(p, E.H, E.W, rv, sg) for (p, rv, sg, _) in plan]
    pins = []
    for s in range(0, len(plan), MB):
        p = ctx.host_alloc((MB, E.H, E.W), np.uint8)
        p[:] = np.stack([frames[s + m][0] for m in range(MB)])
        pins.append(p)
    poses = np.array([np.concatenate([q[3][0], q[3][1]]) for q in plan])
    yield {"files": files, "plan": plan, "frames": frames, "pins": pins, "poses": poses}
    for p in pins:
        ctx.host_free(p)


def make(omni, scene, lens, on, microbatch):
    from omni_swarm_amd import pipeline
    c, f, P = omni.capi, scene["files"], E.PARAMS
    return pipeline.KeyframePipeline(0, f["sp"], f["comp"], f["mean"], f["vlad"], E.W, E.H, E.THR, E.MAXN, c.PREC_F16, microbatch, 2, c.STORE_F32, 1, P["inner_product_thres"],
                                     P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"], geometry=True,
                                     pinhole_depth=dict(fx=E.FX, fy=E.FY, cx=E.CX, cy=E.CY, depth_near=E.NEAR, depth_far=E.FAR, accept_min_3d_pts=E.ACCEPT_MIN),
                                     camera_model=LENSES[lens], device_depth_landmarks=on)


def collect(pl, hits, n):
    out = {"hits": hits, "cand": pl.candidates().copy(), "edges": pl.edges().copy(), "rows": pl.db_rows, "frames": []}
    for i in range(n):
        out["frames"].append(pl.frame_landmarks(i, 0))
    pl.close()
    return out


def by_run(omni, scene, lens, on):
    pl = make(omni, scene, lens, on, MB)
    assert pl.device_depth_landmarks() == on
    n = len(scene["plan"])
    pl.set_poses(0, scene["poses"])
    pl.set_depth(0, np.stack([f[1] for f in scene["frames"]]))
    return collect(pl, pl.run(n, 0, [p.ctypes.data for p in scene["pins"]], 0, None, True), n)


def by_push(omni, scene, lens, on):
    pl = make(omni, scene, lens, on, 3)                                       # 16 key frames in micro-batches of 3: five full units and one of 1
    hits, buf = 0, np.zeros((E.H, E.W), np.uint16)
    keep = []
    for i, (gray, depth) in enumerate(scene["frames"]):
        if on:                                                                # ONE buffer for every key frame, overwritten as soon as the push returns
            buf[:] = depth
            hits += pl.push_keyframe([gray], i, float(i), scene["poses"][i], False, depth=buf)
            buf[:] = 0xFFFF if i % 2 else 1000
        else:                                                                 # the host path borrows the frame until its unit is finished
            keep.append(np.ascontiguousarray(depth))
            hits += pl.push_keyframe([gray], i, float(i), scene["poses"][i], False, depth=keep[-1])
    hits += pl.flush()
    return collect(pl, hits, len(scene["frames"]))


def same(a, b) -> list:
    bad = [k for k in ("hits", "rows") if a[k] != b[k]]
    bad += [k for k in ("cand", "edges") if a[k].shape != b[k].shape or not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))]
    for i, (fa, fb) in enumerate(zip(a["frames"], b["frames"])):
        bad += [f"frame {i} {k}" for k in FIELDS if fa[k].shape != fb[k].shape or not np.array_equal(fa[k].view(np.uint8), fb[k].view(np.uint8))]
    return bad


@pytest.mark.parametrize("intake", ["run", "push"])
@pytest.mark.parametrize("lens", list(LENSES))
def test_switch_on_equals_switch_off(omni, ctx, scene, lens, intake):
    go = by_run if intake == "run" else by_push
    off, on = go(omni, scene, lens, False), go(omni, scene, lens, True)
    n3 = [int(f["landmarks_flag"].sum()) for f in on["frames"]]
    print(f"{lens} lens by {intake}: hits {off['hits']} / {on['hits']}, candidates {len(off['cand'])} / {len(on['cand'])}, edges {len(off['edges'])} / {len(on['edges'])}, "
          f"landmarks per key frame {n3}")
    assert same(off, on) == []
    assert on["rows"] == len(scene["plan"]) and min(n3) > E.ACCEPT_MIN and on["hits"] == len(on["cand"]) >= E.N_PLACES            # not vacuous
    if lens == "ideal":
        assert len(on["edges"]) >= E.N_PLACES - 1                             # the loop closures of the scene (tests/test_gpu_e2e_depth.py has the ground truth)


def test_switch_round_trip_and_refusals(omni, ctx, scene):
    from omni_swarm_amd import pipeline
    c, f, P = omni.capi, scene["files"], E.PARAMS
    pl = make(omni, scene, "ideal", None, 2)
    try:
        assert pl.device_depth_landmarks() is False                           # the default stays off
        pl.set_device_depth_landmarks(True)
        assert pl.device_depth_landmarks() is True
        pl.set_device_depth_landmarks(False)
        assert pl.device_depth_landmarks() is False
        pl.push_keyframe([scene["frames"][0][0]], 0, 0.0, scene["poses"][0], False, depth=scene["frames"][0][1])
        with pytest.raises(c.OmniError, match="after the first key frame"):
            pl.set_device_depth_landmarks(True)
        pl.flush()
    finally:
        pl.close()
    common = (0, f["sp"], f["comp"], f["mean"], f["vlad"], 128, 96, 0.015, 100, c.PREC_F16, 2, 2, c.STORE_F32, 1, P["inner_product_thres"], P["init_mode_product_thres"],
              P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"])
    for kw in (dict(), dict(stereo_pinhole=dict(fx=64.0, fy=64.0, cx=63.5, cy=47.5))):          # configurations 1 (STEREO_FISHEYE) and 0 (STEREO_PINHOLE)
        pl = pipeline.KeyframePipeline(*common, geometry=True, **kw)
        try:
            for on in (True, False):
                with pytest.raises(c.OmniError, match="camera_configuration is not 2"):
                    pl.set_device_depth_landmarks(on)
            assert pl.device_depth_landmarks() is False
        finally:
            pl.close()
