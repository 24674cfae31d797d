"""LoopDetectorCore's late verdicts -- defer_loop + resolve_loops, the certainty rule of host/verify_plan.hpp applied during the replay of a batch -- against the
frame-by-frame on_image_recv that verifies every candidate on the spot (tests/cpp/detector_batch_verify.cpp: a plain g++ program over host/omni_swarm.hpp linked
against libomni_hip.so, started as a child process).  The frames are the 12-frame, 3-drone mixed batch of tests/test_gpu_detector_mixed.py, whose program the new
one includes unchanged.  With inter_drone_init_frames = 3 the crossing falls inside the batch.  Identical: every LoopCandidate field including `loop`, the counters,
ntotal and the id maps; exactly one early resolve, at the crossing."""
import os
import subprocess

import pytest

from tests import test_gpu_detector_mixed as DM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("detector_batch_verify") / "detector_batch_verify")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", out, os.path.join(DM.ROOT, "tests", "cpp", "detector_batch_verify.cpp"), "-L", DM.LIBDIR,
                           "-lomni_hip", f"-Wl,-rpath,{DM.LIBDIR}"])
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_late_verdicts_equal_frame_by_frame(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and lines[-1] == "OK", r.stdout[-3000:] + r.stderr[-2000:]
    assert [l.split(":")[0] for l in lines if l.startswith("RUN")] == ["RUN batch"]
