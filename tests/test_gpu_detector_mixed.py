"""LoopDetectorCore's batch whose rows come from both places -- a key-frame unit's block in HBM and remote frames' descriptors on the host, gathered by
csrc/rows_assemble.hip -- against the frame-by-frame on_image_recv (tests/cpp/detector_mixed.cpp: a plain g++ program over host/omni_swarm.hpp linked against
libomni_hip.so, started as a child process like tests/cpp/host_smoke.cpp).  12 synthetic frames of 3 drones with planted near-duplicates on both sides of both
thresholds, a malformed remote frame, an image without landmarks and a non-key frame; once without a geometry stage and once with a compute_loop stub that accepts
every second candidate, so that init mode ends inside the batch; then a batch of remote frames alone.  Identical: every LoopCandidate field with the score's bits,
ntotal of both indexes, imgid2fisheye, imgid2dir, the loop counters."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "omni-swarm_amd", "lib")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("detector_mixed") / "detector_mixed")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", out, os.path.join(ROOT, "tests", "cpp", "detector_mixed.cpp"), "-L", LIBDIR, "-lomni_hip",
                           f"-Wl,-rpath,{LIBDIR}"])
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_mixed_batch_equals_frame_by_frame(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and lines[-1] == "OK", r.stdout[-3000:] + r.stderr[-2000:]
    assert [l.split(":")[0] for l in lines[:-1]] == ["RUN stub 0", "RUN stub 1"]
