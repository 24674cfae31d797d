"""CPU gate of the certainty rule that lets the detector leave inter-drone loop candidates unverified until their batch ends (host/verify_plan.hpp, through
omni_verify_plan of libomni_host_verify.so).  A frame of remote drone x runs in init_mode while c = inter_drone_loop_count[{x, self}] < T; with u candidates between
x and self pending, the mode is certain when c >= T or c + u < T, and everything pending is resolved otherwise.  Against a serial walk that verifies every candidate
on the spot, over 400 random streams (drone ids 0..3, T in 0..5, batches of 1..12 frames, random verdicts): the same init_mode per frame, the same final counters,
and a resolve exactly where trying every assignment of the pending verdicts shows the mode to depend on them.  tests/cpp/verify_plan_pin.cpp: the header alone in a
stand-alone program under -fsanitize=address,undefined."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELF = 1


def plan(T, frames, batches, n_drones=4):
    """frames: [(drone, partner, partner_init, verdict)]"""
    from omni_swarm_amd.pipeline import verify_plan
    d, p, pi, v = (list(x) for x in zip(*frames)) if frames else ([], [], [], [])
    return verify_plan(SELF, T, d, p, pi, v, batches, n_drones)


def inter(drone, partner):
    """the remote drone whose counter the candidate can raise, or None (no candidate, two frames of the self drone, two remote drones: never verified)"""
    if partner < 0 or drone == partner or SELF not in (drone, partner):
        return None
    return drone if drone != SELF else partner


def serial(T, frames, n_drones=4):
    """every candidate verified on the spot: (init_mode per frame, counters)"""
    c, modes = [0] * n_drones, []
    for drone, partner, partner_init, verdict in frames:
        mode = drone != SELF and c[drone] < T
        x = inter(drone, partner_init if mode else partner)
        if x is not None and verdict:
            c[x] += 1
        modes.append(mode)
    return modes, c


def test_the_edges_of_the_rule(omni):
    R = lambda verdict=1: (2, SELF, SELF, verdict)            # a frame of drone 2 matched against a frame of the self drone
    # c = T - 1 with u = 0: certain, init mode, nothing to resolve; the batch's end resolves the one candidate
    modes, early, end, cnt = plan(2, [R(), R()], [1, 1])
    assert modes == [True, True] and early == [False, False] and end == [True, True] and cnt[2] == 2
    # c = T - 1 with u = 1: the pending verdict decides -> resolved in front of the frame; accepted: init mode is over, rejected: it is not
    assert plan(2, [R(), R(), R()], [1, 2])[:2] == ([True, True, False], [False, False, True])
    assert plan(2, [R(), R(0), R()], [1, 2])[:2] == ([True, True, True], [False, False, True])
    # c = T: certain, whatever is pending
    modes, early, end, cnt = plan(2, [R(), R(), R(), R(), R()], [2, 3])
    assert modes == [True, True, False, False, False] and early == [False] * 5 and end == [True, True] and cnt[2] == 5
    # T = 0: never init mode, never a resolve in front of a frame
    assert plan(0, [R()] * 6, [6])[:3] == ([False] * 6, [False] * 6, [True])
    # c + u < T: certain however many are pending
    assert plan(9, [R()] * 8, [8])[:2] == ([True] * 8, [False] * 8)
    # a candidate of a self-drone frame against a frame of drone 2 counts in u of drone 2
    assert plan(1, [(SELF, 2, 2, 1), R()], [2])[:2] == ([False, False], [False, True])
    # ... one between two self-drone frames, or between two remote drones, does not
    assert plan(1, [(SELF, SELF, SELF, 1), (3, 2, 2, 1), R()], [3])[:3] == ([False, True, True], [False, False, False], [True])
    # two remote drones interleaved: drone 3's pending candidates do not make drone 2's mode uncertain, but a resolve forced by one serves both
    A, B = (2, SELF, SELF, 1), (3, SELF, SELF, 1)
    modes, early, end, cnt = plan(2, [A, B, B, A, B, A], [6])
    assert modes == [True, True, True, True, False, False] and early == [False, False, False, False, True, False] and cnt[2:] == [3, 3]
    # a frame without a candidate, an empty batch, no frames at all
    assert plan(2, [(2, -1, -1, 0)], [0, 1])[:3] == ([True], [False], [False, False])
    assert plan(2, [], []) == ([], [], [], [0, 0, 0, 0])


def test_refusals(omni):
    for frames, batches, word in (([(2, SELF, SELF, 1)], [2], "add up"), ([(7, SELF, SELF, 1)], [1], "outside"), ([(2, 9, SELF, 1)], [1], "outside"),
                                  ([(2, SELF, SELF, 1)], [-1, 2], "negative")):
        with pytest.raises(omni.capi.OmniError, match=word):
            plan(2, frames, batches)


def test_against_a_serial_walk(omni):
    rng = np.random.default_rng(11)
    early_total = crossings = init_only = 0
    for _ in range(400):
        T = int(rng.integers(0, 6))
        batches = [int(rng.integers(1, 13)) for _ in range(int(rng.integers(1, 4)))]
        frames = []
        for _ in range(sum(batches)):
            drone = int(rng.integers(0, 4))
            partner_init = int(rng.choice([-1, SELF, SELF, SELF, 0, 2, 3])) if drone != SELF else int(rng.choice([-1, SELF, 0, 2, 3]))
            partner = partner_init if (drone == SELF or rng.random() < 0.6) else -1      # the init-mode threshold is the lower one: it finds what the other finds, and more
            frames.append((drone, partner, partner_init, int(rng.random() < 0.6)))
        modes, early, end, cnt = plan(T, frames, batches)
        want_modes, want_cnt = serial(T, frames)
        assert modes == want_modes and cnt == want_cnt, (T, batches, frames)
        # a resolve exactly where the mode depends on a pending verdict: try every assignment of the verdicts pending since the last resolve
        c, at = [0] * 4, 0
        for b, n in enumerate(batches):
            pending = []                                      # (remote drone, verdict)
            for i in range(at, at + n):
                drone, partner, partner_init, verdict = frames[i]
                if drone != SELF:
                    mine = [v for x, v in pending if x == drone]
                    depends = len({c[drone] + sum(a) < T for a in itertools.product((0, 1), repeat=len(mine))}) > 1
                    assert early[i] == depends, (T, batches, frames, i)
                    if depends:
                        for x, v in pending:
                            c[x] += v
                        pending = []
                        early_total += 1
                else:
                    assert not early[i]
                x = inter(drone, partner_init if modes[i] else partner)
                if x is not None:
                    pending.append((x, verdict))
                init_only += modes[i] and partner != partner_init
            assert end[b] == bool(pending)
            for x, v in pending:
                c[x] += v
            at += n
        assert c == cnt
        crossings += any(0 < T <= v for v in cnt)
    assert early_total > 100 and crossings > 100 and init_only > 100      # conditions on the cases, not measurements


def test_the_header_alone_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "verify_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "verify_plan_pin.cpp")])
    r = subprocess.run([exe, "11"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
