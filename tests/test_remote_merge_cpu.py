"""CPU gate of the order rule that lets remote key frames join a key-frame unit's detector batch (host/remote_queue.hpp, through omni_remote_merge_plan of
libomni_host_remote.so): a remote frame queued after p local key frames is seen by the detector after local frame p - 1 and before local frame p, remote frames
among themselves in arrival order.  The unit [a, b) takes every queued frame with p <= b: p < a goes to the head, p == b to the tail, p > b stays queued.  Against a
brute-force sort by (place, kind, arrival) over a few hundred random cases, and tests/cpp/remote_merge_pin.cpp: the header alone in a stand-alone program under
-fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(a, b, ps):
    """every frame that belongs to the batch, sorted by (the local number it stands in front of, remote before local, arrival)"""
    keyed = [((max(p, a), 0, q), (True, q)) for q, p in enumerate(ps) if p <= b] + [((s, 1, 0), (False, s - a)) for s in range(a, b)]
    return [slot for _, slot in sorted(keyed)], sum(p <= b for p in ps)


def test_head_tail_and_what_stays_queued(omni):
    from omni_swarm_amd.pipeline import remote_merge_plan as plan
    R, L = (lambda q: (True, q)), (lambda i: (False, i))
    assert plan(8, 12, [3]) == ([R(0), L(0), L(1), L(2), L(3)], 1)                           # p < a: waited since before the unit -> the head
    assert plan(8, 12, [8]) == ([R(0), L(0), L(1), L(2), L(3)], 1)                           # p == a: in front of the unit's first key frame
    assert plan(8, 12, [10]) == ([L(0), L(1), R(0), L(2), L(3)], 1)                          # between local 9 and local 10
    assert plan(8, 12, [12]) == ([L(0), L(1), L(2), L(3), R(0)], 1)                          # p == b: the tail
    assert plan(8, 12, [13]) == ([L(0), L(1), L(2), L(3)], 0)                                # p > b: stays queued
    assert plan(8, 12, [2, 8, 8, 9, 12, 12, 13, 20]) == ([R(0), R(1), R(2), L(0), R(3), L(1), L(2), L(3), R(4), R(5)], 6)      # arrival order among equal p
    assert plan(8, 12, []) == ([L(0), L(1), L(2), L(3)], 0)                                  # an empty queue
    assert plan(5, 5, []) == ([], 0) and plan(0, 0, [0, 0]) == ([R(0), R(1)], 2)             # no local key frames: remote frames alone
    assert plan(5, 5, [1, 5, 6]) == ([R(0), R(1)], 2)


def test_refusals(omni):
    from omni_swarm_amd.pipeline import remote_merge_plan as plan
    for args, word in (((4, 3, []), "b < a"), ((0, 4, [2, 1]), "decreases"), ((0, 4, [-1]), "negative")):
        with pytest.raises(omni.capi.OmniError, match=word):
            plan(*args)


def test_against_a_brute_force_sort(omni):
    from omni_swarm_amd.pipeline import remote_merge_plan as plan
    rng = np.random.default_rng(7)
    seen_head = seen_tail = seen_left = 0
    for _ in range(400):
        a = int(rng.integers(0, 30))
        b = a + int(rng.integers(0, 9))
        ps = sorted(int(p) for p in rng.integers(max(0, a - 3), b + 4, size=int(rng.integers(0, 12))))
        got, want = plan(a, b, ps), brute(a, b, ps)
        assert got == want, (a, b, ps)
        slots, taken = got
        assert [i for r, i in slots if r] == list(range(taken)) and [i for r, i in slots if not r] == list(range(b - a))      # arrival order, unit order, nothing lost
        seen_head += any(p < a for p in ps); seen_tail += any(p == b for p in ps); seen_left += any(p > b for p in ps)
    assert min(seen_head, seen_tail, seen_left) > 50


def test_the_header_alone_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "remote_merge_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "remote_merge_pin.cpp")])
    r = subprocess.run([exe, "11"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
