"""CPU checks of the stream plan (csrc/stream_plan.h): how many HIP streams a default key-frame pipeline keeps, how many hardware queues the library asks of
the HIP runtime for them, and the rule by which its load-time initializer (csrc/ctx.hip) treats a GPU_MAX_HW_QUEUES the process already has.
tests/cpp/stream_plan_pin.cpp compiles the header with g++ and prints the constants and hw_queues_to_set over option x preset; both are restated here
independently.  Then the rule as the library applies it: a fresh child process per case loads libomni_hip.so through ctypes and reads the variable back
through libc's getenv.  (There is no test of the queue count itself: a process cannot see its own queues; the evidence is the kernel trace,
profiles/r11_queues.md.)"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "omni-swarm_amd", "lib", "libomni_hip.so")
OPTIONS = [0, 8, 16, 32, 64]
PRESETS = [None, "", "abc", "2", "4", "8", "16", "32", "48"]
CAP = 32


def plan_streams():
    """a default pipeline: default_pipelines lanes x 2, one tail lane x 2, the detector, PnP, one caller context, the null stream"""
    return 4 * 2 + 1 * 2 + 1 + 1 + 1 + 1


def request(streams):
    """rounded up to a multiple of 4, at least 8, never above 32"""
    return min(CAP, max(8, -(-streams // 4) * 4))


def to_set(option, preset):
    """0: leave the environment alone.  option 0 -> 0; preset unset, unparsable or lower than the option -> the option; equal or higher -> leave; never above 32"""
    if option == 0:
        return 0
    option = min(option, CAP)
    if preset is not None and re.fullmatch(r"[+-]?\d+", preset) and int(preset) >= option:
        return 0
    return option


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "stream_plan_pin.cpp")])
    return [line.split() for line in subprocess.run([exe], capture_output=True, check=True, text=True).stdout.splitlines()]


def test_the_plan_counts_the_streams_of_a_default_pipeline_and_asks_for_whole_fours(pin):
    plan = {l[1]: int(l[2]) for l in pin if l[0] == "plan"}
    assert plan == {"default_pipelines": 4, "lane_streams": 2, "tail_lanes": 1, "single_streams": 4, "streams": plan_streams(), "min_request": 8, "max": CAP,
                    "request": request(plan_streams())}
    assert plan["streams"] == 14 and plan["request"] == 16 and plan["request"] >= plan["streams"]
    got = {int(l[1]): int(l[2]) for l in pin if l[0] == "request"}
    assert got == {s: request(s) for s in range(41)}
    assert all(v % 4 == 0 and 8 <= v <= CAP for v in got.values()) and all(got[s] >= s for s in range(CAP + 1))


def test_hw_queues_to_set_overwrites_a_lower_preset_and_never_lowers_a_higher_one(pin):
    name = lambda p: "-" if p is None else ('""' if p == "" else p)
    got = {(int(l[1]), l[2]): int(l[3]) for l in pin if l[0] == "set"}
    assert got == {(o, name(p)): to_set(o, p) for o in OPTIONS for p in PRESETS}
    assert len(got) == len(OPTIONS) * len(PRESETS) and all(0 <= v <= CAP for v in got.values())
    for o in OPTIONS:
        for p in ("2", "4", "8", "16", "32", "48"):
            v = got[(o, p)]
            assert v == 0 or v > int(p)                            # whatever is written is higher than what was there
            assert v != 0 or o == 0 or int(p) >= min(o, CAP)       # ... and a preset is only left alone when it is no lower than the request


def test_the_config_table_takes_its_default_from_the_plan_and_stops_at_32(pin):
    import omni_loader
    capi = omni_loader.load().capi
    o = {t["env"]: t for t in capi.config_table()}["OMNI_HW_QUEUES"]
    plan = {l[1]: int(l[2]) for l in pin if l[0] == "plan"}
    assert (o["default"], o["lo"], o["hi"]) == (plan["request"], 0, CAP)
    host = open(os.path.join(ROOT, "omni-swarm_amd", "host", "keyframe_pipeline.hpp")).read()
    assert re.search(r"default_pipelines\(int precision\) \{ return precision == OMNI_PREC_F16 \? omni::STREAM_PLAN_DEFAULT_PIPELINES : 2; \}", host)


CHILD = r"""
import ctypes, sys
ctypes.CDLL(sys.argv[1])
libc = ctypes.CDLL(None)
libc.getenv.restype = ctypes.c_char_p
v = libc.getenv(b"GPU_MAX_HW_QUEUES")
print("unset" if v is None else v.decode())
"""


@pytest.mark.parametrize("preset, option, want", [("4", None, "16"), ("24", None, "24"), ("4", "0", "4"), (None, None, "16"),
                                                  ("4", "8", "8"), ("16", "8", "16"), (None, "0", "unset"), ("abc", None, "16"), ("4", "64", "16")])
def test_loading_the_library_applies_the_rule_to_the_process(preset, option, want):
    """preset 4 -> the plan's number; 24 stays; OMNI_HW_QUEUES=0 leaves 4 (or nothing) alone; unset -> the plan's number; OMNI_HW_QUEUES=8 over 4 gives exactly
    8 and does not lower 16; a preset that is no number is replaced; an option outside the table's range counts as the default (config_option_now)"""
    assert os.path.exists(LIB), "python -c 'import __graft_entry__ as g; g.build()'"
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "OMNI_HW_QUEUES", "OMNI_LIB")}
    if preset is not None:
        env["GPU_MAX_HW_QUEUES"] = preset
    if option is not None:
        env["OMNI_HW_QUEUES"] = option
    out = subprocess.run([sys.executable, "-c", CHILD, LIB], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == [want]
