// How many HIP streams a default key-frame pipeline keeps, and how many hardware queues the library therefore asks of the HIP runtime when it is loaded.
// The runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless set), idle streams included, and two streams on one queue run
// strictly one after the other: units "in flight" on streams that share a queue are not in flight together.  This header is the one statement of the count
// and of the rule by which the library's initializer (ctx.hip) treats a value the process already has.  Plain host C++, no HIP:
// tests/cpp/stream_plan_pin.cpp compiles it under g++ and tests/test_stream_plan_cpu.py compares every case against an independent restatement.
#pragma once
#include <cerrno>
#include <cstdlib>

namespace omni {

// ---- the streams of a default pipeline (host/keyframe_pipeline.hpp) ----
constexpr int STREAM_PLAN_DEFAULT_PIPELINES = 4;       // KeyframePipeline::default_pipelines(OMNI_PREC_F16): units in flight, one lane each
constexpr int STREAM_PLAN_LANE_STREAMS = 2;            // Lane: sp_ctx (upload, SuperPoint, matcher, result copies) + vlad_ctx (MobileNetVLAD)
constexpr int STREAM_PLAN_TAIL_LANES = 1;              // prepare(): the lane of a run's trailing partial micro-batch
constexpr int STREAM_PLAN_SINGLE_STREAMS = 4;          // the detector's high-priority context, PnP's, one context of the caller's, the null stream
constexpr int STREAM_PLAN_STREAMS = (STREAM_PLAN_DEFAULT_PIPELINES + STREAM_PLAN_TAIL_LANES) * STREAM_PLAN_LANE_STREAMS + STREAM_PLAN_SINGLE_STREAMS;

// ---- the queues to ask for: that many, in whole fours (the runtime's own default is 4), at least 8, never above 32 ----
constexpr int HW_QUEUES_MIN_REQUEST = 8;
constexpr int HW_QUEUES_MAX = 32;
constexpr int hw_queues_request(int streams) {
    const int r = (streams + 3) / 4 * 4;
    return r < HW_QUEUES_MIN_REQUEST ? HW_QUEUES_MIN_REQUEST : (r > HW_QUEUES_MAX ? HW_QUEUES_MAX : r);
}
constexpr int HW_QUEUES_DEFAULT = hw_queues_request(STREAM_PLAN_STREAMS);      // OMNI_HW_QUEUES' default (config.hip)

// What the initializer writes into GPU_MAX_HW_QUEUES; 0 = it leaves the environment alone.  option: OMNI_HW_QUEUES; preset: the variable's value when the
// library is loaded (nullptr: unset).  A preset that is no whole number, or lower than the option, is replaced by the option; one that is as high or higher
// stays (a process that chose more keeps it: the library never lowers the count); nothing above HW_QUEUES_MAX is ever written.
inline int hw_queues_to_set(int option, const char* preset) {
    if (option <= 0) return 0;
    if (option > HW_QUEUES_MAX) option = HW_QUEUES_MAX;
    if (preset && preset[0]) {
        errno = 0;
        char* end = nullptr;
        const long v = strtol(preset, &end, 10);
        if (!errno && end != preset && *end == '\0' && v >= option) return 0;
    }
    return option;
}

}  // namespace omni
