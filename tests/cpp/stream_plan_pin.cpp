// The stream plan (omni-swarm_amd/csrc/stream_plan.h) on the host, for tests/test_stream_plan_cpu.py.
//   stream_plan_pin
//     "plan NAME value" for every constant of the plan and for hw_queues_request(s), s = 0 .. 40;
//     "set OPTION PRESET result" for hw_queues_to_set over option {0, 8, 16, 32, 64} x preset {unset, "", "abc", "2", "4", "8", "16", "32", "48"}
//     (PRESET printed as - when unset and as "" when empty)
#include <cstdio>

#include "../../omni-swarm_amd/csrc/stream_plan.h"

using namespace omni;

int main() {
    printf("plan default_pipelines %d\n", STREAM_PLAN_DEFAULT_PIPELINES);
    printf("plan lane_streams %d\n", STREAM_PLAN_LANE_STREAMS);
    printf("plan tail_lanes %d\n", STREAM_PLAN_TAIL_LANES);
    printf("plan single_streams %d\n", STREAM_PLAN_SINGLE_STREAMS);
    printf("plan streams %d\n", STREAM_PLAN_STREAMS);
    printf("plan min_request %d\n", HW_QUEUES_MIN_REQUEST);
    printf("plan max %d\n", HW_QUEUES_MAX);
    printf("plan request %d\n", HW_QUEUES_DEFAULT);
    for (int s = 0; s <= 40; ++s) printf("request %d %d\n", s, hw_queues_request(s));
    const int options[] = {0, 8, 16, 32, 64};
    const char* presets[] = {nullptr, "", "abc", "2", "4", "8", "16", "32", "48"};
    for (int o : options)
        for (const char* p : presets) printf("set %d %s %d\n", o, !p ? "-" : (p[0] ? p : "\"\""), hw_queues_to_set(o, p));
    return 0;
}
