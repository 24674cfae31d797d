// remote_queue.hpp -- where the key frames other drones sent go in a key-frame unit's detector batch (KeyframePipeline::Config::remote_in_stream), as a pure function.
//
// Every local key frame has a sequence number in hand-over order; a queued remote frame carries p, the number of local key frames handed over before it arrived.  The
// serial flow (flush, then on_remote_frame) shows the detector each remote frame after local frame p - 1 and before local frame p, remote frames among themselves in
// arrival order.  A unit covers the local numbers [a, b).  When its batch is begun it takes every queued frame with p <= b -- the queue is in arrival order and p never
// decreases along it, so that is a prefix -- and places each before local frame max(p, a): a frame that has waited since before the unit (p < a: the locals in front
// of it are all through the detector already) at the head, p == b at the tail.  a == b is a batch of remote frames alone.  Plain C++, no GPU: tests/cpp/remote_merge_pin.cpp
// and tests/test_remote_merge_cpu.py (through omni_remote_merge_plan) pin it against a sort by (max(p, a), kind, arrival).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace omni {

struct RemoteMergeSlot {
    bool remote;           // false: local key frame `index` of the unit (0 .. b - a - 1); true: queue entry `index` (0 = the oldest)
    int64_t index;
};

// the batch of the unit [a, b) in detector order; *n_taken: how many queue entries, from the front, it holds.  queue_p: p of the queued frames in arrival order
inline std::vector<RemoteMergeSlot> remote_merge_plan(int64_t a, int64_t b, const int64_t* queue_p, int64_t n_queue, int64_t* n_taken) {
    if (b < a || n_queue < 0 || (n_queue > 0 && !queue_p)) throw std::invalid_argument("remote_merge_plan: a unit [a, b) with b < a, or no queue");
    for (int64_t q = 0; q < n_queue; ++q)
        if (queue_p[q] < 0 || (q > 0 && queue_p[q] < queue_p[q - 1])) throw std::invalid_argument("remote_merge_plan: p is negative or decreases along the queue");
    std::vector<RemoteMergeSlot> out;
    int64_t q = 0;
    for (int64_t s = a; s <= b; ++s) {                        // in front of local frame s (s == b: behind the last one)
        while (q < n_queue && queue_p[q] <= s) out.push_back({true, q++});
        if (s < b) out.push_back({false, s - a});
    }
    if (n_taken) *n_taken = q;
    return out;
}

}  // namespace omni
