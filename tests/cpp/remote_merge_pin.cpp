// remote_merge_pin.cpp -- host/remote_queue.hpp alone in a stand-alone program (tests/test_remote_merge_cpu.py builds it with -fsanitize=address,undefined):
// remote_merge_plan against an independent restatement -- walk the serial flow frame by frame -- over random units and queues, heap vectors of exactly the needed
// size, and the refusals.  usage: remote_merge_pin <seed>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../omni-swarm_amd/host/remote_queue.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// The serial flow: local key frames 0 .. b - 1 are handed over one by one; a remote frame with p arrives when p have been.  What the detector sees from the moment
// the unit [a, b) is due: everything that arrived and was not seen, then the unit's frames with the arrivals between them.
static std::vector<omni::RemoteMergeSlot> serial(int64_t a, int64_t b, const std::vector<int64_t>& ps, int64_t* taken) {
    std::vector<omni::RemoteMergeSlot> out;
    std::vector<char> seen(ps.size(), 0);
    for (int64_t handed = a; handed <= b; ++handed) {            // `handed` local key frames are through (or, for the first step, waiting at the unit's door)
        for (size_t q = 0; q < ps.size(); ++q)
            if (!seen[q] && ps[q] <= handed) { seen[q] = 1; out.push_back({true, (int64_t)q}); }
        if (handed < b) out.push_back({false, handed - a});
    }
    *taken = 0;
    for (char s : seen) *taken += s;
    return out;
}

int main(int argc, char** argv) {
    std::mt19937_64 rng(argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    int64_t cases = 0, slots = 0;
    for (int it = 0; it < 2000; ++it) {
        const int64_t a = pick(0, 40), b = a + pick(0, 9);
        std::vector<int64_t> ps((size_t)pick(0, 14));
        int64_t p = pick(a > 4 ? a - 4 : 0, a + 1);
        for (auto& v : ps) { v = p; p += pick(0, 2); }
        int64_t taken = -1, want_taken = -1;
        const std::vector<omni::RemoteMergeSlot> got = omni::remote_merge_plan(a, b, ps.empty() ? nullptr : ps.data(), (int64_t)ps.size(), &taken);
        const std::vector<omni::RemoteMergeSlot> want = serial(a, b, ps, &want_taken);
        CHECK(taken == want_taken && got.size() == want.size() && (int64_t)got.size() == (b - a) + taken);
        for (size_t s = 0; s < got.size(); ++s) CHECK(got[s].remote == want[s].remote && got[s].index == want[s].index);
        for (int64_t q = taken; q < (int64_t)ps.size(); ++q) CHECK(ps[(size_t)q] > b);      // what stays queued comes behind the unit
        ++cases; slots += (int64_t)got.size();
    }
    CHECK(omni::remote_merge_plan(3, 3, nullptr, 0, nullptr).empty());                   // n_taken may be null
    int refused = 0;
    const int64_t down[2] = {5, 4}, neg[1] = {-1}, one[1] = {1};
    try { omni::remote_merge_plan(4, 3, one, 1, nullptr); } catch (const std::invalid_argument&) { ++refused; }
    try { omni::remote_merge_plan(0, 8, down, 2, nullptr); } catch (const std::invalid_argument&) { ++refused; }
    try { omni::remote_merge_plan(0, 8, neg, 1, nullptr); } catch (const std::invalid_argument&) { ++refused; }
    try { omni::remote_merge_plan(0, 8, nullptr, 2, nullptr); } catch (const std::invalid_argument&) { ++refused; }
    CHECK(refused == 4);
    std::printf("%lld cases, %lld slots\nOK\n", (long long)cases, (long long)slots);
    return 0;
}
