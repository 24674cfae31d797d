// verify_plan_pin.cpp -- host/verify_plan.hpp alone in a stand-alone program (tests/test_verify_plan_cpu.py builds it with -fsanitize=address,undefined):
// verify_plan_batch against an independent restatement -- verify every candidate on the spot, frame by frame -- over random streams cut into batches, heap vectors
// of exactly the needed size, the rule's three answers on its edges, and the refusals.  usage: verify_plan_pin <seed>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../omni-swarm_amd/host/verify_plan.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using omni::VerifyFrame;
using omni::VerifyRule;

int main(int argc, char** argv) {
    std::mt19937_64 rng(argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    const int self = 1;
    CHECK(omni::verify_rule(2, 0, 3) == VerifyRule::DEFER_INIT && omni::verify_rule(2, 1, 3) == VerifyRule::RESOLVE && omni::verify_rule(3, 0, 3) == VerifyRule::DEFER_NORMAL);
    CHECK(omni::verify_rule(3, 9, 3) == VerifyRule::DEFER_NORMAL && omni::verify_rule(0, 0, 0) == VerifyRule::DEFER_NORMAL && omni::verify_rule(0, 2, 3) == VerifyRule::DEFER_INIT);
    CHECK(omni::verify_rule(0, 3, 3) == VerifyRule::RESOLVE && omni::verify_rule(0, 7, -1) == VerifyRule::DEFER_NORMAL);
    int64_t cases = 0, frames_seen = 0, early = 0;
    for (int it = 0; it < 2000; ++it) {
        const int64_t T = pick(0, 5);
        std::map<int, int64_t> got_count, want_count;
        for (int64_t b = pick(1, 3); b > 0; --b) {
            std::vector<VerifyFrame> frames((size_t)pick(0, 12));
            for (auto& f : frames) {
                f.drone = (int)pick(0, 3);
                f.partner_init = (int)pick(-1, 3);
                f.partner = (f.drone == self || pick(0, 9) < 6) ? f.partner_init : -1;
                f.verdict = pick(0, 9) < 6;
            }
            bool end_resolve = false;
            const std::vector<omni::VerifyStep> got = omni::verify_plan_batch(self, T, frames.empty() ? nullptr : frames.data(), (int64_t)frames.size(), got_count, &end_resolve);
            CHECK(got.size() == frames.size());
            bool any = false;
            for (size_t i = 0; i < frames.size(); ++i) {       // the serial flow: the verdict is in before the next frame
                const VerifyFrame& f = frames[i];
                const bool mode = f.drone != self && want_count[f.drone] < T;
                CHECK(got[i].init_mode == mode);
                CHECK(!got[i].resolved_before || f.drone != self);
                const int partner = mode ? f.partner_init : f.partner;
                if (partner >= 0 && partner != f.drone && (partner == self || f.drone == self)) { any = true; if (f.verdict) ++want_count[f.drone != self ? f.drone : partner]; }
                early += got[i].resolved_before;
            }
            CHECK(any || !end_resolve);
            for (int x = 0; x < 4; ++x) CHECK(got_count[x] == want_count[x]);
            ++cases; frames_seen += (int64_t)frames.size();
        }
    }
    CHECK(early > 200);
    std::map<int, int64_t> count;
    CHECK(omni::verify_plan_batch(self, 3, nullptr, 0, count, nullptr).empty());          // end_resolve may be null
    int refused = 0;
    try { omni::verify_plan_batch(self, 3, nullptr, 2, count, nullptr); } catch (const std::invalid_argument&) { ++refused; }
    try { omni::verify_plan_batch(self, 3, nullptr, -1, count, nullptr); } catch (const std::invalid_argument&) { ++refused; }
    try { omni::verify_rule(-1, 0, 3); } catch (const std::invalid_argument&) { ++refused; }
    try { omni::verify_rule(0, -1, 3); } catch (const std::invalid_argument&) { ++refused; }
    CHECK(refused == 4);
    omni::VerifyPending p;
    p.defer(2); p.defer(2); p.defer(3);
    CHECK(p.of(2) == 2 && p.of(3) == 1 && p.of(4) == 0 && p.total() == 3);
    p.resolved();
    CHECK(p.of(2) == 0 && p.total() == 0);
    std::printf("%lld batches, %lld frames, %lld early resolves\nOK\n", (long long)cases, (long long)frames_seen, (long long)early);
    return 0;
}
