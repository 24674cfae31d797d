// verify_plan.hpp -- when the detector may leave an inter-drone loop candidate unverified (KeyframePipeline::Config::batch_verify), as a pure function.
//
// LoopDetectorCore::on_image_recv runs a frame of remote drone x in init_mode while c = inter_drone_loop_count[{x, self}] < T = inter_drone_init_frames
// (loop_detector.cpp:66-72), and every accepted loop between x and self adds 1 to c (:826-827).  That is the only place a candidate's verdict is read.  The counter
// only grows and each of the u candidates between x and self that are deferred and not yet verified can add at most 1 to it, so the mode of x's next frame is
// known without their verdicts when c >= T (not init_mode, whatever they say) or c + u < T (init_mode, whatever they say).  Otherwise everything pending is
// resolved -- one batched verification, the verdicts applied in candidate order -- and the mode is read from the new c.  A candidate of a frame of the self drone
// against a frame of x counts in u of x like one of x's own frames; a candidate between two frames of the self drone touches no counter that is ever read.
// Plain C++, no GPU: tests/cpp/verify_plan_pin.cpp and tests/test_verify_plan_cpu.py (through omni_verify_plan) pin it against a serial walk.
#pragma once
#include <cstdint>
#include <map>
#include <stdexcept>
#include <vector>

namespace omni {

enum class VerifyRule { DEFER_NORMAL, DEFER_INIT, RESOLVE };      // init_mode false, certain; init_mode true, certain; not known before the pending verdicts

inline VerifyRule verify_rule(int64_t c, int64_t u, int64_t T) {
    if (c < 0 || u < 0) throw std::invalid_argument("verify_rule: a negative count");
    if (c >= T) return VerifyRule::DEFER_NORMAL;
    if (c + u < T) return VerifyRule::DEFER_INIT;
    return VerifyRule::RESOLVE;
}

// u per remote drone, between two resolves
class VerifyPending {
public:
    int64_t of(int drone) const { const auto it = u_.find(drone); return it == u_.end() ? 0 : it->second; }
    void defer(int drone) { ++u_[drone]; ++total_; }
    void resolved() { u_.clear(); total_ = 0; }
    int64_t total() const { return total_; }
private:
    std::map<int, int64_t> u_;
    int64_t total_ = 0;
};

// One frame of a stream as the rule sees it.  drone: the frame's drone.  partner / partner_init: the drone of the old frame its candidate is matched against when the
// frame runs out of / in init_mode (-1: no candidate; a frame of the self drone reads `partner`).  verdict: what the verification of that candidate says.
struct VerifyFrame { int drone, partner, partner_init; bool verdict; };
struct VerifyStep { bool init_mode, resolved_before; };      // per frame: its mode; whether everything pending had to be resolved in front of it

// The replay of one detector batch with deferred verdicts: count holds c per remote drone (read and updated), every frame's mode and forced resolve come back, and
// everything pending is resolved when the batch ends (*end_resolve: there was something to resolve).  A candidate between a remote frame and a frame of another
// remote drone is never verified (loop_detector.cpp:110-115) and counts nowhere.
inline std::vector<VerifyStep> verify_plan_batch(int self_id, int64_t T, const VerifyFrame* frames, int64_t n, std::map<int, int64_t>& count, bool* end_resolve) {
    if (n < 0 || (n > 0 && !frames)) throw std::invalid_argument("verify_plan_batch: no frames");
    struct Ticket { int drone; bool verdict; };
    std::vector<Ticket> tickets;
    VerifyPending pending;
    auto resolve = [&] { for (const Ticket& t : tickets) if (t.verdict) ++count[t.drone]; tickets.clear(); pending.resolved(); };
    std::vector<VerifyStep> out;
    for (int64_t i = 0; i < n; ++i) {
        const VerifyFrame& f = frames[i];
        VerifyStep s{false, false};
        if (f.drone != self_id) {
            VerifyRule r = verify_rule(count[f.drone], pending.of(f.drone), T);
            if (r == VerifyRule::RESOLVE) { resolve(); s.resolved_before = true; r = verify_rule(count[f.drone], 0, T); }
            s.init_mode = r == VerifyRule::DEFER_INIT;
        }
        const int partner = s.init_mode ? f.partner_init : f.partner;
        if (partner >= 0) {
            const int x = f.drone != self_id ? f.drone : partner;       // the remote drone of the pair
            if (x != self_id && (f.drone == self_id || partner == self_id)) { tickets.push_back({x, f.verdict}); pending.defer(x); }
        }
        out.push_back(s);
    }
    if (end_resolve) *end_resolve = !tickets.empty();
    resolve();
    return out;
}

}  // namespace omni
