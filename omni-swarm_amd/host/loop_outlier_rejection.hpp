// loop_outlier_rejection.hpp -- SwarmLocalOutlierRejection::OutlierRejectionLoopEdges (swarm_localization/src/swarm_outlier_rejection/
// swarm_outlier_rejection.cpp:98-167) on edge records (include/omni_hip.h omni_pcm_edge): which of the loop edges seen so far agree with each other.
//
//   add(edges)   edges already seen by id are ignored; new ones are filed under both orders of their drone pair; with `redundant` off only the pairs with THIS drone at
//                one end are evaluated -- graph (self, other) -- and with it on every pair, graph (a, b) with a >= b (:122-139).  An evaluated pair's new edges are
//                appended to its graph, in the order given, in calls of at most 64: the consistency rows come from omni_pcm_add (csrc/pcm.hip, a handle per graph on the
//                context given) or, without a context, from omni_pcm_rows_host (the g++ build of the same header: the same bits), and the clique heuristic
//                (omni_pcm_max_clique_host) then runs on the host's copy of the graph's rows.  Its vertices are the pair's inlier set, under both orders.
//   good(e)      an edge passes when its drone pair has no inlier set yet or when the set holds its id (:142-157).
// An edge that does not fit its graph any more (the handle is full) stays outside it and passes like an edge of a pair that was never evaluated; it is counted.
// The LOOP_INLIERS message and its broadcast (:41-96, :135) are not part of this library.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/omni_hip.h"

namespace omni {

class LoopOutlierRejection {
public:
    struct Params {
        int self_id = 1;
        bool redundant = false;
        int capacity = OMNI_PCM_DEFAULT_CAPACITY;
        omni_pcm_params pcm{0.6, 0.01, 0.003};
    };
    // [0] edges entered into a graph, [1] pairs of edges evaluated, [2] consistent pairs, [3] clique runs, [4] (the pipeline's: edges with a frame it never saw),
    // [5] edges that met a full handle
    struct Stats { int64_t v[6] = {0, 0, 0, 0, 0, 0}; };

    // ctx == nullptr: the rows are computed on the host
    LoopOutlierRejection(omni_ctx* ctx, const Params& p) : ctx_(ctx), p_(p) {
        if (p.capacity < OMNI_PCM_MIN_CAPACITY || p.capacity > OMNI_PCM_MAX_CAPACITY || p.capacity % 64)
            throw std::invalid_argument("LoopOutlierRejection: capacity must be a multiple of 64 in 64..32768, not " + std::to_string(p.capacity));
    }
    ~LoopOutlierRejection() { for (auto& g : graphs_) if (g.second.handle) omni_pcm_destroy(g.second.handle); }
    LoopOutlierRejection(const LoopOutlierRejection&) = delete;
    LoopOutlierRejection& operator=(const LoopOutlierRejection&) = delete;

    const Params& params() const { return p_; }
    const Stats& stats() const { return stats_; }

    void add(const std::vector<omni_pcm_edge>& edges) {
        std::map<std::pair<int, int>, std::vector<omni_pcm_edge>> fresh;
        for (const omni_pcm_edge& e : edges) {
            if (seen_.count(e.id)) continue;
            fresh[{e.drone_a, e.drone_b}].push_back(e);
            if (e.drone_a != e.drone_b) fresh[{e.drone_b, e.drone_a}].push_back(e);
        }
        for (auto& kv : fresh) {
            const int a = kv.first.first, b = kv.first.second;
            if (p_.redundant ? a < b : a != p_.self_id) continue;
            // (an id that comes twice in one call enters once)
            std::vector<omni_pcm_edge> list;
            for (const omni_pcm_edge& e : kv.second) if (seen_.insert(e.id).second) list.push_back(e);
            if (!list.empty()) evaluate(a, b, list);
        }
    }
    bool good(int64_t id, int drone_a, int drone_b) const {
        if (outside_.count(id)) return true;
        const auto it = inliers_.find({drone_a, drone_b});
        return it == inliers_.end() || it->second.count(id) != 0;
    }
    bool good(const omni_pcm_edge& e) const { return good(e.id, e.drone_a, e.drone_b); }
    std::vector<omni_pcm_edge> good(const std::vector<omni_pcm_edge>& edges) const {
        std::vector<omni_pcm_edge> out;
        for (const omni_pcm_edge& e : edges) if (good(e)) out.push_back(e);
        return out;
    }
    // the inlier set of a pair (either order), nullptr when the pair was never evaluated
    const std::set<int64_t>* inliers(int drone_a, int drone_b) const {
        const auto it = inliers_.find({drone_a, drone_b});
        return it == inliers_.end() ? nullptr : &it->second;
    }

private:
    struct Graph {
        omni_pcm* handle = nullptr;
        std::vector<omni_pcm_edge> edges;       // the vertices, in the order they entered
        std::vector<uint64_t> rows;             // [edges.size()][words]: the host's copy of the bit matrix
    };
    static void fail(const char* what) { throw std::runtime_error(std::string(what) + ": " + omni_last_error()); }

    void evaluate(int a, int b, const std::vector<omni_pcm_edge>& list) {
        Graph& g = graphs_[{a, b}];
        const size_t words = (size_t)p_.capacity / 64;
        if (ctx_ && !g.handle && omni_pcm_create(ctx_, p_.capacity, &p_.pcm, &g.handle) != OMNI_OK) fail("omni_pcm_create");
        std::vector<int32_t> deg((size_t)p_.capacity);
        for (size_t at = 0; at < list.size();) {
            const size_t held = g.edges.size(), n = std::min<size_t>(OMNI_PCM_MAX_ADD, list.size() - at);
            if (held + n > (size_t)p_.capacity) {                                                           // OMNI_PCM_FULL: nothing of this call and nothing behind it
                stats_.v[5] += (int64_t)(list.size() - at);
                for (size_t k = at; k < list.size(); ++k) outside_.insert(list[k].id);
                break;
            }
            g.edges.insert(g.edges.end(), list.begin() + (long)at, list.begin() + (long)(at + n));
            g.rows.resize((held + n) * words, 0);
            uint64_t* fresh_rows = g.rows.data() + held * words;
            if (g.handle) {
                const int rc = omni_pcm_add(g.handle, list.data() + at, (int)n, deg.data(), fresh_rows, nullptr);
                if (rc != OMNI_OK) fail("omni_pcm_add");                                                    // (FULL cannot come: checked above)
            } else if (omni_pcm_rows_host(g.edges.data(), (int)(held + n), (int)held, &p_.pcm, (int)words, fresh_rows, deg.data(), nullptr) != OMNI_OK) {
                fail("omni_pcm_rows_host");
            }
            // the mirrored bits of the earlier rows, and the count of consistent pairs: every set bit (i, j < i) of a new row
            for (size_t i = held; i < held + n; ++i)
                for (size_t j = 0; j < i; ++j)
                    if ((g.rows[i * words + (j >> 6)] >> (j & 63)) & 1) { ++stats_.v[2]; if (j < held) g.rows[j * words + (i >> 6)] |= 1ull << (i & 63); }
            stats_.v[0] += (int64_t)n;
            stats_.v[1] += (int64_t)(n * held + n * (n - 1) / 2);
            at += n;
        }
        std::vector<int32_t> clique(g.edges.size() + 1);
        int size = 0;
        if (omni_pcm_max_clique_host(g.rows.empty() ? &zero_ : g.rows.data(), (int)g.edges.size(), (int)words, clique.data(), &size) != OMNI_OK) fail("omni_pcm_max_clique_host");
        ++stats_.v[3];
        std::set<int64_t> in;
        for (int k = 0; k < size; ++k) in.insert(g.edges[(size_t)clique[(size_t)k]].id);
        inliers_[{b, a}] = in;
        inliers_[{a, b}] = std::move(in);
    }

    omni_ctx* ctx_;
    Params p_;
    Stats stats_;
    std::set<int64_t> seen_, outside_;          // outside_: edges that met a full handle
    std::map<std::pair<int, int>, Graph> graphs_;
    std::map<std::pair<int, int>, std::set<int64_t>> inliers_;
    uint64_t zero_ = 0;
};

}  // namespace omni
