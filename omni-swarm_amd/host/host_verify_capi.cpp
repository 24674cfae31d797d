// host_verify_capi.cpp -> lib/libomni_host_verify.so: the C entry points of KeyframePipeline::Config::batch_verify (keyframe_pipeline.hpp, verify_plan.hpp).
// A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_verify.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
omni::KeyframePipeline& pipe(omni_pipeline* h, const char* who) {
    if (!h) throw std::invalid_argument(std::string(who) + ": null pipeline");
    return *h->p;
}
}  // namespace

extern "C" {

const char* omni_verify_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_batch_verify(omni_pipeline* h, int on) {
    try { pipe(h, "omni_pipeline_set_batch_verify").set_batch_verify(on != 0); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_batch_verify(omni_pipeline* h, int* on) {
    try {
        if (!on) throw std::invalid_argument("omni_pipeline_get_batch_verify: null argument");
        *on = pipe(h, "omni_pipeline_get_batch_verify").batch_verify() ? 1 : 0;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_verify_stats(omni_pipeline* h, int64_t out[4]) {
    try {
        if (!out) throw std::invalid_argument("omni_pipeline_verify_stats: null argument");
        pipe(h, "omni_pipeline_verify_stats").verify_stats(out);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int64_t omni_pipeline_edge_ids(omni_pipeline* h, int64_t* out, int64_t max) {
    if (!h) return -1;
    const auto& e = h->p->edges();
    for (int64_t i = 0; out && i < (int64_t)e.size() && i < max; ++i) out[i] = e[(size_t)i].id;
    return (int64_t)e.size();
}

int omni_pipeline_corr_stats(omni_pipeline* h, int64_t out[2]) {
    try {
        if (!out) throw std::invalid_argument("omni_pipeline_corr_stats: null argument");
        pipe(h, "omni_pipeline_corr_stats").corr_stats(out);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_verify_correspond_host(const omni_corr_io* io, int cand, int max_dirs, int main_dir_new, int main_dir_old, const uint8_t* step_present, const double* old_quat,
                                double* dq_old_out, float* X, float* u, int32_t* n_corr, int32_t* result, int32_t* size_gate, int32_t* new_idx, int32_t* old_idx,
                                int32_t* n_pair_corr) {
    try {
        if (!io || !io->cands || !step_present || !old_quat || !dq_old_out || !X || !u || !n_corr || !result || !size_gate || !new_idx || !old_idx || !n_pair_corr)
            throw std::invalid_argument("omni_verify_correspond_host: null argument");
        if (const char* why = omni::corr::refusal(io->n_cands, io->n_pairs, io->max_n, io->cap, io->cands)) throw std::invalid_argument(std::string("omni_verify_correspond_host: ") + why);
        if (cand < 0 || cand >= io->n_cands || max_dirs < 1 || max_dirs > omni::corr::kMaxPairs || main_dir_new < 0 || main_dir_new >= max_dirs || main_dir_old < 0 ||
            main_dir_old >= max_dirs)
            throw std::invalid_argument("omni_verify_correspond_host: a candidate or a direction out of range");
        const omni_corr_cand& cd = io->cands[cand];
        int present = 0;
        for (int s = 0; s < max_dirs; ++s) present += step_present[s] != 0;
        if (present != cd.pair_count) throw std::invalid_argument("omni_verify_correspond_host: step_present does not name pair_count steps");
        const size_t mn = (size_t)io->max_n;
        omni::FisheyeFrameDescriptor nw, old;
        nw.images.resize((size_t)max_dirs); old.images.resize((size_t)max_dirs);
        for (int d = 0; d < max_dirs; ++d) {
            omni::PoseMsg e;
            for (int k = 0; k < 4; ++k) e.quat_wxyz[k] = old_quat[4 * d + k];
            old.images[(size_t)d].camera_extrinsic = e;
        }
        std::map<const float*, int> pair_of;                      // the new image's descriptor block -> the io's pair
        for (int s = 0, j = 0; s < max_dirs; ++s) {
            if (!step_present[s]) continue;
            const int p = cd.pair_first + j++;
            if (io->hg_status[p] == OMNI_HG_HOST) throw std::invalid_argument("omni_verify_correspond_host: a pair with status OMNI_HG_HOST");
            if (io->nq[p] < 1 || io->nt[p] < 1 || io->nq[p] > io->max_n || io->nt[p] > io->max_n || io->n_flags[p] < 0 || io->n_flags[p] > io->max_n || io->n_matches[p] < 0 ||
                io->n_matches[p] > io->max_n)
                throw std::invalid_argument("omni_verify_correspond_host: a pair's sizes are out of range");
            int dn, dold;
            omni::corr::pair_dirs(main_dir_new, main_dir_old, max_dirs, s, &dn, &dold);
            omni::ImageDescriptor &x = nw.images[(size_t)dn], &y = old.images[(size_t)dold];
            const size_t nq = (size_t)io->nq[p], nt = (size_t)io->nt[p];
            x.landmark_num = (int)nq; y.landmark_num = (int)nt;
            x.landmarks_2d.assign(nq, {}); x.landmarks_2d_norm.assign(nq, {}); x.landmarks_3d.resize(nq); x.feature_descriptor.assign(nq * 4, 0.f);
            x.landmarks_flag.assign(io->q_flags + p * mn, io->q_flags + p * mn + io->n_flags[p]);
            for (size_t i = 0; i < nq; ++i) x.landmarks_3d[i] = {io->q_3d[3 * (p * mn + i)], io->q_3d[3 * (p * mn + i) + 1], io->q_3d[3 * (p * mn + i) + 2]};
            y.landmarks_2d.assign(nt, {}); y.landmarks_3d.assign(nt, {}); y.landmarks_2d_norm.resize(nt); y.feature_descriptor.assign(nt * 4, 0.f);
            for (size_t i = 0; i < nt; ++i) y.landmarks_2d_norm[i] = {io->t_norm[2 * (p * mn + i)], io->t_norm[2 * (p * mn + i) + 1]};
            pair_of[x.feature_descriptor.data()] = p;
        }
        omni::LoopGeometry g;
        g.MAX_DIRS = max_dirs; g.MIN_MATCH_PRE_DIR = cd.min_match_pre_dir; g.MIN_DIRECTION_LOOP = cd.min_direction_loop; g.MIN_LOOP_NUM = cd.min_loop_num;
        g.INIT_MODE_MIN_LOOP_NUM = cd.init_mode_min_loop_num;
        g.match = [&](const float* q, int, const float*, int, int, std::vector<omni::DMatch>& out) {
            out.clear();
            const int p = pair_of.at(q);
            for (int i = 0; i < io->n_matches[p]; ++i) out.push_back({io->q_idx[p * mn + (size_t)i], io->t_idx[p * mn + (size_t)i], 0.f});
        };
        g.homography_mask = [&](const omni::ImageDescriptor& x, const omni::ImageDescriptor&, const std::vector<omni::geom::Vec2>& old_2d, const std::vector<omni::geom::Vec2>&,
                                std::vector<uint8_t>& mask) {
            const int p = pair_of.at(x.feature_descriptor.data());
            mask.assign(io->mask + p * mn, io->mask + p * mn + old_2d.size());
            return true;
        };
        omni::LoopGeometry::Correspondence c;
        const bool ok = g.compute_correspond_features(nw, old, main_dir_new, main_dir_old, c);
        const size_t n = c.new_norm_2d.size();
        if (n > (size_t)io->cap || c.new_3d.size() != n || c.old_norm_2d.size() != n || c.new_idx.size() != (size_t)cd.pair_count)
            throw std::logic_error("omni_verify_correspond_host: the correspondence does not have the candidate's shape");
        const omni::geom::Quat main_quat_old = omni::to_pose(old.images[(size_t)main_dir_old].camera_extrinsic).att;
        for (int j = 0; j < cd.pair_count; ++j) {
            const omni::geom::Quat dq = main_quat_old.inverse() * omni::to_pose(old.images[(size_t)c.dirs_old[(size_t)j]].camera_extrinsic).att;
            dq_old_out[4 * j] = dq.w; dq_old_out[4 * j + 1] = dq.x; dq_old_out[4 * j + 2] = dq.y; dq_old_out[4 * j + 3] = dq.z;
            n_pair_corr[j] = (int32_t)c.new_idx[(size_t)j].size();
            for (size_t k = 0; k < c.new_idx[(size_t)j].size(); ++k) { new_idx[(size_t)j * mn + k] = c.new_idx[(size_t)j][k]; old_idx[(size_t)j * mn + k] = c.old_idx[(size_t)j][k]; }
        }
        for (size_t i = 0; i < n; ++i) {
            X[3 * i] = (float)c.new_3d[i].x; X[3 * i + 1] = (float)c.new_3d[i].y; X[3 * i + 2] = (float)c.new_3d[i].z;      // (float-valued already: exact)
            u[2 * i] = (float)c.old_norm_2d[i].x; u[2 * i + 1] = (float)c.old_norm_2d[i].y;
        }
        *n_corr = (int32_t)n; *result = ok ? 1 : 0;
        *size_gate = ((int)n > g.MIN_LOOP_NUM || (cd.init_mode != 0 && (int)n > g.INIT_MODE_MIN_LOOP_NUM)) ? 1 : 0;      // loop_geometry.hpp compute_loop_core
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_verify_plan(int self_id, int64_t T, int64_t n_frames, const int32_t* drone, const int32_t* partner, const int32_t* partner_init, const uint8_t* verdict,
                     const int64_t* batch_len, int64_t n_batches, int32_t* init_mode_out, int32_t* resolved_before_out, int32_t* end_resolve_out, int64_t* count_out,
                     int n_drones) {
    try {
        if (n_frames < 0 || n_batches < 0 || n_drones < 0) throw std::invalid_argument("omni_verify_plan: a negative size");
        if ((n_frames > 0 && (!drone || !partner || !partner_init || !verdict || !init_mode_out || !resolved_before_out)) || (n_batches > 0 && (!batch_len || !end_resolve_out)) ||
            (n_drones > 0 && !count_out))
            throw std::invalid_argument("omni_verify_plan: null argument");
        int64_t sum = 0;
        for (int64_t b = 0; b < n_batches; ++b) { if (batch_len[b] < 0) throw std::invalid_argument("omni_verify_plan: a negative batch length"); sum += batch_len[b]; }
        if (sum != n_frames) throw std::invalid_argument("omni_verify_plan: the batch lengths do not add up to n_frames");
        auto known = [n_drones](int d) { return d >= 0 && d < n_drones; };
        if (n_frames > 0 && !known(self_id)) throw std::invalid_argument("omni_verify_plan: self_id outside 0 .. n_drones - 1");
        std::vector<omni::VerifyFrame> frames((size_t)n_frames);
        for (int64_t i = 0; i < n_frames; ++i) {
            if (!known(drone[i]) || (partner[i] != -1 && !known(partner[i])) || (partner_init[i] != -1 && !known(partner_init[i])))
                throw std::invalid_argument("omni_verify_plan: a drone outside 0 .. n_drones - 1");
            frames[(size_t)i] = {drone[i], partner[i], partner_init[i], verdict[i] != 0};
        }
        std::map<int, int64_t> count;
        int64_t at = 0;
        for (int64_t b = 0; b < n_batches; ++b) {
            bool end_resolve = false;
            const std::vector<omni::VerifyStep> steps = omni::verify_plan_batch(self_id, T, frames.data() + at, batch_len[b], count, &end_resolve);
            for (size_t s = 0; s < steps.size(); ++s) { init_mode_out[at + (int64_t)s] = steps[s].init_mode; resolved_before_out[at + (int64_t)s] = steps[s].resolved_before; }
            end_resolve_out[b] = end_resolve;
            at += batch_len[b];
        }
        for (int x = 0; x < n_drones; ++x) { const auto it = count.find(x); count_out[x] = it == count.end() ? 0 : it->second; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
