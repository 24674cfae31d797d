// host_camera_capi.cpp -> lib/libomni_host_camera.so: the C entry points of KeyframePipeline::Config::camera_model (keyframe_pipeline.hpp, camera_model.hpp)
// and of the camodocal file reader.  A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same
// (host_capi_types.hpp).
#include <map>
#include <string>

#include "host_capi_types.hpp"
#include "swarm_loop_params.hpp"
#include "omni_host_camera.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* omni_camera_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_camera_model(omni_pipeline* h, const omni_camera_model* model, const double* intrinsics4) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_set_camera_model: null pipeline");
        h->p->set_camera_model(model ? *model : omni::cam::ideal(), intrinsics4);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_camera_model(omni_pipeline* h, omni_camera_model* model_out, double* intrinsics4_out) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_get_camera_model: null pipeline");
        const omni::CameraModel c = h->p->camera();
        if (model_out) *model_out = c.model;
        if (intrinsics4_out) { intrinsics4_out[0] = c.fx; intrinsics4_out[1] = c.fy; intrinsics4_out[2] = c.cx; intrinsics4_out[3] = c.cy; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_camera_from_yaml(const char* yaml_text, int width, int height, omni_camera_model* model_out, double* intrinsics4_out, int* image_size2_out) {
    try {
        if (!yaml_text) throw std::invalid_argument("omni_camera_from_yaml: null text");
        const omni::CameraModel file = omni::CameraModel::from_camodocal_yaml(yaml_text);
        const omni::CameraModel c = width > 0 && height > 0 ? file.scaled(width, height) : file;
        if (model_out) *model_out = c.model;
        if (intrinsics4_out) { intrinsics4_out[0] = c.fx; intrinsics4_out[1] = c.fy; intrinsics4_out[2] = c.cx; intrinsics4_out[3] = c.cy; }
        if (image_size2_out) { image_size2_out[0] = file.image_width; image_size2_out[1] = file.image_height; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

omni_pipeline* omni_pipeline_create_from_launch_camera(int device, const char* launch_xml, const char* node_name, const char* args, const char* sp_weights,
                                                       const char* vlad_weights, const char* pca_comp_csv, const char* pca_mean_csv, int precision, int microbatch,
                                                       int pipelines, int storage, int geometry, const char* camera_yaml) {
    try {
        if (!launch_xml || !sp_weights || !vlad_weights) throw std::invalid_argument("omni_pipeline_create_from_launch_camera: null argument");
        std::map<std::string, std::string> av;
        if (args) {
            const std::string a(args);
            size_t i = 0;
            while (i < a.size()) {
                size_t j = a.find('\n', i);
                if (j == std::string::npos) j = a.size();
                const std::string item = a.substr(i, j - i);
                const size_t k = item.find(":=");
                if (k != std::string::npos) av[item.substr(0, k)] = item.substr(k + 2);
                i = j + 1;
            }
        }
        omni::SwarmLoopParams p = omni::SwarmLoopParams::from_launch(launch_xml, node_name ? node_name : "swarm_loop", av);
        if (p.camera_configuration != 1 && p.camera_configuration != 2)
            throw std::runtime_error("camera_configuration " + std::to_string(p.camera_configuration) + ": a launch file configures STEREO_FISHEYE (1) and PINHOLE_DEPTH (2); "
                                     "STEREO_PINHOLE (0): omni_pipeline_create_stereo_pinhole (omni_host_stereo.h), then omni_pipeline_set_camera_model");
        if (camera_yaml) p.read_camera_config(camera_yaml);
        omni::KeyframePipeline::Config c;
        c.cx = p.width / 2.0; c.cy = p.height / 2.0; c.fx = c.fy = p.width / 2.0;      // (without a camera file: 90 degrees, as omni_pipeline_create_from_launch)
        p.to_pipeline_config(c);
        c.device = device; c.sp_weights = sp_weights; c.vlad_weights = vlad_weights; c.precision = precision; c.microbatch = microbatch; c.pipelines = pipelines;
        c.storage = storage; c.geometry = geometry != 0;
        if (pca_comp_csv) c.pca_comp = pca_comp_csv;
        if (pca_mean_csv) c.pca_mean = pca_mean_csv;
        auto* pl = new omni::KeyframePipeline(c);
        try { pl->apply_params(p); } catch (...) { delete pl; throw; }
        return new omni_pipeline{pl};
    } catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

int omni_pipeline_frame_landmarks(omni_pipeline* h, int64_t msg_id, int direction, int max_n, int* n, float* landmarks_2d, float* landmarks_2d_norm, float* landmarks_3d,
                                  uint8_t* landmarks_flag) {
    try {
        if (!h || !n) throw std::invalid_argument("omni_pipeline_frame_landmarks: null argument");
        const auto& db = h->p->detector().fisheyeframe_database;
        const auto it = db.find(msg_id);
        if (it == db.end()) throw std::out_of_range("omni_pipeline_frame_landmarks: key frame " + std::to_string(msg_id) + " is not in the database");
        if (direction < 0 || direction >= (int)it->second.images.size()) throw std::out_of_range("omni_pipeline_frame_landmarks: no such direction");
        const omni::ImageDescriptor& im = it->second.images[(size_t)direction];
        const size_t k = im.landmarks_2d.size();
        *n = (int)k;
        if ((int)k > max_n) return 0;
        for (size_t i = 0; i < k; ++i) {
            if (landmarks_2d) { landmarks_2d[2 * i] = im.landmarks_2d[i].x; landmarks_2d[2 * i + 1] = im.landmarks_2d[i].y; }
            if (landmarks_2d_norm && i < im.landmarks_2d_norm.size()) { landmarks_2d_norm[2 * i] = im.landmarks_2d_norm[i].x; landmarks_2d_norm[2 * i + 1] = im.landmarks_2d_norm[i].y; }
            if (landmarks_3d && i < im.landmarks_3d.size()) { landmarks_3d[3 * i] = im.landmarks_3d[i].x; landmarks_3d[3 * i + 1] = im.landmarks_3d[i].y; landmarks_3d[3 * i + 2] = im.landmarks_3d[i].z; }
            if (landmarks_flag && i < im.landmarks_flag.size()) landmarks_flag[i] = im.landmarks_flag[i];
        }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
