// keyframe_pipeline.hpp -- the per-key-frame host flow of SwarmLoop::VIOKF_callback (swarm_loop/src/swarm_loop.cpp:140-170:
//     ret = loop_cam->on_flattened_images(stereoframe, imgs);  ...  loop_detector->on_image_recv(ret, imgs);)
// as a C++17 driver over the adapters of omni_swarm.hpp, for a STREAM of key frames: `pipelines` micro-batches of `microbatch` key
// frames are in flight on the GPU (each an omni_cam unit: upload + SuperPoint + MobileNetVLAD + up/down BF + one D2H), while the host
// hands the finished ones to LoopDetectorCore::on_images_recv_batch in arrival order.  The reference does the same work strictly
// serially, one blocking engine call at a time.  This is the host loop bench.py times (through host_capi.cpp); Python only
// prepares the synthetic inputs and brackets the run with the barrier.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <future>
#include <memory>
#include <thread>

#include "../csrc/corr_plan.h"
#include "../csrc/stream_plan.h"
#include "../csrc/wire_plan.h"
#include "camera_model.hpp"
#include "fisheye_flatten.hpp"
#include "loop_geometry.hpp"
#include "loop_net_wire.hpp"
#include "loop_outlier_rejection.hpp"
#include "omni_swarm.hpp"
#include "pose_graph.hpp"
#include "remote_queue.hpp"

namespace omni {

// fixed pool of host threads for the geometry stage (one candidate per task)
class TaskPool {
public:
    explicit TaskPool(int n) {
        for (int i = 0; i < n; ++i)
            workers_.emplace_back([this] {
                for (;;) {
                    std::function<void()> job;
                    {
                        std::unique_lock<std::mutex> lk(mu_);
                        cv_.wait(lk, [this] { return stop_ || !jobs_.empty(); });
                        if (stop_ && jobs_.empty()) return;
                        job = std::move(jobs_.front());
                        jobs_.pop_front();
                    }
                    job();
                }
            });
    }
    ~TaskPool() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    template <typename F> auto submit(F&& f) -> std::future<decltype(f())> {
        auto task = std::make_shared<std::packaged_task<decltype(f())()>>(std::forward<F>(f));
        auto fut = task->get_future();
        { std::lock_guard<std::mutex> lk(mu_); jobs_.emplace_back([task] { (*task)(); }); }
        cv_.notify_one();
        return fut;
    }
    int size() const { return (int)workers_.size(); }
private:
    std::vector<std::thread> workers_;
    std::deque<std::function<void()>> jobs_;
    std::mutex mu_;
    std::condition_variable cv_;
    bool stop_ = false;
};

class KeyframePipeline {
public:
    // Config::wire_img_desc (include/omni_host_wire_messages.h OMNI_WIRE_IMG_*)
    enum { WIRE_IMG_OFF = 0, WIRE_IMG_IMAGE = 1, WIRE_IMG_WHOLE = 2, WIRE_IMG_PC_REPLAY = 3 };
    static constexpr size_t REMOTE_IMAGES_MAX = 64;       // received images kept for take_remote_image; beyond it the oldest is dropped and counted
    struct Config {
        int device = 0, width = 600, height = 480, max_num = 200, precision = OMNI_PREC_F16;
        float thres = 0.02f;
        int microbatch = 8, pipelines = 0 /* units in flight; <= 0: default_pipelines(precision) */, storage = OMNI_STORE_F32, self_id = 1;
        double inner_product_thres = 0.3, init_mode_product_thres = 0.2;
        int match_index_dist = 5, min_loop_num = 30, min_direction_loop = 3;
        std::string sp_weights, pca_comp, pca_mean, vlad_weights;
        // geometric verification (f64, host): lift the key points of the flattened pinhole views, triangulate up/down matches
        // (loop_cam.cpp:397-444, 558-569) and hand every candidate to LoopGeometry::compute_loop (loop_detector.cpp:627-836)
        bool geometry = false;
        double fx = 300, fy = 300, cx = 300, cy = 240, triangle_thres = 0.006, stereo_baseline = 0.10;
        int accept_min_3d_pts = 50;
        // the lens behind fx fy cx cy (camera_model.hpp, csrc/camera_plan.h): camodocal's PINHOLE with distortion coefficients or MEI (fx fy cx cy then hold
        // gamma1 gamma2 u0 v0), what the reference's camera_config_path file describes.  Every lift goes through it -- the message's landmarks_2d_norm, the
        // triangulation's double lift on either path, PINHOLE_DEPTH's depth landmarks.  Default: the ideal pinhole.  The raw-fisheye mode flattens into ideal
        // views and refuses anything else.  (set_camera_model: before the first key frame.)
        omni_camera_model camera_model = cam::ideal();
        // STEREO_FISHEYE / STEREO_PINHOLE with `geometry`: the lifting and the up/down triangulation of generate_stereo_image_descriptor (loop_cam.cpp:397-444) run
        // inside the key-frame unit, f64 on the GPU (csrc/landmarks.hip: bit-identical to the host functions, tests/test_gpu_landmarks.py), and finish() copies the
        // landmarks out of the unit's result block instead of submitting one triangulation task per direction.  Off: the host path (fill_stereo_landmarks on the
        // geometry pool).  PINHOLE_DEPTH has a switch of its own, below.  (set_device_landmarks: before the first key frame.)
        bool device_landmarks = true;
        // PINHOLE_DEPTH with `geometry`: the lift of every key point and the depth landmarks of generate_gray_depth_image_descriptor (loop_cam.cpp:260-304) run inside
        // the key-frame unit, f64 on the GPU (csrc/depth_landmarks.hip: bit-identical to fill_image_descriptor + fill_depth_landmarks, tests/test_gpu_depth_landmarks.py);
        // the unit's depth frames are COPIED at push_keyframe / taken out of set_depth's range at enqueue and go up with the unit, and finish() copies the landmarks
        // out of the unit's result block.  Off (the default: DESIGN.md section 0.2k has the measurements): the host path, both functions inline on the calling thread,
        // the depth frames borrowed until the unit is finished.  (set_device_depth_landmarks: before the first key frame.)
        bool device_depth_landmarks = false;
        // OUTPUT_RAW_SUPERPOINT_DESC (loop_cam.cpp:51-53, 577-582) as a calibration mode: every lane owns a PCA-fit accumulator in HBM attached to its SuperPoint
        // handle (omni_sp_set_pcafit, csrc/pca_fit.hip), so the 256-d descriptors of every key point of the stream enter the fit's moments without leaving the GPU;
        // pca_fit_moments / pca_fit / pca_fit_write read them, and components_.csv / mean_.csv come out of the library instead of a notebook.  Results of the
        // pipeline are the same with the switch on or off.  Off by default.  The sharded database refuses it.  (set_fit_pca: before the first key frame.)
        bool fit_pca = false;
        // The LoopNet wire (host/loop_net_wire.hpp; swarm_loop/src/loop_net.cpp).  `wire`: the pipeline owns a LoopNetWire; every finished local key frame's
        // packets -- LoopNet::broadcast_fisheye_desc of its message -- are kept in order until take_packets hands them out, and packets of other drones enter
        // through recv_packet / scan_recv: every frame the wire completes goes through flush() + on_remote_frame.  `device_wire`: the packets are packed inside
        // the key-frame unit on the GPU (csrc/wire_pack.hip) and finish() copies them and numbers them in the wire's own id sequence, instead of running
        // broadcast_fisheye_desc on the calling thread; the same bytes either way.  It packs the landmarks the device made: it needs device_landmarks or
        // device_depth_landmarks in effect and is refused otherwise, as on the sharded database, which builds no messages.  send_all_features: LoopNet's
        // SEND_ALL_FEATURES.  All off by default.  (set_wire: before the first key frame.)
        bool wire = false, device_wire = false, send_all_features = false;
        // LoopNet's other two message kinds on the same wire (loop_net.cpp:9-10).  `wire_img_desc`: which images also leave as a whole ImageDescriptor_t
        // (SWARM_LOOP_IMG_DES, loop_net.cpp:37-41, 103-116) -- WIRE_IMG_IMAGE: behind an image's landmark packets, without the 64-d descriptors, with the JPEG file
        // (LoopNet's send_img; refused unless send_img is in effect); WIRE_IMG_WHOLE: with the descriptors (send_whole_img_desc), and with the file exactly when
        // send_img is in effect; WIRE_IMG_PC_REPLAY: the whole descriptor ALONE, no header and landmark packets (is_pc_replay).  With device_wire the packet is
        // packed inside the unit (wire_pack_image_kernel), out of its arrays and the file its JPEG stage left in HBM; the same bytes either way.
        // `wire_loop_conn`: every edge that enters edges() leaves as a SWARM_LOOP_CONN packet (loop_net.cpp:122-127), an outbox entry of its own; edges of other
        // drones arrive in remote_edges().  Both off by default.  (set_wire_messages: before the first key frame, with the wire on; not on the sharded database.)
        int wire_img_desc = 0;
        bool wire_loop_conn = false;
        // Remote key frames join the unit stream.  Off (the default): every frame the wire completes goes through flush() + on_remote_frame -- the units in flight
        // are waited for, the frame's four global descriptors go up in four blocking copies and its search is waited for.  On: the frame is QUEUED
        // (queue_remote_frame; drain_inbox does it for the wire's frames) with p, the number of local key frames handed over before it, and the next key-frame
        // unit's detector batch takes it at its place in the serial order (host/remote_queue.hpp): its rows are gathered with the unit's on the GPU
        // (csrc/rows_assemble.hip; LoopDetectorCore's mixed batch) and its verdict is replayed with the unit's.  With no local key frame around, queue_remote_frame,
        // poll() and flush() begin a batch of remote frames alone.  Candidates, edges, counters and rows are the serial flow's.  The sharded database, which builds
        // no messages, refuses it.  (set_remote_in_stream: before the first key frame.)
        bool remote_in_stream = false;
        // `geometry`: inter-drone loop candidates are verified with their batch.  Off (the default): a candidate between a frame of another drone and a frame of
        // this one is verified on the spot -- its own matcher + homography round trip, its own PnP on one pool thread -- because the detector reads the verdict for
        // the init-mode counters.  On: such a candidate is deferred like one between two frames of this drone, and everything deferred is verified in ONE round trip
        // when the detector's batch ends -- or earlier, in front of a remote frame whose mode depends on a pending verdict (host/verify_plan.hpp; only around the
        // crossing of inter_drone_init_frames).  Candidates, edges and their ids, counters and rows are the switch-off flow's.  Independent of remote_in_stream; the
        // sharded database, which builds no messages, refuses it.  (set_batch_verify: between two calls, while no detector batch is pending.)
        bool batch_verify = false;
        // `geometry`: pairwise-consistency outlier rejection of the loop edges (SwarmLocalOutlierRejection::OutlierRejectionLoopEdges, swarm_localization/src/
        // swarm_outlier_rejection/swarm_outlier_rejection.cpp:98-298; host/loop_outlier_rejection.hpp).  Every edge that enters edges() or remote_edges() is compared
        // with every earlier edge of its drone pair on the GPU (csrc/pcm.hip; the arithmetic is csrc/pcm_plan.h's), the clique heuristic runs on the host, and
        // good_edges() lists the edges that agree with each other.  The stage only ADDS an output: edges(), candidates, counters and rows are what they are without
        // it.  pcm_thres: the reference's default (swarm_localization_node.cpp:475); pcm_redundant: every drone pair is evaluated, not only those with this drone at
        // one end (:122-139); pcm_capacity: edges per drone pair (a multiple of 64 in 64..32768).  The odometry covariance per metre of path is the reference's
        // swarm_loop.cpp:247-248.  Off by default.  The sharded database, which builds no messages, refuses it.  (set_pcm: before the first key frame.)
        bool pcm = false, pcm_redundant = false;
        double pcm_thres = 0.6, pcm_pos_covariance_per_meter = 0.01, pcm_yaw_covariance_per_meter = 0.003;
        int pcm_capacity = OMNI_PCM_DEFAULT_CAPACITY;
        // The 4-DoF pose graph over the window's ego motion and loop edges (host/pose_graph.hpp builds it, csrc/pgo.hip solves it; the loop + ego-motion part of
        // swarm_localization_solver.cpp:1064-1213, :1668-1712): optimize() solves the last pose_graph_window key frames per drone (the reference's max_keyframe_num
        // is 50, swarm_localization_node.cpp:465; 2..256) with the edges good_edges() returns, from pose_graph_starts initial pose sets (1..64).  The stage only adds
        // outputs -- estimated_poses(), drift(), pose_graph_stats().  Off by default; refused on the sharded database and without a geometry stage, like pcm.
        bool pose_graph = false;
        int pose_graph_window = 50, pose_graph_starts = 1;
        // `geometry`: the homography RANSAC of every direction pair of a loop candidate (compute_correspond_features, loop_detector.cpp:589-598) runs on the GPU, in
        // the round trip that matches the pairs anyway (omni_bf_match_homography_multi, csrc/homography.hip: the same mask bit for bit, tests/test_gpu_homography.py);
        // the candidate's host task takes the masks instead of running geom::find_homography_ransac -- 2 000 f64 9 x 9 eigen-solves per pair of a candidate
        // that is NOT a loop.  A pair the device hands back (degenerate points: status HOST) runs on the host as before.  Off: the host path for every pair.
        // On by default: DESIGN.md section 0.2b has the gates and the measurements.  (set_device_homography: any time between two calls.)
        bool device_homography = true;
        // `geometry`: the RANSAC half of compute_relative_pose's solvePnPRansac (loop_detector.cpp:390-391: 100 EPnP hypotheses, 1 000 in init_mode) runs on the
        // GPU (omni_pnp_ransac_multi, csrc/pnp.hip: the same mask and best model bit for bit, tests/test_gpu_pnp.py), one blocking call per candidate from its
        // geometry task on a context of its own; the refit (geom::pnp_refit) stays in the task.  A candidate the device hands back (status HOST) or that has more
        // points than the entry takes runs geom::solve_pnp_ransac as before.  OFF by default: DESIGN.md section 0.2d has the measurements a later change will
        // decide on.  (set_device_pnp: any time between two calls.)
        bool device_pnp = false;
        // send_img (swarm_loop.cpp:224-225; launch/pc-outdoor-fisheye.launch sets it with jpg_quality 75): the main image of every direction goes into its message as
        // a JPEG file (encode_image, loop_cam.cpp:56-71, 306-308, 463-469), encoded inside the key-frame unit on the GPU (csrc/jpeg.hip) and copied by finish() into
        // ImageDescriptor::image.  The bytes are libjpeg's defaults, pinned against Pillow (csrc/jpeg_plan.h); cv::imencode's own parity is unpinned.  The fisheye
        // mask reaches the picture, as in the reference.  jpeg_capacity: bytes per image in the unit's result block (<= 0: width * height / 2); an image that does
        // not fit leaves `image` empty and counts in jpeg_truncated().  (set_send_img: before the first key frame.)
        bool send_img = false;
        // is_compressed_images (the VINS settings file, swarm_loop.cpp:291-292, 303-304): the camera frames arrive as JPEG files (sensor_msgs::CompressedImage; every
        // frame through cv::imdecode(data, IMREAD_GRAYSCALE), :72-89) and are decoded on the GPU inside the key-frame unit, in front of the resize
        // (omni_cam_enqueue_jpeg_host; csrc/jpeg_dec.hip).  A key frame then carries (pointer, size) pairs instead of pixel pointers, in push_keyframe and in
        // run().  STEREO_PINHOLE, PINHOLE_DEPTH and STEREO_FISHEYE's raw-fisheye mode (below): a flattened-view STEREO_FISHEYE pipeline ignores the switch (the
        // reference has no compressed path for it), and so does the sharded
        // mode.  A frame that cannot be decoded comes out all zeros -- no key points, landmark_num 0 -- and counts in jpeg_corrupt().
        bool compressed_images = false;
        int jpg_quality = 50;
        int64_t jpeg_capacity = 0;
        // CameraConfig (loop_defines.h:111-116): STEREO_FISHEYE = 1 -- a key frame is 4 directions x (up, down) flattened views, the bottom quarter of
        // every view blanked; PINHOLE_DEPTH = 2 (launch/realsense.launch, BASELINE.json configs[0]: 640 x 480) -- a key frame is ONE gray image, not
        // blanked, plus its 16-bit depth image in millimetres (set_depth), MAX_DIRS = 1 (swarm_loop.cpp:279-280), the query image is direction 0
        // (loop_detector.cpp:252-258) and the landmarks are read from the depth image (loop_cam.cpp:260-304)
        int camera_configuration = 1;
        double depth_near = 0.3, depth_far = 10.0;      // DEPTH_NEAR_THRES / DEPTH_FAR_THRES: the reference's own defaults (swarm_loop.cpp:251-252; launch/realsense.launch sets 0.3 / 100)
        // The streaming intake's latency bound (push_keyframe / poll).  The reference reports a key frame's loop synchronously (swarm_loop.cpp:140-170); a
        // micro-batch that only left for the GPU when `microbatch` key frames had arrived would, at the reference's 1 Hz key-frame rate (max_freq), hold a key
        // frame for seconds.  So: (1) dispatch_when_idle: a key frame that arrives while NO unit is in flight goes to the GPU at once, as a unit of one --
        // batches only grow while the GPU is busy anyway (adaptive batching: full throughput under load, one frame's compute time when idle);
        // (2) max_wait_ms: a partly filled micro-batch older than this is sent as it is by the next push_keyframe() or poll() (< 0: never -- only flush()).
        bool dispatch_when_idle = true;
        double max_wait_ms = 50.0;
        // STEREO_PINHOLE = 0 (loop_cam.cpp:189-196: generate_stereo_image_descriptor for ONE direction): a key frame is a left and a right image, the left camera in
        // the role of the up camera (both networks) and the right one in the role of the down camera (SuperPoint, stereo match), not blanked, MAX_DIRS = 1, the
        // query image is direction 0.  src_width x src_height > 0: the frames arrive at the CAMERA's size and are resized to width x height inside the unit
        // (omni_cam_enqueue_raw_*: the cv::resize of superpoint_tensorrt.cpp:123-125 on the GPU); 0: they have the networks' size already.  Key points stay in
        // network-image coordinates and are lifted as they are (loop_cam.cpp:558-569): fx fy cx cy are those of the width x height image.
        int src_width = 0, src_height = 0;
        // body -> camera of the two cameras (xyz + quaternion wxyz; swarm_loop.cpp:294-306 body_T_cam0 / body_T_cam1).  Defaults: the forward camera of
        // PINHOLE_DEPTH, and the same displaced by stereo_baseline along its own x axis (to its right)
        bool have_stereo_extrinsics = false;
        double left_extrinsic[7] = {0, 0, 0, 1, 0, 0, 0}, right_extrinsic[7] = {0, 0, 0, 1, 0, 0, 0};
        // STEREO_FISHEYE = 1 with fisheye_src_width x fisheye_src_height > 0, the raw-fisheye mode: a key frame is ONE up frame and ONE down frame of the fisheye
        // camera's size instead of 8 flattened views, and the flattening (the reference's upstream does it: VINS-Fisheye's FisheyeUndist publishes flattened_gray;
        // the reference itself has no such path) runs inside the key-frame unit (omni_cam_enqueue_fisheye_*; csrc/flatten.hip).  The two cameras' maps are made at
        // construction by generate_all_undist_maps(MEI model, width, fisheye_fov_deg, camera 0 / 1): their four side views, views fisheye_first_view.., must be
        // width x height.  fisheye_mei_*: xi k1 k2 p1 p2 gamma1 gamma2 u0 v0, the order omni_fisheye_maps takes.  With compressed_images the two frames are
        // JPEG files, decoded in front of the flattening (omni_cam_enqueue_fisheye_jpeg_host).
        int fisheye_src_width = 0, fisheye_src_height = 0;
        double fisheye_fov_deg = 235.0;
        double fisheye_mei_up[9] = {0, 0, 0, 0, 0, 1, 1, 0, 0}, fisheye_mei_down[9] = {0, 0, 0, 0, 0, 1, 1, 0, 0};
        int fisheye_first_view = 1;
        // what the camera configuration decides, one question each
        bool stereo() const { return camera_configuration != 2; }      // two cameras per direction: up / down (left / right), stereo match, triangulated landmarks
        int dirs() const { return camera_configuration == 1 ? 4 : 1; }
        bool masked() const { return camera_configuration == 1; }       // loop_cam.cpp:536 blanks rows for STEREO_FISHEYE only; its query image is direction 1
        bool resized() const { return camera_configuration == 0 && src_width > 0; }              // camera-size stereo-pinhole frames: resized inside the unit
        bool fisheye_raw() const { return camera_configuration == 1 && fisheye_src_width > 0; }   // raw fisheye frames: flattened inside the unit
        bool raw() const { return resized() || fisheye_raw(); }         // the caller hands over the camera's frames, not network-size images
        int in_width() const { return fisheye_raw() ? fisheye_src_width : (resized() ? src_width : width); }      // the size of the images a caller hands over
        int in_height() const { return fisheye_raw() ? fisheye_src_height : (resized() ? src_height : height); }
        int frames_per_keyframe() const { return fisheye_raw() ? 2 : (stereo() ? 2 : 1) * dirs(); }       // ... and how many of them make a key frame
        int frames_per_camera() const { return fisheye_raw() ? 1 : dirs(); }
        // compressed_images as the mode takes it: a flattened-view STEREO_FISHEYE pipeline ignores the switch (the sharded database too: KeyframePipeline::compressed)
        bool compressed() const { return compressed_images && (camera_configuration != 1 || fisheye_raw()); }
    };

    // units in flight when the caller does not say: fp16's small-grid tails (NMS, sampling, matcher, MobileNetVLAD's last blocks) are filled by the next
    // units' kernels, so four pay; the fp32-class modes are CU-filling convolutions end to end and gain nothing beyond two
    static int default_pipelines(int precision) { return precision == OMNI_PREC_F16 ? omni::STREAM_PLAN_DEFAULT_PIPELINES : 2; }
    static Config resolved(Config c) {
        if (c.camera_configuration < 0 || c.camera_configuration > 2)
            throw std::runtime_error("KeyframePipeline: camera_configuration must be 0 (STEREO_PINHOLE), 1 (STEREO_FISHEYE) or 2 (PINHOLE_DEPTH)");
        if ((c.src_width > 0) != (c.src_height > 0) || (c.src_width > 0 && c.camera_configuration != 0))
            throw std::runtime_error("KeyframePipeline: src_width x src_height (frames resized inside the unit) belongs to camera_configuration 0 (STEREO_PINHOLE), both or neither");
        if ((c.fisheye_src_width > 0) != (c.fisheye_src_height > 0) || c.fisheye_src_width < 0 || (c.fisheye_src_width > 0 && c.camera_configuration != 1))
            throw std::runtime_error("KeyframePipeline: fisheye_src_width x fisheye_src_height (raw fisheye frames flattened inside the unit) belongs to camera_configuration 1 (STEREO_FISHEYE), both or neither");
        if (c.fisheye_raw()) {
            // generate_all_undist_maps makes one top view and, for a field of view above 180 degrees, four side views of width x side_view_height
            const int side_h = side_view_height((unsigned)c.width, c.fisheye_fov_deg), n_views = side_h > 0 ? 5 : 1;
            if (c.fisheye_first_view < 0 || n_views != c.fisheye_first_view + 4)
                throw std::runtime_error("KeyframePipeline: raw-fisheye mode needs fisheye_first_view + 4 = " + std::to_string(c.fisheye_first_view + 4) + " views, a field of view of " +
                                         std::to_string(c.fisheye_fov_deg) + " degrees gives " + std::to_string(n_views));
            if (side_h != c.height)
                throw std::runtime_error("KeyframePipeline: raw-fisheye mode: the side views are " + std::to_string(c.width) + " x " + std::to_string(side_h) + " but the networks take " +
                                         std::to_string(c.width) + " x " + std::to_string(c.height));
        }
        check_camera_model(c, c.camera_model);
        if (c.pipelines <= 0) c.pipelines = default_pipelines(c.precision);
        return c;
    }
    // what cam::check refuses, and a lens in the one mode whose views are ideal by construction
    static void check_camera_model(const Config& c, const omni_camera_model& m) {
        if (const char* why = cam::check(m)) throw std::runtime_error(std::string("KeyframePipeline: ") + why);
        if (c.fisheye_raw() && !cam::is_ideal(m))
            throw std::runtime_error("KeyframePipeline: the raw-fisheye mode flattens the frames into ideal pinhole views inside the unit, so its key points have no lens to undo: "
                                     "camera_model must stay the ideal pinhole (the fisheye lens itself is fisheye_mei_up / fisheye_mei_down)");
    }
    int pipelines() const { return cfg_.pipelines; }
    int microbatch() const { return cfg_.microbatch; }
    bool stereo_rig() const { return cfg_.stereo(); }
    bool fisheye_raw() const { return cfg_.fisheye_raw(); }
    int in_width() const { return cfg_.in_width(); }       // the size of the images a caller hands over
    int in_height() const { return cfg_.in_height(); }

    explicit KeyframePipeline(const Config& c0) : KeyframePipeline(resolved(c0), 0) {}
private:
    KeyframePipeline(const Config& c, int) : cfg_(c), index_ctx_(c.device, true), det_(index_ctx_, c.self_id, c.storage) {
        det_.INNER_PRODUCT_THRES = c.inner_product_thres; det_.INIT_MODE_PRODUCT_THRES = c.init_mode_product_thres;
        det_.MATCH_INDEX_DIST = c.match_index_dist; det_.MIN_LOOP_NUM = c.min_loop_num; det_.MIN_DIRECTION_LOOP = c.min_direction_loop;
        det_.stereo_fisheye = c.masked();
        geo_.MAX_DIRS = c.dirs();
        for (int p = 0; p < c.pipelines; ++p) lanes_.push_back(std::make_unique<Lane>(c, c.microbatch));
        apply_fit_pca();
        if (c.fisheye_raw()) {
            // ONE pair of flatten objects serves every lane: omni_cam_enqueue_fisheye_* launches the remap on the UNIT's stream and only reads the maps and the
            // view table (flatten_unit_launch, csrc/flatten.hip: neither the object's own stream nor its lock), which nothing writes after omni_flatten_create
            for (int cam = 0; cam < 2; ++cam) {
                const double* p = cam ? c.fisheye_mei_down : c.fisheye_mei_up;
                MeiCamera mei;
                mei.xi = p[0]; mei.k1 = p[1]; mei.k2 = p[2]; mei.p1 = p[3]; mei.p2 = p[4]; mei.gamma1 = p[5]; mei.gamma2 = p[6]; mei.u0 = p[7]; mei.v0 = p[8];
                const FlattenMaps maps = generate_all_undist_maps(mei, (unsigned)c.width, c.fisheye_fov_deg, cam);
                if ((int)maps.w.size() != c.fisheye_first_view + 4) throw std::runtime_error("KeyframePipeline: raw-fisheye mode: the maps have " + std::to_string(maps.w.size()) + " views");
                for (size_t v = (size_t)c.fisheye_first_view; v < maps.w.size(); ++v)
                    if (maps.w[v] != c.width || maps.h[v] != c.height) throw std::runtime_error("KeyframePipeline: raw-fisheye mode: a side view is not width x height");
                flatten_[cam] = std::make_unique<FlattenHIP>(index_ctx_, c.fisheye_src_width, c.fisheye_src_height, maps.w, maps.h, maps.xy);
            }
        }
        apply_stereo_model();
        apply_jpeg();
        if (c.wire) { const bool dw = c.device_wire; cfg_.wire = cfg_.device_wire = false; set_wire(true, dw, c.send_all_features); }
        cfg_.wire_img_desc = 0; cfg_.wire_loop_conn = false;
        if (c.wire_img_desc || c.wire_loop_conn) set_wire_messages(c.wire_img_desc, c.wire_loop_conn);
        if (c.device_pnp) ensure_pnp_context();
        if (c.geometry) {
            geo_.self_id = c.self_id; geo_.MIN_LOOP_NUM = c.min_loop_num; geo_.MIN_DIRECTION_LOOP = c.min_direction_loop;
            // Per candidate: (1) on this thread, the up to four direction pairs of compute_correspond_features (loop_detector.cpp:431-537) are
            // matched in ONE GPU round trip (the matcher is a pure function of its two descriptor sets); (2) the rest of compute_loop -- flag
            // filter, homography-RANSAC mask, PnP-RANSAC + refit, verification: f64, milliseconds -- runs as a task on a pool of host threads,
            // its per-pair match() calls served from (1).  Tasks of one micro-batch run side by side; finish() collects them IN CANDIDATE ORDER,
            // so edges, their ids and the on_loop order are those of the serial flow.  The detector itself only needs compute_loop's verdict for
            // the init-mode counters of REMOTE drones (inter_drone_loop_count, loop_detector.cpp:66-72,826-827): candidates between two frames
            // of the self drone are deferred, anything else is verified on the spot.
            {
                int nt = -1;                                            // (the library's one table of switches: csrc/config.h)
                check(omni_config_value("OMNI_GEOMETRY_THREADS", &nt), "omni_config_value");
                if (nt < 0) nt = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency() / 2));
                if (nt > 0) pool_ = std::make_unique<TaskPool>(nt);
            }
            det_.compute_loop = [this](const FisheyeFrameDescriptor& a, const FisheyeFrameDescriptor& b, int da, int db, bool im) {
                ++geometry_calls_;
                if (a.drone_id == cfg_.self_id && b.drone_id == cfg_.self_id) {      // verdict not needed by the detector: deferred to collect_geometry()
                    // CONTRACT: for a candidate between two frames of the self drone the callback returns false HERE, whatever the verdict will be:
                    // LoopCandidate::loop of the detector's record stays false and inter_drone_loop_count[{self, self}] is not counted by the detector (the
                    // reference counts it, loop_detector.cpp:826-827, and never reads it: init mode only exists for OTHER drones, :66-72).  The verdict is
                    // the edge: edges() / geometry_stats() hold it once the micro-batch's tasks are drained, and drain_geometry() adds the count then.
                    deferred_.push_back({&a, &b, da, db, im});
                    return false;
                }
                collect_geometry();                                     // keep the order: everything deferred earlier comes first
                deferred_.push_back({&a, &b, da, db, im});
                const size_t before = edges_.size();
                collect_geometry();
                return edges_.size() > before;
            };
            if (c.batch_verify) apply_batch_verify(true);
        }
        if (c.pcm) { cfg_.pcm = false; set_pcm(true, c.pcm_thres, c.pcm_redundant, c.pcm_capacity); }
        if (c.pose_graph) { cfg_.pose_graph = false; set_pose_graph(true, c.pose_graph_window, c.pose_graph_starts); }
    }
    // Config::batch_verify: the detector's late-verdict hooks.  A ticket is a place in deferred_; a resolve is one start_geometry + drain_geometry over everything
    // deferred so far -- the candidates between two frames of this drone that came before included, so the edge order is the candidate order
    void apply_batch_verify(bool on) {
        if (!on) { det_.defer_loop = nullptr; det_.resolve_loops = nullptr; return; }
        det_.defer_loop = [this](const FisheyeFrameDescriptor& a, const FisheyeFrameDescriptor& b, int da, int db, bool im) {
            ++geometry_calls_;
            deferred_.push_back({&a, &b, da, db, im, true});
            return verify_deferred_++;
        };
        det_.resolve_loops = [this] {
            drain_geometry();                                       // what earlier batches left running comes first
            verdicts_.clear();
            const int64_t before = matcher_round_trips_;
            start_geometry(nullptr);
            drain_geometry();
            verify_round_trips_ += matcher_round_trips_ - before;
            return std::move(verdicts_);
        };
    }
public:
    bool batch_verify() const { return cfg_.batch_verify; }
    // between two calls, while no detector batch is pending (what the C entry point omni_pipeline_set_batch_verify sets)
    void set_batch_verify(bool on) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (on && shard_) throw std::runtime_error("set_batch_verify: the sharded database builds no messages");
        if (on && !cfg_.geometry) throw std::runtime_error("set_batch_verify: the pipeline has no geometry stage");
        if (det_pending_.active || !deferred_.empty()) throw std::runtime_error("set_batch_verify: a detector batch is pending (flush first)");
        cfg_.batch_verify = on;
        apply_batch_verify(on);
    }
    // ---- pairwise-consistency outlier rejection of the loop edges (Config::pcm) ---------------------------------------------------------------------------------
    bool pcm() const { return cfg_.pcm; }
    double pcm_thres() const { return cfg_.pcm_thres; }
    bool pcm_redundant() const { return cfg_.pcm_redundant; }
    int pcm_capacity() const { return cfg_.pcm_capacity; }
    // before the first key frame (what the C entry point omni_pipeline_set_pcm sets)
    void set_pcm(bool on, double thres, bool redundant, int capacity) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (any_keyframe_seen_) throw std::runtime_error("set_pcm after the first key frame");
        if (on && shard_) throw std::runtime_error("set_pcm: the sharded database builds no messages");
        if (on && !cfg_.geometry) throw std::runtime_error("set_pcm: the pipeline has no geometry stage");
        if (on && !(thres > 0)) throw std::invalid_argument("set_pcm: pcm_thres must be positive");
        if (!on) { pcm_.reset(); pcm_ctx_.reset(); cfg_.pcm = false; return; }
        LoopOutlierRejection::Params p;
        p.self_id = cfg_.self_id; p.redundant = redundant; p.capacity = capacity;
        p.pcm = omni_pcm_params{thres, cfg_.pcm_pos_covariance_per_meter, cfg_.pcm_yaw_covariance_per_meter};
        // omni_pcm_add is blocking: a stream of its own, not the detector's, and a high-priority one -- short work the host waits on next to units that fill the GPU
        if (!pcm_ctx_) pcm_ctx_ = std::make_unique<Context>(cfg_.device, true);
        pcm_ = std::make_unique<LoopOutlierRejection>(pcm_ctx_->get(), p);       // (refuses the capacity)
        cfg_.pcm = true; cfg_.pcm_thres = thres; cfg_.pcm_redundant = redundant; cfg_.pcm_capacity = capacity;
    }
    // edges() and remote_edges(), in that order, without those the stage rejected.  An edge one of whose frames this pipeline never saw is outside the graph and
    // passes.  Without the stage: all of them.
    std::vector<LoopEdge> good_edges() {
        std::lock_guard<std::mutex> lk(intake_mu_);
        pcm_feed();
        std::vector<LoopEdge> out;
        for (const std::vector<LoopEdge>* v : {&edges_, &remote_edges_})
            for (const LoopEdge& e : *v)
                if (!pcm_ || pcm_outside_.count(e.id) || pcm_->good(e.id, e.drone_id_a, e.drone_id_b)) out.push_back(e);
        return out;
    }
    // [0] edges entered, [1] pairs evaluated, [2] consistent pairs, [3] clique runs, [4] edges left out because the pipeline never saw one of their frames, [5] edges
    // that met a full handle
    void pcm_stats(int64_t out[6]) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        pcm_feed();
        for (int i = 0; i < 6; ++i) out[i] = pcm_ ? pcm_->stats().v[i] : 0;
        out[4] = pcm_unknown_;
    }
    // the records the stage entered so far, in the order they entered (what a host recomputation takes: tests)
    const std::vector<omni_pcm_edge>& pcm_records() { std::lock_guard<std::mutex> lk(intake_mu_); pcm_feed(); return pcm_records_; }

    // ---- the 4-DoF pose graph of the window (Config::pose_graph) -------------------------------------------------------------------------------------------------
    struct EstimatedPose { int drone = 0, pose_index = -1; int64_t keyframe_id = 0; double pose[4] = {0, 0, 0, 0}, odom[4] = {0, 0, 0, 0}, init[4] = {0, 0, 0, 0}; };
    // [0] optimize() calls, [1] poses, [2] ego-motion edges, [3] loop edges, [4] loop edges outside the window, [5] drones no edge reaches, [6] key frames merged
    // into their predecessor's pose, [7] the best start (-1: none), [8] its status (OMNI_PGO_*), [9] its outer iterations, [10] its conjugate-gradient steps -- all
    // of the last call; cost: its initial and final cost
    struct PoseGraphStats { int64_t v[11] = {0, 0, 0, 0, 0, 0, 0, -1, OMNI_PGO_EMPTY, 0, 0}; double cost[2] = {0, 0}; };
    bool pose_graph() const { return cfg_.pose_graph; }
    int pose_graph_window() const { return cfg_.pose_graph_window; }
    int pose_graph_starts() const { return cfg_.pose_graph_starts; }
    // before the first key frame (what the C entry point omni_pipeline_set_pose_graph sets)
    void set_pose_graph(bool on, int window, int starts) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (any_keyframe_seen_) throw std::runtime_error("set_pose_graph after the first key frame");
        if (on && shard_) throw std::runtime_error("set_pose_graph: the sharded database builds no messages");
        if (on && !cfg_.geometry) throw std::runtime_error("set_pose_graph: the pipeline has no geometry stage");
        if (on && (window < SwarmPoseGraph::kMinWindow || window > SwarmPoseGraph::kMaxWindow)) throw std::invalid_argument("set_pose_graph: pose_graph_window outside 2..256");
        if (on && (starts < 1 || starts > OMNI_PGO_MAX_STARTS)) throw std::invalid_argument("set_pose_graph: pose_graph_starts outside 1..64");
        if (pg_handle_) { omni_pgo_destroy(pg_handle_); pg_handle_ = nullptr; }
        pg_.reset();
        if (!on) { pg_ctx_.reset(); cfg_.pose_graph = false; return; }
        SwarmPoseGraph::Params p;
        p.self_id = cfg_.self_id; p.window = window; p.starts = starts;
        p.pos_covariance_per_meter = cfg_.pcm_pos_covariance_per_meter; p.yaw_covariance_per_meter = cfg_.pcm_yaw_covariance_per_meter;
        // omni_pgo_solve_multi is blocking: a context of its own, as for pcm
        if (!pg_ctx_) pg_ctx_ = std::make_unique<Context>(cfg_.device, true);
        if (omni_pgo_create(pg_ctx_->get(), &pg_handle_) != OMNI_OK) throw std::runtime_error(std::string("omni_pgo_create: ") + omni_last_error());
        pg_ = std::make_unique<SwarmPoseGraph>(p);
        cfg_.pose_graph = true; cfg_.pose_graph_window = window; cfg_.pose_graph_starts = starts;
    }
    // Solves the current window (blocking): the problem host/pose_graph.hpp builds from the key frames seen so far and good_edges(), on the GPU, every start a
    // workgroup; the cheapest start's poses are what estimated_poses() returns.  Returns that start's status (OMNI_PGO_*).
    int optimize() {
        if (!cfg_.pose_graph) throw std::runtime_error("optimize: the pose graph is off");
        const std::vector<LoopEdge> good = good_edges();
        std::lock_guard<std::mutex> lk(intake_mu_);
        std::vector<SwarmPoseGraph::Loop> loops;
        for (const LoopEdge& e : good) {
            SwarmPoseGraph::Loop l;
            l.id = e.id; l.drone_a = e.drone_id_a; l.drone_b = e.drone_id_b; l.keyframe_a = e.keyframe_id_a; l.keyframe_b = e.keyframe_id_b;
            l.rel[0] = e.relative_pose.pos.x; l.rel[1] = e.relative_pose.pos.y; l.rel[2] = e.relative_pose.pos.z;
            l.rel[3] = e.relative_pose.att.w; l.rel[4] = e.relative_pose.att.x; l.rel[5] = e.relative_pose.att.y; l.rel[6] = e.relative_pose.att.z;
            for (int k = 0; k < 3; ++k) { l.pos_cov[k] = e.pos_cov[k]; l.ang_cov[k] = e.ang_cov[k]; }
            loops.push_back(l);
        }
        pg_problem_ = pg_->build(loops);
        const SwarmPoseGraph::Problem& P = pg_problem_;
        PoseGraphStats st;
        st.v[0] = pg_stats_.v[0] + 1;
        st.v[1] = P.n_poses; st.v[2] = P.ego_edges; st.v[3] = P.loop_edges; st.v[4] = P.loops_outside; st.v[5] = P.unreachable_drones; st.v[6] = P.merged;
        pg_solution_.assign(P.poses.begin(), P.poses.begin() + (long)(4 * (size_t)P.n_poses));
        if (P.n_poses > 0) {
            std::vector<double> out(P.poses.size());
            std::vector<omni_pgo_stats> ss((size_t)P.n_starts);
            const omni_pgo_params pr = pg_params_;
            int best = -1;
            if (omni_pgo_solve_multi(pg_handle_, &pr, P.poses.data(), P.fixed.data(), P.edges.data(), P.n_poses, (int)P.edges.size(), P.n_starts, out.data(), ss.data(), &best,
                                     nullptr) != OMNI_OK)
                throw std::runtime_error(std::string("omni_pgo_solve_multi: ") + omni_last_error());
            const int use = best >= 0 ? best : 0;
            st.v[7] = best; st.v[8] = ss[(size_t)use].status; st.v[9] = ss[(size_t)use].iterations; st.v[10] = ss[(size_t)use].cg_iterations;
            st.cost[0] = ss[(size_t)use].initial_cost; st.cost[1] = ss[(size_t)use].final_cost;
            pg_solution_.assign(out.begin() + (long)(4 * (size_t)P.n_poses * (size_t)use), out.begin() + (long)(4 * (size_t)P.n_poses * (size_t)(use + 1)));
        }
        pg_stats_ = st;
        return (int)st.v[8];
    }
    // every window key frame of the last optimize(), drones ascending, oldest first: the estimate, the odometry pose and the initial value (start 0), x y z yaw, and
    // the pose of the problem the frame maps to -- one locked call, so that a reader never sees two optimize() calls mixed
    std::vector<EstimatedPose> estimated_poses() {
        std::lock_guard<std::mutex> lk(intake_mu_);
        std::vector<EstimatedPose> out;
        for (const SwarmPoseGraph::Frame& f : pg_problem_.frames) {
            EstimatedPose e;
            e.drone = f.drone; e.pose_index = f.pose_index; e.keyframe_id = f.keyframe_id;
            for (int k = 0; k < 4; ++k) { e.pose[k] = pg_solution_[4 * (size_t)f.pose_index + (size_t)k]; e.odom[k] = f.odom[k]; e.init[k] = f.init[k]; }
            out.push_back(e);
        }
        return out;
    }
    // this drone's newest estimated pose . inverse(its odometry pose), x y z yaw; false when the last optimize() held no frame of this drone
    bool drift(double out[4]) {
        const std::vector<EstimatedPose> est = estimated_poses();
        const EstimatedPose* last = nullptr;
        for (const EstimatedPose& e : est) if (e.drone == cfg_.self_id) last = &e;
        if (!last) return false;
        double inv[4];
        pgo::pose_inverse(last->odom, inv);
        pgo::pose_mul(last->pose, inv, out);
        return true;
    }
    PoseGraphStats pose_graph_stats() { std::lock_guard<std::mutex> lk(intake_mu_); return pg_stats_; }
    // the exact problem the last optimize() solved (what a host recomputation takes: tests), and the solver's parameters
    SwarmPoseGraph::Problem pose_graph_problem() { std::lock_guard<std::mutex> lk(intake_mu_); return pg_problem_; }
    omni_pgo_params pose_graph_params() { std::lock_guard<std::mutex> lk(intake_mu_); return pg_params_; }
private:
    // the cumulative path length of a drone at the key frames this pipeline saw, local and remote, from their pose_drone in the order they came
    void pcm_note_frame(int drone, int64_t kf_id, const PoseMsg& pose) {
        if (pg_) {                                                   // Config::pose_graph reads the same key frames
            const double p7[7] = {pose.position[0], pose.position[1], pose.position[2], pose.quat_wxyz[0], pose.quat_wxyz[1], pose.quat_wxyz[2], pose.quat_wxyz[3]};
            pg_->note_frame(drone, kf_id, p7);
        }
        if (!pcm_) return;
        PcmPath& t = pcm_path_[drone];
        if (t.any) { const double dx = pose.position[0] - t.last[0], dy = pose.position[1] - t.last[1], dz = pose.position[2] - t.last[2]; t.length += std::sqrt(dx * dx + dy * dy + dz * dz); }
        t.any = true; t.last[0] = pose.position[0]; t.last[1] = pose.position[1]; t.last[2] = pose.position[2];
        pcm_arc_[{drone, kf_id}] = t.length;
    }
    // the new edges of edges() and remote_edges() enter the stage: after every detector batch and every drained inbox, and before the stage's outputs are read
    void pcm_feed() {
        if (!pcm_ || (pcm_fed_local_ == edges_.size() && pcm_fed_remote_ == remote_edges_.size())) return;
        std::vector<omni_pcm_edge> batch;
        auto put = [](double* o, const geom::Pose& q) { o[0] = q.pos.x; o[1] = q.pos.y; o[2] = q.pos.z; o[3] = q.att.w; o[4] = q.att.x; o[5] = q.att.y; o[6] = q.att.z; };
        auto take = [&](const std::vector<LoopEdge>& v, size_t& fed) {
            for (; fed < v.size(); ++fed) {
                const LoopEdge& e = v[fed];
                const auto a = pcm_arc_.find({e.drone_id_a, e.keyframe_id_a}), b = pcm_arc_.find({e.drone_id_b, e.keyframe_id_b});
                if (a == pcm_arc_.end() || b == pcm_arc_.end()) { ++pcm_unknown_; pcm_outside_.insert(e.id); continue; }
                omni_pcm_edge r;
                r.id = e.id; r.drone_a = e.drone_id_a; r.drone_b = e.drone_id_b;
                put(r.relative_pose, e.relative_pose); put(r.self_pose_a, e.self_pose_a); put(r.self_pose_b, e.self_pose_b);
                r.arc_a = a->second; r.arc_b = b->second;
                for (int k = 0; k < 3; ++k) { r.pos_cov[k] = e.pos_cov[k]; r.ang_cov[k] = e.ang_cov[k]; }
                batch.push_back(r);
            }
        };
        take(edges_, pcm_fed_local_);
        take(remote_edges_, pcm_fed_remote_);
        if (batch.empty()) return;
        pcm_records_.insert(pcm_records_.end(), batch.begin(), batch.end());
        pcm_->add(batch);
    }
public:
    // [0] inter-drone candidates deferred, [1] resolves at the end of a detector batch (a frame outside a batch is a batch of one), [2] early resolves forced by
    // the rule, [3] matcher round trips spent on [1] and [2]
    // candidates whose correspondences the round trip assembled so far, and candidates it handed back to the host functions
    void corr_stats(int64_t out[2]) const { out[0] = corr_candidates_device_; out[1] = corr_candidates_host_; }
    void verify_stats(int64_t out[4]) const { out[0] = verify_deferred_; out[1] = det_.end_resolves; out[2] = det_.early_resolves; out[3] = verify_round_trips_; }
    // The geometry of every deferred candidate: (1) ONE GPU round trip matches the direction pairs of all of them (compute_correspond_features
    // pairs up to four directions per candidate, loop_detector.cpp:431-537; the matcher is a pure function of its two descriptor sets);
    // (2) one task per candidate on the pool: flag filter, homography-RANSAC masks, PnP-RANSAC + refit, verification (f64), its match() calls
    // served from (1); (3) the accepted edges are numbered and appended in candidate order.
    // start_geometry() does (1) and submits (2); drain_geometry() does (3).  finish() leaves a micro-batch's tasks running while the host
    // waits for the NEXT micro-batch's CNN unit and drains them before it starts that one's geometry: batches are drained in the order they
    // were started and candidates in the order the detector returned them, so edges, ids and latencies are those of the serial flow.
    void collect_geometry() { drain_geometry(); start_geometry(nullptr); drain_geometry(); }
    void drain_geometry() {
        while (!geo_inflight_.empty()) {
            GeoBatch& gb = geo_inflight_.front();
            for (size_t fi = 0; fi < gb.futs.size(); ++fi) {
                std::pair<bool, LoopEdge> r = gb.futs[fi].get();
                if (r.first) {
                    geo_.number_edge(r.second); edges_.push_back(r.second);
                    if (cfg_.wire_loop_conn && net_) queue_loop_conn(edges_.back());
                    if (fi < gb.self_self.size() && gb.self_self[fi]) det_.inter_drone_loop_count[{cfg_.self_id, cfg_.self_id}] += 2;      // what the detector would have counted (:826-827, both orders)
                }
                if (fi < gb.verdict.size() && gb.verdict[fi]) verdicts_.push_back(r.first ? 1 : 0);      // batch_verify: the detector's ticket, in candidate order
            }
            if (gb.timed) latencies_ms_.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - gb.t_enqueue).count());
            geo_inflight_.pop_front();
        }
    }
    // held: frames of the micro-batch that were not moved into the database (the tasks point into them); t_enqueue: its latency is recorded
    // when its last task has been collected.  Returns true when tasks were left in flight.
    bool start_geometry(std::vector<FisheyeFrameDescriptor>* held, const std::chrono::steady_clock::time_point* t_enqueue = nullptr) {
        if (deferred_.empty()) return false;
        struct Prepared { size_t first = 0, count = 0; };
        std::vector<BFMatcherL2X::Pair> pairs;
        std::vector<BFMatcherL2X::PairH> pairs_h;                    // device_homography: the same pairs with their 2-D points and flags
        const bool dev_hg = device_homography();
        PnPRansacX* const dev_pnp = device_pnp() ? pnp_.get() : nullptr;      // (lives as long as the pipeline once made: the tasks may keep the pointer)
        std::vector<int> pair_dim;                                   // descriptor length of every pair (one match_multi call per distinct length)
        std::vector<Prepared> prep(deferred_.size());
        const int nd = geo_.MAX_DIRS;
        // batch_verify with device_homography: the correspondences of every candidate the entry takes are assembled behind the homography masks in the same round
        // trip (BFMatcherL2X::match_homography_corr_multi, csrc/corr_assemble.hip), and its task starts at compute_relative_pose.  A candidate with a pair that was
        // not listed (malformed descriptors, an image without key points), with pairs of different descriptor lengths, with more points than the entry takes or
        // with landmark arrays shorter than its key points goes through the path above
        const bool corr_on = cfg_.batch_verify && dev_hg;
        std::vector<char> corr_ok(deferred_.size(), 0);
        std::vector<BFMatcherL2X::PairC> pairs_c;                    // corr_on: pairs_h with the gathers' sources (same positions)
        for (size_t ci = 0; ci < deferred_.size(); ++ci) {
            const FisheyeFrameDescriptor &a = *deferred_[ci].a, &b = *deferred_[ci].b;
            const int da = deferred_[ci].da, db = deferred_[ci].db;
            prep[ci].first = pairs.size();
            for (int d = da; d < da + nd; ++d) {                       // the pairing rule of compute_correspond_features (frame pair)
                const int dn = d % nd, dold = ((db - da + nd) % nd + d) % nd;
                if (dn < (int)a.images.size() && dold < (int)b.images.size() && b.images[dold].landmark_num > 0 && a.images[dn].landmark_num > 0) {
                    const ImageDescriptor &x = a.images[dn], &y = b.images[dold];
                    const int nx = (int)x.landmarks_2d.size(), ny = (int)y.landmarks_2d.size();
                    if (nx > 0 && ny > 0 && x.feature_descriptor.size() % nx == 0) {
                        const int dim = (int)(x.feature_descriptor.size() / nx);
                        if (dim > 0 && (int)y.feature_descriptor.size() == ny * dim) {
                            pairs.push_back({x.feature_descriptor.data(), nx, y.feature_descriptor.data(), ny}); pair_dim.push_back(dim);
                            if (dev_hg) pairs_h.push_back({x.feature_descriptor.data(), nx, y.feature_descriptor.data(), ny, &x.landmarks_2d[0].x, &y.landmarks_2d[0].x,
                                                           x.landmarks_flag.data(), (int)std::min(x.landmarks_flag.size(), (size_t)nx)});
                        }
                    }
                }
            }
            prep[ci].count = pairs.size() - prep[ci].first;
            if (corr_on) {
                int wanted = 0;
                bool ok = da >= 0 && db >= 0 && da < (int)a.images.size() && db < (int)b.images.size();
                const geom::Quat main_quat_old = ok ? to_pose(b.images[db].camera_extrinsic).att : geom::Quat{};
                size_t at = prep[ci].first;
                for (int s = 0; s < nd; ++s) {
                    int dn, dold;
                    corr::pair_dirs(da, db, nd, s, &dn, &dold);
                    if (!(dn < (int)a.images.size() && dold < (int)b.images.size() && b.images[dold].landmark_num > 0 && a.images[dn].landmark_num > 0)) continue;
                    ++wanted;
                    const ImageDescriptor &x = a.images[dn], &y = b.images[dold];
                    // (the pairs were listed above in this order: the pair at `at` is this one, or one is missing and the candidate is not served)
                    if (!ok || at >= prep[ci].first + prep[ci].count || pairs[at].query != x.feature_descriptor.data() || pairs[at].train != y.feature_descriptor.data() ||
                        pair_dim[at] != pair_dim[prep[ci].first] || pairs[at].nq > BFMatcherL2X::kMaxPoints || pairs[at].nt > BFMatcherL2X::kMaxPoints ||
                        (int)x.landmarks_3d.size() < pairs[at].nq || (int)x.landmarks_2d_norm.size() < pairs[at].nq || (int)y.landmarks_2d_norm.size() < pairs[at].nt) { ok = false; continue; }
                    const geom::Quat dq = main_quat_old.inverse() * to_pose(y.camera_extrinsic).att;
                    pairs_c.resize(pairs.size());
                    pairs_c[at] = {pairs_h[at], &x.landmarks_3d[0].x, &y.landmarks_2d_norm[0].x, {dq.w, dq.x, dq.y, dq.z}};
                    ++at;
                }
                corr_ok[ci] = ok && wanted >= 1 && wanted <= corr::kMaxPairs && (size_t)wanted == prep[ci].count;
            }
        }
        pairs_c.resize(pairs.size());
        std::vector<std::vector<DMatch>> outs(pairs.size());
        std::vector<BFMatcherL2X::Homography> hgs(dev_hg ? pairs.size() : 0);
        std::vector<std::shared_ptr<BFMatcherL2X::Corr>> corrs(deferred_.size());
        {
            std::vector<char> done(pairs.size(), 0);
            for (size_t c0 = 0; corr_on && c0 < deferred_.size();) {          // whole candidates, one descriptor length, at most 64 pairs and 64 candidates per round trip
                if (!corr_ok[c0]) { ++c0; continue; }
                const int dim = pair_dim[prep[c0].first];
                std::vector<BFMatcherL2X::PairC> sub;
                std::vector<BFMatcherL2X::CandC> cands;
                std::vector<size_t> which;
                size_t c1 = c0;
                for (; c1 < deferred_.size() && cands.size() < (size_t)corr::kMaxCall; ++c1) {
                    if (!corr_ok[c1] || pair_dim[prep[c1].first] != dim) continue;
                    if (sub.size() + prep[c1].count > (size_t)corr::kMaxCall) break;
                    cands.push_back({(int)sub.size(), (int)prep[c1].count, geo_.MIN_MATCH_PRE_DIR, geo_.MIN_DIRECTION_LOOP, geo_.MIN_LOOP_NUM, geo_.INIT_MODE_MIN_LOOP_NUM, deferred_[c1].im});
                    for (size_t j = 0; j < prep[c1].count; ++j) sub.push_back(pairs_c[prep[c1].first + j]);
                    which.push_back(c1);
                    corr_ok[c1] = 0;                                          // (taken)
                }
                std::vector<std::vector<DMatch>> so;
                std::vector<BFMatcherL2X::Homography> sh;
                std::vector<BFMatcherL2X::Corr> sc;
                bf_.match_homography_corr_multi(sub, cands, dim, so, sh, sc);
                ++matcher_round_trips_;
                for (size_t k = 0; k < which.size(); ++k) {
                    const size_t ci = which[k];
                    for (size_t j = 0; j < prep[ci].count; ++j) {
                        const size_t p = prep[ci].first + j;
                        outs[p] = std::move(so[(size_t)cands[k].pair_first + j]); hgs[p] = std::move(sh[(size_t)cands[k].pair_first + j]); done[p] = 1;
                    }
                    corrs[ci] = std::make_shared<BFMatcherL2X::Corr>(std::move(sc[k]));
                }
            }
            for (size_t p0 = 0; p0 < pairs.size(); ++p0) {
                if (done[p0]) continue;
                std::vector<BFMatcherL2X::Pair> sub;
                std::vector<BFMatcherL2X::PairH> sub_h;
                std::vector<size_t> where;
                for (size_t p = p0; p < pairs.size(); ++p)
                    if (!done[p] && pair_dim[p] == pair_dim[p0] && sub.size() < 64) { sub.push_back(pairs[p]); if (dev_hg) sub_h.push_back(pairs_h[p]); where.push_back(p); done[p] = 1; }
                std::vector<std::vector<DMatch>> so;
                std::vector<BFMatcherL2X::Homography> sh;
                if (dev_hg) bf_.match_homography_multi(sub_h, pair_dim[p0], so, sh);
                else bf_.match_multi(sub, pair_dim[p0], so);
                ++matcher_round_trips_;
                for (size_t j = 0; j < where.size(); ++j) { outs[where[j]] = std::move(so[j]); if (dev_hg) hgs[where[j]] = std::move(sh[j]); }
            }
        }
        using Result = std::pair<bool, LoopEdge>;
        geo_inflight_.emplace_back();
        GeoBatch& gb = geo_inflight_.back();
        if (held) gb.held = std::move(*held);                      // (a moved vector keeps its elements where they are)
        if (t_enqueue) { gb.timed = true; gb.t_enqueue = *t_enqueue; }
        std::vector<std::future<Result>>& futs = gb.futs;
        for (size_t ci = 0; ci < deferred_.size(); ++ci) {
            auto mine_p = std::make_shared<std::vector<BFMatcherL2X::Pair>>(pairs.begin() + prep[ci].first, pairs.begin() + prep[ci].first + prep[ci].count);
            auto mine_o = std::make_shared<std::vector<std::vector<DMatch>>>();
            auto mine_d = std::make_shared<std::vector<int>>(pair_dim.begin() + prep[ci].first, pair_dim.begin() + prep[ci].first + prep[ci].count);
            auto mine_h = std::make_shared<std::vector<BFMatcherL2X::Homography>>();
            for (size_t j = 0; j < prep[ci].count; ++j) { mine_o->push_back(std::move(outs[prep[ci].first + j])); if (dev_hg) mine_h->push_back(std::move(hgs[prep[ci].first + j])); }
            const Deferred c = deferred_[ci];
            const std::shared_ptr<BFMatcherL2X::Corr> mine_c = corrs[ci] && corrs[ci]->gate != OMNI_CORR_HOST ? corrs[ci] : nullptr;
            if (corrs[ci]) ++(mine_c ? corr_candidates_device_ : corr_candidates_host_);
            auto work = [this, g0 = geo_, mine_p, mine_o, mine_d, mine_h, mine_c, c, dev_pnp]() -> Result {    // g0: the parameters, copied on this thread
                LoopGeometry g = g0;
                if (mine_c)                                            // the candidate's correspondences from the round trip above: the task starts at compute_relative_pose
                    g.correspondences = [&](const FisheyeFrameDescriptor& nw, const FisheyeFrameDescriptor& old, int main_dir_new, int main_dir_old,
                                            LoopGeometry::Correspondence& cr) {
                        for (int s = 0; s < g.MAX_DIRS; ++s) {
                            int dn, dold;
                            corr::pair_dirs(main_dir_new, main_dir_old, g.MAX_DIRS, s, &dn, &dold);
                            if (dn < (int)nw.images.size() && dold < (int)old.images.size() && old.images[dold].landmark_num > 0 && nw.images[dn].landmark_num > 0) {
                                cr.dirs_new.push_back(dn); cr.dirs_old.push_back(dold);
                            }
                        }
                        if (cr.dirs_new.size() != mine_c->new_idx.size()) return -1;
                        cr.new_idx = mine_c->new_idx; cr.old_idx = mine_c->old_idx;
                        for (int i = 0; i < mine_c->n_corr; ++i) {
                            cr.new_3d.push_back({mine_c->X[3 * i], mine_c->X[3 * i + 1], mine_c->X[3 * i + 2]});
                            cr.old_norm_2d.push_back({mine_c->u[2 * i], mine_c->u[2 * i + 1]});
                        }
                        for (const BFMatcherL2X::Homography& h : *mine_h)      // what homography_mask would have counted, pair by pair
                            if (h.status == OMNI_HG_OK || h.status == OMNI_HG_NO_MODEL) ++homography_pairs_device_;
                        return mine_c->gate == OMNI_CORR_OK ? 1 : 0;
                    };
                if (dev_pnp)                                           // the candidate's PnP RANSAC on the device, from this thread; what it hands back runs on the host
                    g.pnp_ransac = [this, dev_pnp](const std::vector<geom::Vec3>& X, const std::vector<geom::Vec2>& u, int iterations, std::vector<uint8_t>& mask, geom::Rt& best) {
                        const size_t n = X.size();
                        if (n < 6 && u.size() == n) return 0;          // solve_pnp_ransac's `false` without any work: no round trip for it, and it is not counted
                        if (u.size() != n || n > (size_t)PnPRansacX::kMaxPoints) { ++pnp_candidates_host_; return -1; }
                        std::vector<float> Xf(n * 3), uf(n * 2);       // float-valued already (Point3f landmarks, rotate_pt_norm2d's float cast): exact
                        for (size_t i = 0; i < n; ++i) { Xf[3 * i] = (float)X[i].x; Xf[3 * i + 1] = (float)X[i].y; Xf[3 * i + 2] = (float)X[i].z; uf[2 * i] = (float)u[i].x; uf[2 * i + 1] = (float)u[i].y; }
                        std::vector<PnPRansacX::Result> r;
                        dev_pnp->run_multi({{Xf.data(), uf.data(), (int)n, iterations}}, r);
                        if (r[0].status == OMNI_PNP_HOST) { ++pnp_candidates_host_; return -1; }
                        ++pnp_candidates_device_;
                        if (r[0].status != OMNI_PNP_OK) return 0;
                        mask = r[0].mask;
                        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) best.R.m[a][b] = r[0].Rt[3 * a + b];
                        best.t = {r[0].Rt[9], r[0].Rt[10], r[0].Rt[11]};
                        return 1;
                    };
                if (!mine_h->empty())                                  // the pair's mask from the round trip above; a pair the device handed back runs on the host
                    g.homography_mask = [&](const ImageDescriptor& nw, const ImageDescriptor& old, const std::vector<geom::Vec2>& old_2d, const std::vector<geom::Vec2>&,
                                            std::vector<uint8_t>& mask) {
                        for (size_t p = 0; p < mine_p->size(); ++p) {
                            if ((*mine_p)[p].query != nw.feature_descriptor.data() || (*mine_p)[p].train != old.feature_descriptor.data()) continue;
                            const BFMatcherL2X::Homography& h = (*mine_h)[p];
                            if ((h.status != OMNI_HG_OK && h.status != OMNI_HG_NO_MODEL) || h.mask.size() != old_2d.size()) break;
                            mask = h.mask;
                            ++homography_pairs_device_;
                            return true;
                        }
                        ++homography_pairs_host_;
                        return false;
                    };
                g.match = [&](const float* q, int nq, const float* t, int nt, int dim, std::vector<DMatch>& out) {
                    for (size_t p = 0; p < mine_p->size(); ++p)
                        if ((*mine_p)[p].query == q && (*mine_p)[p].train == t && (*mine_p)[p].nq == nq && (*mine_p)[p].nt == nt && (*mine_d)[p] == dim) { out = (*mine_o)[p]; return; }
                    // every pair compute_correspond_features can ask for was listed above (the same rule, whatever its descriptor length); a pair that
                    // was not has malformed descriptors (a length that is not a multiple of its key-point count): no matches
                    out.clear();
                };
                Result r;
                r.first = g.compute_loop_core(*c.a, *c.b, c.da, c.db, r.second, c.im);
                return r;
            };
            gb.self_self.push_back(c.a->drone_id == cfg_.self_id && c.b->drone_id == cfg_.self_id);
            gb.verdict.push_back(c.verdict);
            if (pool_) futs.push_back(pool_->submit(work));
            else { std::promise<Result> pr; pr.set_value(work()); futs.push_back(pr.get_future()); }
        }
        deferred_.clear();
        return true;
    }
    // device time of the two all-gathers of every exchange unit collected so far (microseconds: new rows, per-shard top-k lists); sharded mode only
    const std::vector<std::pair<float, float>>& exchange_us() const { return exchange_us_; }
    void clear_exchange_us() { exchange_us_.clear(); }
    int geometry_calls() const { return geometry_calls_; }
    int last_run_fifo() const { return last_fifo_; }
    // where the host thread's time goes, per unit (micro-batch), in milliseconds since the last reset: [0] enqueue (upload + launches), [1] waiting for
    // the unit's results, [2] building the frame messages (+ stereo landmarks), [3] the detector step (index appends / searches, one GPU round trip),
    // [4] geometry hand-over; returns the number of units.  The loop runs at the GPU's pace while [1] > 0: the host then waits for the GPU, not the GPU for it.
    int host_times(double out[5], bool reset) {
        for (int i = 0; i < 5; ++i) out[i] = host_units_ ? host_ms_[i] / host_units_ : 0.0;
        const int n = host_units_;
        if (reset) { for (double& v : host_ms_) v = 0; host_units_ = 0; }
        return n;
    }
    const std::vector<LoopEdge>& edges() const { return edges_; }
    // every loop candidate the detector returned (query_fisheyeframe_from_database found an old frame), in key-frame order
    struct Candidate { int64_t new_msg_id, old_msg_id; int dir_new, dir_old; };
    const std::vector<Candidate>& candidates() const { return candidates_; }
    // odometry poses of the key frames (VIO's pose_drone, swarm_loop.cpp:140-170 takes it from the key-frame message): key frame msg_id gets
    // poses7[msg_id - first_msg_id] = position xyz + quaternion wxyz; key frames outside the range keep the identity
    PoseMsg pose_of(int64_t kf_id) const { return (kf_id >= pose_base_ && kf_id < pose_base_ + (int64_t)poses_.size()) ? poses_[(size_t)(kf_id - pose_base_)] : PoseMsg{}; }
    void set_poses(int64_t first_msg_id, const double* poses7, int64_t n) {
        pose_base_ = first_msg_id;
        poses_.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            PoseMsg m;
            for (int k = 0; k < 3; ++k) m.position[k] = poses7[i * 7 + k];
            for (int k = 0; k < 4; ++k) m.quat_wxyz[k] = poses7[i * 7 + 3 + k];
            poses_[(size_t)i] = m;
        }
    }
    // extrinsics of the virtual pinhole views of the stacked fisheye pair: direction d looks along the body x axis rotated by 90 deg * d,
    // the up / down cameras sit +- baseline/2 along body z (camera axes: x right, y down, z forward)
    geom::Pose view_extrinsic(int direction, bool up) const {
        if (cfg_.camera_configuration == 0 && cfg_.have_stereo_extrinsics) {      // the rig's own (set_stereo_extrinsics): left = up, right = down
            const double* e = up ? cfg_.left_extrinsic : cfg_.right_extrinsic;
            return {{e[0], e[1], e[2]}, {e[3], e[4], e[5], e[6]}};
        }
        if (cfg_.dirs() == 1) {                             // the one forward-looking camera, at the body origin; STEREO_PINHOLE's right camera stereo_baseline to its right
            geom::Mat3 R;
            R.m[0][0] = 0;  R.m[0][1] = 0;  R.m[0][2] = 1;
            R.m[1][0] = -1; R.m[1][1] = 0;  R.m[1][2] = 0;
            R.m[2][0] = 0;  R.m[2][1] = -1; R.m[2][2] = 0;
            return {{0, (up || !cfg_.stereo()) ? 0.0 : -cfg_.stereo_baseline, 0}, geom::quat_from_R(R)};      // (the camera's x axis is the body's -y)
        }
        const double yaw = M_PI / 2 * direction, c = std::cos(yaw), s = std::sin(yaw);
        geom::Mat3 R;            // Rz(yaw) * [[0,0,1],[-1,0,0],[0,-1,0]]
        R.m[0][0] = s;  R.m[0][1] = 0;  R.m[0][2] = c;
        R.m[1][0] = -c; R.m[1][1] = 0;  R.m[1][2] = s;
        R.m[2][0] = 0;  R.m[2][1] = -1; R.m[2][2] = 0;
        return {{0, 0, (up ? 0.5 : -0.5) * cfg_.stereo_baseline}, geom::quat_from_R(R)};
    }

    // ---- the stereo landmarks inside the key-frame unit (Config::device_landmarks) ----------------------------------------------------------------------
    bool device_landmarks() const { return cfg_.device_landmarks && cfg_.geometry && cfg_.stereo() && !shard_; }      // (the sharded database builds no messages)
    // what every lane's unit is given: the pinhole model, the accept rule and the extrinsics finish() stamps on the messages (as PoseMsg: to_pose normalises them)
    omni_stereo_model stereo_model() const {
        omni_stereo_model m{};
        m.fx = cfg_.fx; m.fy = cfg_.fy; m.cx = cfg_.cx; m.cy = cfg_.cy; m.triangle_thres = cfg_.triangle_thres; m.accept_min_3d_pts = cfg_.accept_min_3d_pts;
        m.dirs_per_keyframe = cfg_.dirs();
        for (int d = 0; d < cfg_.dirs(); ++d)
            for (int up = 0; up < 2; ++up) {
                const PoseMsg e = to_msg(view_extrinsic(d, up != 0));
                double* o = up ? m.up_extrinsic[d] : m.down_extrinsic[d];
                std::copy(e.position, e.position + 3, o); std::copy(e.quat_wxyz, e.quat_wxyz + 4, o + 3);
            }
        return m;
    }
    // ---- PINHOLE_DEPTH's depth landmarks inside the key-frame unit (Config::device_depth_landmarks) ---------------------------------------------------------------
    bool device_depth_landmarks() const { return cfg_.device_depth_landmarks && cfg_.geometry && cfg_.camera_configuration == 2 && !shard_; }      // (the sharded database builds no messages)
    // what every lane's unit is given: the intrinsics, the depth window, the accept rule and the extrinsic finish() stamps on the messages (view 0's, as a PoseMsg);
    // the depth images have the networks' size (the reference reads them at network-size key-point coordinates)
    omni_depth_model depth_model() const {
        omni_depth_model m{};
        m.fx = cfg_.fx; m.fy = cfg_.fy; m.cx = cfg_.cx; m.cy = cfg_.cy; m.depth_near = cfg_.depth_near; m.depth_far = cfg_.depth_far; m.accept_min_3d_pts = cfg_.accept_min_3d_pts;
        m.depth_width = cfg_.width; m.depth_height = cfg_.height;
        const PoseMsg e = to_msg(view_extrinsic(0, true));
        std::copy(e.position, e.position + 3, m.extrinsic); std::copy(e.quat_wxyz, e.quat_wxyz + 4, m.extrinsic + 3);
        return m;
    }
    // before the first key frame: switches the stage on or off on every lane (what the C entry point omni_pipeline_set_device_depth_landmarks sets).  Refused for a
    // stereo camera configuration, which reads no depth image
    void set_device_depth_landmarks(bool on) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (cfg_.camera_configuration != 2) throw std::runtime_error("set_device_depth_landmarks: camera_configuration is not 2 (PINHOLE_DEPTH)");
        if (any_keyframe_seen_) throw std::runtime_error("set_device_depth_landmarks after the first key frame");
        if (!on && cfg_.wire && cfg_.device_wire) throw std::runtime_error("set_device_depth_landmarks(false): device_wire packs the landmarks the device made (set_wire first)");
        cfg_.device_depth_landmarks = on;
        apply_stereo_model();
    }
    bool device_depth_landmarks_config() const { return cfg_.device_depth_landmarks; }      // the switch as set, whatever the mode makes of it
    // ---- the PCA fit of the stream's 256-d descriptors (Config::fit_pca) ------------------------------------------------------------------------------------------
    bool fit_pca() const { return cfg_.fit_pca; }
    // before the first key frame (what the C entry point omni_pipeline_set_fit_pca sets): every lane gets, or gives up, an accumulator of its own -- lanes run on
    // different streams.  Refused on the sharded database, which builds no descriptors of its own
    void set_fit_pca(bool on) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (on && shard_) throw std::runtime_error("set_fit_pca: the sharded database builds no descriptors of its own");
        if (any_keyframe_seen_) throw std::runtime_error("set_fit_pca after the first key frame");
        cfg_.fit_pca = on;
        apply_fit_pca();
    }
    // waits for every lane, then merges the lanes' accumulators: lanes_ in order, then the tail lanes in key order
    PcaMoments pca_fit_moments() {
        if (!cfg_.fit_pca) throw std::runtime_error("pca_fit_moments: the pipeline was made without fit_pca");
        sync();
        PcaMoments m;
        for (auto& l : lanes_) if (l->fit) m.merge(l->fit->moments());
        for (auto& t : tail_lanes_) if (t.second->fit) m.merge(t.second->fit->moments());
        return m;
    }
    PcaSolution pca_fit(int pca_dim = 64) { return pca_solve(pca_fit_moments(), pca_dim); }
    void pca_fit_write(const std::string& comp_path, const std::string& mean_path, int pca_dim = 64) { pca_fit(pca_dim).write(comp_path, mean_path); }
    void pca_fit_reset() {
        if (!cfg_.fit_pca) throw std::runtime_error("pca_fit_reset: the pipeline was made without fit_pca");
        sync();
        for (auto& l : lanes_) if (l->fit) l->fit->reset();
        for (auto& t : tail_lanes_) if (t.second->fit) t.second->fit->reset();
    }
    // ---- the homography RANSAC of the loop candidates on the GPU (Config::device_homography) --------------------------------------------------------------
    bool device_homography() const { return cfg_.device_homography && cfg_.geometry && !shard_; }      // (the sharded database builds no messages)
    bool device_homography_config() const { return cfg_.device_homography; }      // the switch as set, whatever the mode makes of it
    // between two calls of run / push_keyframe / poll / flush (what the C entry point omni_pipeline_set_device_homography sets): the next micro-batch's candidates
    void set_device_homography(bool on) { std::lock_guard<std::mutex> lk(intake_mu_); cfg_.device_homography = on; }
    // direction pairs whose mask came from the device / that ran geom::find_homography_ransac although the switch was on (the device's status HOST), so far
    int homography_pairs_device() const { return homography_pairs_device_.load(); }
    int homography_pairs_host() const { return homography_pairs_host_.load(); }
    // ---- the PnP RANSAC of the loop candidates on the GPU (Config::device_pnp) ------------------------------------------------------------------------------
    bool device_pnp() const { return cfg_.device_pnp && cfg_.geometry && !shard_; }      // (the sharded database builds no messages)
    bool device_pnp_config() const { return cfg_.device_pnp; }      // the switch as set, whatever the mode makes of it
    // between two calls of run / push_keyframe / poll / flush (what the C entry point omni_pipeline_set_device_pnp sets): the next micro-batch's candidates
    void set_device_pnp(bool on) { std::lock_guard<std::mutex> lk(intake_mu_); if (on) ensure_pnp_context(); cfg_.device_pnp = on; }
    // candidates whose RANSAC ran on the device / that ran geom::solve_pnp_ransac although the switch was on (handed back, or too many points), so far
    int pnp_candidates_device() const { return pnp_candidates_device_.load(); }
    int pnp_candidates_host() const { return pnp_candidates_host_.load(); }
    // ---- the lens of every lift (Config::camera_model) ---------------------------------------------------------------------------------------------------
    CameraModel camera() const { CameraModel c; c.model = cfg_.camera_model; c.fx = cfg_.fx; c.fy = cfg_.fy; c.cx = cfg_.cx; c.cy = cfg_.cy; return c; }
    omni_camera_model camera_model() const { return cfg_.camera_model; }
    // before the first key frame (what the C entry point omni_pipeline_set_camera_model sets); intrinsics4 = fx fy cx cy of the network-size image, nullptr: kept
    void set_camera_model(const omni_camera_model& m, const double* intrinsics4 = nullptr) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (any_keyframe_seen_) throw std::runtime_error("set_camera_model after the first key frame");
        check_camera_model(cfg_, m);
        if (intrinsics4 && !(intrinsics4[0] != 0 && intrinsics4[1] != 0 && intrinsics4[0] == intrinsics4[0] && intrinsics4[1] == intrinsics4[1]))
            throw std::invalid_argument("set_camera_model: focal lengths " + std::to_string(intrinsics4[0]) + ", " + std::to_string(intrinsics4[1]));
        cfg_.camera_model = m;
        if (intrinsics4) { cfg_.fx = intrinsics4[0]; cfg_.fy = intrinsics4[1]; cfg_.cx = intrinsics4[2]; cfg_.cy = intrinsics4[3]; }
        apply_stereo_model();
    }
    // before the first key frame: switches the stage on or off on every lane (what the C entry point omni_pipeline_set_device_landmarks sets)
    void set_device_landmarks(bool on) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (any_keyframe_seen_) throw std::runtime_error("set_device_landmarks after the first key frame");
        if (!on && cfg_.wire && cfg_.device_wire && cfg_.stereo()) throw std::runtime_error("set_device_landmarks(false): device_wire packs the landmarks the device made (set_wire first)");
        cfg_.device_landmarks = on;
        apply_stereo_model();
    }
    // ---- is_compressed_images: the frames arrive as JPEG files (Config::compressed_images) ---------------------------------------------------------------
    bool compressed() const { return cfg_.compressed() && !shard_; }
    bool compressed_config() const { return cfg_.compressed_images; }
    int64_t jpeg_corrupt() const { return jpeg_corrupt_.load(); }       // frames whose file could not be decoded so far: their pictures were all zeros
    // before the first key frame (what the C entry point omni_pipeline_set_compressed_images sets)
    void set_compressed_images(bool on) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (any_keyframe_seen_) throw std::runtime_error("set_compressed_images after the first key frame");
        cfg_.compressed_images = on;
    }
    // one JPEG file of a key frame, borrowed for the call
    struct JpegFile { const uint8_t* data = nullptr; int64_t size = 0; };

    // ---- send_img: the main images as JPEG files inside the key-frame unit (Config::send_img) ------------------------------------------------------------
    bool send_img() const { return cfg_.send_img && !shard_; }      // (the sharded database builds no messages: the switch is ignored there, like device_landmarks)
    bool send_img_config() const { return cfg_.send_img; }          // the switch as set, whatever the mode makes of it
    int jpg_quality() const { return cfg_.jpg_quality; }
    int64_t jpeg_capacity() const { return cfg_.jpeg_capacity > 0 ? cfg_.jpeg_capacity : std::max<int64_t>((int64_t)cfg_.width * cfg_.height / 2, OMNI_JPEG_HEADER_BYTES + 2); }
    int64_t jpeg_truncated() const { return jpeg_truncated_.load(); }      // main images whose file did not fit jpeg_capacity(), so far: their `image` stayed empty
    // before the first key frame: switches the stage on or off on every lane (what the C entry point omni_pipeline_set_send_img sets); quality 1..100
    void set_send_img(bool on, int quality) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (any_keyframe_seen_) throw std::runtime_error("set_send_img after the first key frame");
        if (on && (quality < 1 || quality > 100)) throw std::invalid_argument("set_send_img: jpg_quality outside 1..100");
        if (!on && cfg_.wire_img_desc == WIRE_IMG_IMAGE) throw std::runtime_error("set_send_img(false): wire_img_desc IMAGE sends the file (set_wire_messages first)");
        cfg_.send_img = on;
        if (on) cfg_.jpg_quality = quality;
        apply_jpeg();
    }
private:
    struct Lane;
    void apply_fit_pca(Lane& l) {
        if (cfg_.fit_pca && !l.fit) { l.fit = std::make_unique<PcaFitX>(l.sp_ctx); l.sp.set_pcafit(l.fit.get()); }
        else if (!cfg_.fit_pca && l.fit) { l.sp.set_pcafit(nullptr); l.fit.reset(); }
    }
    void apply_fit_pca() {
        for (auto& l : lanes_) apply_fit_pca(*l);
        for (auto& t : tail_lanes_) apply_fit_pca(*t.second);
    }
    // (the whole descriptor's stage reads the JPEG stage's files and follows the wire stage: it is set behind either)
    void apply_jpeg(Lane& l) {
        l.cam.set_jpeg(send_img() ? cfg_.jpg_quality : 0, jpeg_capacity());
        const int mode = device_wire() ? cfg_.wire_img_desc : WIRE_IMG_OFF;
        l.cam.set_wire_image(mode >= WIRE_IMG_WHOLE, mode == WIRE_IMG_IMAGE || (mode >= WIRE_IMG_WHOLE && send_img()));
    }
    void apply_jpeg() {
        for (auto& l : lanes_) apply_jpeg(*l);
        for (auto& t : tail_lanes_) apply_jpeg(*t.second);
    }
    void apply_stereo_model(Lane& l) {
        const omni_stereo_model m = stereo_model();
        if (cfg_.stereo()) l.cam.set_camera_model(&cfg_.camera_model);      // (a mono unit's lens travels with its depth model)
        l.cam.set_stereo_model(device_landmarks() ? &m : nullptr);
        if (!cfg_.stereo()) {
            const omni_depth_model d = depth_model();
            l.cam.set_depth_model(device_depth_landmarks() ? &d : nullptr, &cfg_.camera_model);
        }
        l.cam.set_wire(device_wire(), cfg_.send_all_features);      // (behind the models: the stage is refused on a handle without one)
        apply_jpeg(l);
    }
    void apply_stereo_model() {
        for (auto& l : lanes_) apply_stereo_model(*l);
        for (auto& t : tail_lanes_) apply_stereo_model(*t.second);
    }
    // pose_drone of the m key frames of the unit about to be enqueued on `lane` -- the PoseMsgs finish() stamps on its messages
    void unit_poses(Lane* lane, int m, int64_t first_id) {
        if (!device_landmarks() && !device_depth_landmarks()) return;
        pose_stage_.resize((size_t)7 * m);
        for (int k = 0; k < m; ++k) {
            const PoseMsg p = lane->meta.empty() ? pose_of(first_id + k) : lane->meta[(size_t)k].pose;
            std::copy(p.position, p.position + 3, pose_stage_.data() + 7 * k); std::copy(p.quat_wxyz, p.quat_wxyz + 4, pose_stage_.data() + 7 * k + 3);
        }
        lane->cam.set_poses(pose_stage_.data(), m);
        if (device_wire()) {
            // ... and what its main images send besides the unit's arrays: the fields finish() stamps on their messages (stamp_image_descriptor, finish_frame_descriptor)
            const int nd = cfg_.dirs();
            wire_meta_.assign((size_t)m * nd, omni_wire_image_meta{});
            for (int k = 0; k < m; ++k) {
                const bool streamed = !lane->meta.empty();
                const int64_t kf_id = streamed ? lane->meta[(size_t)k].msg_id : first_id + k;
                for (int d = 0; d < nd; ++d) {
                    omni_wire_image_meta& w = wire_meta_[(size_t)k * nd + d];
                    w.timestamp = streamed ? lane->meta[(size_t)k].stamp : (double)kf_id; w.frame_id = kf_id; w.drone_id = cfg_.self_id; w.direction = d;
                    w.prevent_adding_db = 0;                       // (the frame's flag stays on the frame: no local image carries one)
                    std::copy(pose_stage_.data() + 7 * k, pose_stage_.data() + 7 * k + 7, w.pose_drone);
                    const PoseMsg e = to_msg(view_extrinsic(d, true));
                    std::copy(e.position, e.position + 3, w.camera_extrinsic); std::copy(e.quat_wxyz, e.quat_wxyz + 4, w.camera_extrinsic + 3);
                }
            }
            lane->cam.set_wire_meta(wire_meta_.data(), m * nd);
        }
        if (!device_depth_landmarks()) return;
        // ... and its depth frames: the streaming intake's copies (push_keyframe), or run()'s key frames taken out of set_depth's range; nullptr: no depth image
        depth_frames_.resize((size_t)m);
        for (int k = 0; k < m; ++k) {
            const int64_t kf_id = first_id + k;
            depth_frames_[(size_t)k] = !lane->meta.empty() ? lane->meta[(size_t)k].depth
                                       : (depth_ && kf_id >= depth_base_ && kf_id < depth_base_ + depth_n_) ? depth_ + (size_t)(kf_id - depth_base_) * cfg_.width * cfg_.height : nullptr;
        }
        lane->cam.set_depth_host(depth_frames_.data(), cfg_.width, m);
    }
public:

    // STEREO_PINHOLE: the rig's two extrinsics (body -> camera, xyz + quaternion wxyz; swarm_loop.cpp:294-306) instead of the defaults.  Every key frame's
    // messages carry them, so they are fixed before the first key frame
    void set_stereo_extrinsics(const double* left7, const double* right7) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (cfg_.camera_configuration != 0) throw std::runtime_error("set_stereo_extrinsics: camera_configuration is not 0 (STEREO_PINHOLE)");
        if (first_keyframe_seen_) throw std::runtime_error("set_stereo_extrinsics after the first key frame");
        if (!left7 || !right7) throw std::invalid_argument("set_stereo_extrinsics: null argument");
        std::copy(left7, left7 + 7, cfg_.left_extrinsic); std::copy(right7, right7 + 7, cfg_.right_extrinsic);
        cfg_.have_stereo_extrinsics = true;
        apply_stereo_model();                                  // (the units triangulate from the same extrinsics the messages carry)
    }

    // ---- the LoopNet wire (Config::wire, Config::device_wire) -----------------------------------------------------------------------------------------------
    bool wire() const { return net_ != nullptr; }
    bool device_wire() const { return net_ && cfg_.device_wire && (device_landmarks() || device_depth_landmarks()); }
    bool send_all_features() const { return cfg_.send_all_features; }
    // before the first key frame (what the C entry point omni_pipeline_set_wire sets)
    void set_wire(bool on, bool device, bool send_all_features) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (any_keyframe_seen_) throw std::runtime_error("set_wire after the first key frame");
        if (on && shard_) throw std::runtime_error("set_wire: the sharded database builds no messages");
        if (device && !on) throw std::runtime_error("set_wire: device_wire without wire");
        if (device && !(device_landmarks() || device_depth_landmarks()))
            throw std::runtime_error("set_wire: device_wire packs the landmarks the key-frame unit made: it needs device_landmarks (the stereo configurations) or "
                                     "device_depth_landmarks (PINHOLE_DEPTH) in effect, with the geometry stage on");
        cfg_.wire = on; cfg_.device_wire = on && device; cfg_.send_all_features = send_all_features;
        if (!on) { net_.reset(); outbox_.clear(); inbox_.clear(); cfg_.wire_img_desc = WIRE_IMG_OFF; cfg_.wire_loop_conn = false; }
        else if (!net_) {
            net_ = std::make_unique<LoopNetWire>(cfg_.self_id);
            net_->publish = [this](const char* ch, const std::vector<uint8_t>& b) {
                if (!publishing_) return;
                publishing_->off.push_back((int64_t)publishing_->bytes.size()); publishing_->size.push_back((int)b.size());
                publishing_->channel.push_back(std::strcmp(ch, wire::CH_HEADER) == 0 ? 0 : std::strcmp(ch, wire::CH_LANDMARKS) == 0 ? 1 : std::strcmp(ch, wire::CH_IMG_DES) == 0 ? 2 : 3);
                publishing_->bytes.insert(publishing_->bytes.end(), b.begin(), b.end());
            };
            net_->frame_desc_callback = [this](const FisheyeFrameDescriptor& f) { inbox_.push_back(f); };
            net_->loopconn_callback = [this](const LoopEdge& e) { remote_edges_.push_back(e); };
            net_->image_callback = [this](const ImageDescriptor& d) {
                if (d.image.empty()) return;                       // (a descriptor without its file: nothing to show)
                if (remote_images_.size() >= REMOTE_IMAGES_MAX) { remote_images_.pop_front(); ++remote_images_dropped_; }
                remote_images_.push_back({d.drone_id, d.frame_id, d.direction, d.image_width, d.image_height, d.image});
            };
            net_->MIN_DIRECTION_LOOP = cfg_.min_direction_loop;
        }
        if (net_) net_->SEND_ALL_FEATURES = send_all_features;
        apply_stereo_model();
    }
    // the receiving side's settings (loop_net.h:33, swarm_loop.cpp:232; group_by_frame_id false: the reference's frame key)
    void set_wire_recv(double recv_period, int min_direction_loop, bool group_by_frame_id) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (!net_) throw std::runtime_error("set_wire_recv: the wire is off (set_wire)");
        if (!(recv_period >= 0) || min_direction_loop < 1) throw std::invalid_argument("set_wire_recv: recv_period < 0 or MIN_DIRECTION_LOOP < 1");
        net_->recv_period = recv_period; net_->MIN_DIRECTION_LOOP = min_direction_loop; net_->group_by_frame_id = group_by_frame_id;
    }
    // ---- the wire's other two message kinds (Config::wire_img_desc, Config::wire_loop_conn) -----------------------------------------------------------------
    int wire_img_desc() const { return net_ ? cfg_.wire_img_desc : WIRE_IMG_OFF; }
    bool wire_loop_conn() const { return net_ && cfg_.wire_loop_conn; }
    // before the first key frame (what the C entry point omni_pipeline_set_wire_messages sets)
    void set_wire_messages(int img_desc, bool loop_conn) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (any_keyframe_seen_) throw std::runtime_error("set_wire_messages after the first key frame");
        if (shard_) throw std::runtime_error("set_wire_messages: the sharded database builds no messages");
        if (!net_) throw std::runtime_error("set_wire_messages: the wire is off (set_wire)");
        if (img_desc < WIRE_IMG_OFF || img_desc > WIRE_IMG_PC_REPLAY) throw std::invalid_argument("set_wire_messages: wire_img_desc outside 0..3 (OFF, IMAGE, WHOLE, PC_REPLAY)");
        if (img_desc == WIRE_IMG_IMAGE && !send_img()) throw std::runtime_error("set_wire_messages: wire_img_desc IMAGE sends the JPEG file: send_img is not in effect (set_send_img)");
        const int before = cfg_.wire_img_desc;
        cfg_.wire_img_desc = img_desc;
        try { apply_jpeg(); } catch (...) { cfg_.wire_img_desc = before; apply_jpeg(); throw; }       // (the unit refuses a JPEG capacity that is no multiple of 4)
        cfg_.wire_loop_conn = loop_conn;
        // LoopNet(_lcm_uri, send_img, send_whole_img_desc, ..) and IS_PC_REPLAY, as LoopNetWire::broadcast_img_desc reads them
        net_->send_img = img_desc == WIRE_IMG_IMAGE; net_->send_whole_img_desc = img_desc == WIRE_IMG_WHOLE; net_->is_pc_replay = img_desc == WIRE_IMG_PC_REPLAY;
    }
    // received whole descriptors that carry their 64-d descriptors enter the frame flow (LoopNetWire::accept_img_desc: what a replay ground station sets)
    void set_wire_accept_img_desc(bool on) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (!net_) throw std::runtime_error("set_wire_accept_img_desc: the wire is off (set_wire)");
        net_->accept_img_desc = on;
    }
    bool wire_accept_img_desc() const { return net_ && net_->accept_img_desc; }
    // the edges other drones sent (SWARM_LOOP_CONN), in arrival order; this pipeline's own edges are never listed
    const std::vector<LoopEdge>& remote_edges() const { return remote_edges_; }
    // the JPEG files other drones sent inside whole descriptors, oldest first; at most REMOTE_IMAGES_MAX are kept
    struct RemoteImage { int drone_id = 0; int64_t frame_id = 0; int direction = 0, width = 0, height = 0; std::vector<uint8_t> bytes; };
    size_t remote_images_pending() const { return remote_images_.size(); }
    int64_t remote_images_dropped() const { return remote_images_dropped_; }
    const RemoteImage* oldest_remote_image() const { return remote_images_.empty() ? nullptr : &remote_images_.front(); }
    RemoteImage take_remote_image() {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (remote_images_.empty()) throw std::runtime_error("take_remote_image: no image is pending");
        RemoteImage r = std::move(remote_images_.front());
        remote_images_.pop_front();
        return r;
    }
    // one finished local key frame's packets, in sending order: channel 0 = VIOKF_HEADER, 1 = VIOKF_LANDMARKS, 2 = SWARM_LOOP_IMG_DES; or one accepted edge's one
    // packet, channel 3 = SWARM_LOOP_CONN, msg_id the edge's id
    struct SentFrame { int64_t msg_id = 0; std::vector<uint8_t> bytes; std::vector<int64_t> off; std::vector<int> size; std::vector<uint8_t> channel; };
    size_t wire_pending() const { return outbox_.size(); }
    const SentFrame* oldest_packets() const { return outbox_.empty() ? nullptr : &outbox_.front(); }
    SentFrame take_packets() {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (outbox_.empty()) throw std::runtime_error("take_packets: no key frame's packets are pending");
        SentFrame s = std::move(outbox_.front());
        outbox_.pop_front();
        return s;
    }
    // A packet of the transport (LoopNet's two lcm.subscribe handlers, loop_net.cpp:9-13) / the periodic scan (:231-298), between two calls of run / push_keyframe /
    // poll / flush.  Every frame the wire completes goes through the serial flow: flush(), then on_remote_frame -- its candidate lands in candidates(), an accepted
    // loop in edges().  This pipeline's own packets are ignored (sent_message).  false: the packet did not parse or has another shape.
    bool recv_packet(const char* channel, const uint8_t* data, size_t n, double now) {
        if (!net_) throw std::runtime_error("recv_packet: the wire is off (set_wire)");
        if (!channel || (!data && n)) throw std::invalid_argument("recv_packet: null argument");
        const bool ok = net_->on_packet(channel, data, n, now);
        drain_inbox();
        return ok;
    }
    void scan_recv(double now) {
        if (!net_) throw std::runtime_error("scan_recv: the wire is off (set_wire)");
        net_->scan_recv_packets(now);
        drain_inbox();
    }
    int64_t remote_frames() const { return remote_frames_; }
    // the calling thread's milliseconds inside finish() spent on the wire so far: broadcast_fisheye_desc, or the copy and the id patch of device_wire
    double wire_host_ms(bool reset) { const double v = wire_ms_; if (reset) wire_ms_ = 0; return v; }
private:
    void drain_inbox() {
        while (!inbox_.empty()) {
            FisheyeFrameDescriptor f = std::move(inbox_.front());
            inbox_.pop_front();
            ++remote_frames_;
            if (cfg_.remote_in_stream) { queue_remote_frame(std::move(f)); continue; }
            ++remote_stats_[3];
            const int hits = flush();                          // (the local candidates this flush found are returned by the next push_keyframe / poll / flush)
            { std::lock_guard<std::mutex> lk(intake_mu_); carried_hits_ += hits; }
            on_remote_frame(f);
        }
        pcm_feed();
    }
    // finish(): the unit's key frames leave as packets -- broadcast_fisheye_desc on the calling thread, or the unit's own packed bytes with the ids patched in
    void wire_out(Lane& lane) {
        const bool dev = device_wire();
        const omni_cam_wire_result wr = dev ? lane.cam.wire() : omni_cam_wire_result{};
        const int nd = cfg_.dirs(), mode = cfg_.wire_img_desc;
        // the whole descriptors of the same images, packed by the unit behind their packets; under PC_REPLAY they leave alone (loop_net.cpp:37-41)
        const omni_cam_wire_image_result wi = dev && mode != WIRE_IMG_OFF ? lane.cam.wire_image() : omni_cam_wire_image_result{};
        const bool alone = mode == WIRE_IMG_PC_REPLAY;
        auto whole_size = [&](size_t i) {
            if (mode == WIRE_IMG_OFF) return 0;
            const int off = wi.sizes[2 * i], size = wi.sizes[2 * i + 1];
            if (size == 0 && off == 0) return 0;
            if (off != WP_IMAGE_OFFSET || size < WP_IMAGE_HEAD_BYTES || (int64_t)off + size > wi.capacity) throw std::runtime_error("wire_out: a whole descriptor out of place");
            return size;
        };
        for (int m = 0; m < lane.cur; ++m) {
            FisheyeFrameDescriptor& f = frames_[(size_t)m];
            outbox_.emplace_back();
            SentFrame& s = outbox_.back();
            s.msg_id = f.msg_id;
            if (!dev) {
                publishing_ = &s;
                try { net_->broadcast_fisheye_desc(f); } catch (...) { publishing_ = nullptr; throw; }
                publishing_ = nullptr;
                continue;
            }
            size_t total = 0;
            for (int d = 0; d < nd; ++d) {
                const int* tb = wr.table + ((size_t)nd * m + d) * wr.table_ints;
                if (tb[0] < 0 || tb[0] > 1 + wr.max_num || tb[1] < 0 || tb[1] > wr.capacity || (tb[0] > 0 && tb[1] < WP_LANDMARKS_AT)) throw std::runtime_error("wire_out: a packet table out of range");
                if (tb[0] && !alone) total += (size_t)tb[1] - WP_HEADER_OFFSET;
                if (tb[0]) total += (size_t)whole_size((size_t)nd * m + d);
            }
            s.bytes.reserve(total);
            for (int d = 0; d < nd; ++d) {
                const size_t i = (size_t)nd * m + d;
                const int* tb = wr.table + i * wr.table_ints;
                const uint8_t* buf = wr.packets + i * (size_t)wr.capacity;
                if (!tb[0]) continue;
                const int ws = whole_size(i);
                // the image's id (LoopNetWire's sequence: the header's, or under PC_REPLAY the image's one id), then its whole descriptor behind its packets
                int64_t header_id = 0;
                auto whole = [&] {
                    if (!ws) return;
                    const size_t at = s.bytes.size();
                    const uint8_t* src = wi.packets + i * (size_t)wi.capacity + WP_IMAGE_OFFSET;
                    s.bytes.insert(s.bytes.end(), src, src + ws);
                    wp::patch_whole_image_id(s.bytes.data() + at, header_id);
                    s.off.push_back((int64_t)at); s.size.push_back(ws); s.channel.push_back(2);
                };
                if (alone) { header_id = net_->reserve_id(true); f.images[(size_t)d].msg_id = header_id; whole(); continue; }
                // an image's packets lie back to back behind the buffer's padding: one copy, then the ids
                const size_t base = s.bytes.size();
                s.bytes.insert(s.bytes.end(), buf + WP_HEADER_OFFSET, buf + tb[1]);
                for (int k = 0; k < tb[0]; ++k) {
                    const int off = tb[WP_TABLE_HEAD + 2 * k], size = tb[WP_TABLE_HEAD + 2 * k + 1];
                    if (off != (k ? wp::landmark_offset(k - 1) : WP_HEADER_OFFSET) || size != (k ? WP_LANDMARK_BYTES : WP_HEADER_BYTES) || (int64_t)off + size > tb[1])
                        throw std::runtime_error("wire_out: a packet out of place");
                    uint8_t* at = s.bytes.data() + base + (size_t)(off - WP_HEADER_OFFSET);
                    if (k == 0) { header_id = net_->reserve_id(true); wp::patch_header_id(at, header_id); f.images[(size_t)d].msg_id = header_id; }
                    else wp::patch_landmark_ids(at, net_->reserve_id(false), header_id);
                    s.off.push_back((int64_t)(base + (size_t)(off - WP_HEADER_OFFSET))); s.size.push_back(size); s.channel.push_back(k ? 1 : 0);
                }
                whole();
            }
        }
    }
    // an accepted edge as it enters edges(): LoopNet::broadcast_loop_connection (loop_net.cpp:122-127), an outbox entry of its own
    void queue_loop_conn(const LoopEdge& e) {
        outbox_.emplace_back();
        SentFrame& s = outbox_.back();
        s.msg_id = e.id;
        publishing_ = &s;
        try { net_->broadcast_loop_connection(e); } catch (...) { publishing_ = nullptr; throw; }
        publishing_ = nullptr;
    }
public:

    // A key frame that arrived from ANOTHER drone (LoopNet's reassembled message; LoopDetector::on_image_recv, loop_detector.cpp:11-137), handed to the detector on
    // the calling thread between two calls of run / push_keyframe / poll / flush, after a flush().  Everything deferred earlier is verified first; the frame's own
    // candidate is verified on the spot -- the detector needs the verdict for its init-mode counters -- with init_mode's limits (1 000 PnP iterations, the lower
    // gates) while fewer than inter_drone_init_frames loops connect the two drones.  The candidate goes into candidates(), an accepted loop into edges().
    LoopCandidate on_remote_frame(const FisheyeFrameDescriptor& f) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (shard_) throw std::runtime_error("on_remote_frame: the sharded database builds no messages");
        if (f.drone_id == cfg_.self_id) throw std::invalid_argument("on_remote_frame: the frame carries this drone's own id");
        // remote_in_stream: frames queued earlier (and the batch that holds some) come first, so the order is kept
        if (cfg_.remote_in_stream && (!remote_queue_.empty() || det_pending_.active)) carried_hits_ += flush_locked();
        collect_geometry();
        pcm_note_frame(f.drone_id, f.msg_id, f.pose_drone);
        const LoopCandidate r = det_.on_image_recv(f);
        collect_geometry();
        pcm_feed();
        if (r.found) candidates_.push_back({f.msg_id, r.old_msg_id, r.direction_new, r.direction_old});
        return r;
    }
    // ---- remote key frames in the unit stream (Config::remote_in_stream) -------------------------------------------------------------------------------------
    bool remote_in_stream() const { return cfg_.remote_in_stream; }
    // before the first key frame (what the C entry point omni_pipeline_set_remote_in_stream sets)
    void set_remote_in_stream(bool on) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (any_keyframe_seen_) throw std::runtime_error("set_remote_in_stream after the first key frame");
        if (on && shard_) throw std::runtime_error("set_remote_in_stream: the sharded database builds no messages");
        if (!on && remote_pending() > 0) throw std::runtime_error("set_remote_in_stream(false): remote frames are queued (flush first)");
        cfg_.remote_in_stream = on;
    }
    // A key frame of ANOTHER drone joins the stream: it is queued behind the local key frames handed over so far and leaves with the next unit's detector batch --
    // or, when every local key frame in front of it has its batch begun and no batch is pending, at once in a batch of remote frames alone (collected by poll(),
    // the next unit or flush()).  Its candidate goes into candidates(), an accepted loop into edges(), as with on_remote_frame.
    void queue_remote_frame(FisheyeFrameDescriptor&& f) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (shard_) throw std::runtime_error("queue_remote_frame: the sharded database builds no messages");
        if (!cfg_.remote_in_stream) throw std::runtime_error("queue_remote_frame: remote_in_stream is off (set_remote_in_stream)");
        if (f.drone_id == cfg_.self_id) throw std::invalid_argument("queue_remote_frame: the frame carries this drone's own id");
        pcm_note_frame(f.drone_id, f.msg_id, f.pose_drone);
        remote_queue_.push_back({std::move(f), next_seq_});
        ++remote_stats_[0];
        begin_remote_batch();
    }
    // remote frames queued or in a detector batch that has not been collected yet
    int64_t remote_pending() const { return (int64_t)remote_queue_.size() + remote_in_batch_; }
    // [0] frames queued so far, [1] of them, frames that joined a key-frame unit's batch, [2] batches of remote frames alone, [3] flushes a remote frame forced
    // (the frames of the wire that took the switch-off path)
    void remote_stats(int64_t out[4]) const { for (int i = 0; i < 4; ++i) out[i] = remote_stats_[i]; }
    LoopDetectorCore& detector() { return det_; }
    LoopGeometry& geometry() { return geo_; }
    // the reference's launch parameters (host/swarm_loop_params.hpp) that reach the detector and the geometry stage AFTER construction (the constructor took
    // what Config carries: SwarmLoopParams::to_pipeline_config)
    template <class Params> void apply_params(const Params& p) { p.to_detector(det_); p.to_geometry(geo_); }

    // PINHOLE_DEPTH: the depth images (u16 millimetres, height x width, rows packed) of key frames msg_id = first_msg_id .. first_msg_id + n - 1,
    // image i at depth + i * width * height.  Borrowed: they must stay valid until the run() that consumes them returns (with device_depth_landmarks a
    // unit's frames are read when it is enqueued, inside that run()).  A key frame without one gets no landmarks.
    void set_depth(int64_t first_msg_id, const uint16_t* depth, int64_t n) { depth_base_ = first_msg_id; depth_ = depth; depth_n_ = n; }

    // N > 1 GPUs, one process per GPU: the database becomes one row-sharded index over all ranks (omni_shard_*, RCCL inside libomni_hip.so).
    // Collective: every rank attaches with rank 0's unique id.  Each micro-batch is then one exchange unit (two ncclAllGather) and a key
    // frame's candidate is decided on GLOBAL ids with the reference's rule (loop_detector.cpp:232: recency + threshold); the id maps of
    // LoopDetectorCore describe one drone's own database and are not used in this mode.
    void attach_shard(int rank, int world, const char* unique_id) {
        if (cfg_.fit_pca) throw std::runtime_error("attach_shard: fit_pca does not run on the sharded database, which builds no descriptors of its own");
        if (cfg_.wire) throw std::runtime_error("attach_shard: the wire does not run on the sharded database, which builds no messages");
        if (cfg_.remote_in_stream) throw std::runtime_error("attach_shard: remote_in_stream does not run on the sharded database, which builds no messages");
        if (cfg_.batch_verify) throw std::runtime_error("attach_shard: batch_verify does not run on the sharded database, which builds no messages");
        if (cfg_.pcm) throw std::runtime_error("attach_shard: pcm does not run on the sharded database, which builds no messages");
        if (cfg_.pose_graph) throw std::runtime_error("attach_shard: the pose graph does not run on the sharded database, which builds no messages");
        if (cfg_.fisheye_raw()) throw std::runtime_error("attach_shard: the raw-fisheye mode (fisheye_src_width x fisheye_src_height) does not run on the sharded database");
        shard_index_ = std::make_unique<IndexFlatIP>(index_ctx_, 4096, cfg_.storage);
        shard_ = omni_shard_create(index_ctx_.get(), shard_index_->handle(), 4096, rank, world, unique_id);
        if (!shard_) throw std::runtime_error(std::string("omni_shard_create: ") + omni_last_error());
        world_ = world;
        apply_stereo_model();                                  // (off: this mode builds no messages)
        apply_jpeg();
    }
    ~KeyframePipeline() { if (pg_handle_) omni_pgo_destroy(pg_handle_); if (shard_) omni_shard_destroy(shard_); }
    int64_t db_rows() const { return shard_ ? omni_shard_ntotal(shard_) : det_.local_index.ntotal + det_.remote_index.ntotal; }

    // bulk pre-load of the key-frame database: rows [n][4096], dirs() consecutive rows = the directions of one earlier key frame
    void preload(const float* rows, int64_t n) {
        if (shard_) { check(omni_shard_preload_local(shard_, rows, n, n * world_), "omni_shard_preload_local"); return; }    // this rank's rows
        const int64_t base = det_.local_index.ntotal;
        for (int64_t s = 0; s < n; s += 4096) det_.local_index.add(std::min<int64_t>(4096, n - s), rows + s * 4096);
        const int nd = cfg_.dirs();
        for (int64_t i = 0; i < n; ++i) { det_.imgid2fisheye[(int)(base + i)] = -((base + i) / nd) - 1; det_.imgid2dir[(int)(base + i)] = (int)((base + i) % nd); }
    }

    // n_keyframes key frames through the whole hot path.  pool[e] = one micro-batch of images in (pinned) host memory,
    // [up cameras of the MB frames (4 each) | down cameras of the MB frames] (PINHOLE_DEPTH: the MB gray images; STEREO_PINHOLE: [the MB left frames | the MB right
    // frames], at the camera's size when Config::src_width is set), u8, rows packed; micro-batch s uses pool[(first_slot + s) %
    // n_pool].  When n_keyframes is not a multiple of the micro-batch the last rem frames run as their own, smaller unit from `tail`
    // (same layout for rem frames): EXACTLY n_keyframes key frames are processed.  from_host: upload inside the loop
    // (omni_cam_enqueue_host); otherwise the pool entries are device pointers.  Returns the number of loop candidates found.
    int run(int n_keyframes, int64_t first_msg_id, const uint8_t* const* pool, int n_pool, int first_slot, const uint8_t* tail, bool from_host) {
        if (open_ || !stream_pending_.empty()) throw std::runtime_error("run: key frames pushed through push_keyframe are still open -- flush() first");
        if (cfg_.camera_configuration == 0 && n_keyframes > 0) first_keyframe_seen_ = true;
        if (n_keyframes > 0) any_keyframe_seen_ = true;
        const int MB = cfg_.microbatch, nd = cfg_.dirs();
        const int full = n_keyframes / MB, rem = n_keyframes % MB;
        // The units of this call.  Host blocks can be cut anywhere (a unit's upload is a list of segments: omni_cam_enqueue_host_parts), so a run that is not a
        // whole number of micro-batches is cut into units of (nearly) EQUAL size -- 20 key frames = 7 + 7 + 6, not 8 + 8 + 4: a unit far below the size the
        // kernels' grids were sized for runs the same launches at a fraction of the work, and at the reference's key-frame rates (swarm_loop.cpp:140-170: 0.3-1 Hz
        // per drone) every run() is a short one.  Device-resident blocks and the sharded database keep the blocks' own cut (a unit there is one exchange step).
        std::vector<int> sizes;
        // (The raw-fisheye mode keeps the blocks' own cut as well: the fisheye entry takes one segment per camera, it has no _host_parts flavour.)
        const bool recut = from_host && !shard_ && unit_plan_ != 0 && rem != 0 && full >= 1 && !cfg_.fisheye_raw();
        if (recut) sizes = plan_units(n_keyframes, MB, unit_plan_);
        else { sizes.assign(full, MB); if (rem) sizes.push_back(rem); }
        Lane* tail_lane = (!recut && rem) ? prepare(n_keyframes) : nullptr;
        std::deque<std::pair<Lane*, int64_t>> pending;
        int hits = 0;
        // units oldest first (omni_cam_order_after)?  OMNI_PIPELINE_FIFO >= 0 decides; the default (-1) does by what this call is given: the fp32-class
        // modes always (CU-filling convolutions end to end: +2-4 %); fp16 when the whole run is in flight at once (no more units than lanes: the first
        // unit then finishes early and the host's work on it overlaps the rest, +13 % at 3 units, +1.5 % at 4), not in a run the lanes' in-flight limit
        // staggers anyway (the units' kernels taking turns fill each other's tails: +6 % at 5 units, +4 % at 7, +5 % at 8;
        // profiles/r06k_fifo_by_units.log -- until round 6 the rule chained every run of fewer than 8 units)
        const int n_units = (int)sizes.size();
        const int fifo = fifo_cfg_ >= 0 ? fifo_cfg_ : ((cfg_.precision != OMNI_PREC_F16 || n_units <= (int)lanes_.size()) ? 1 : 0);
        last_fifo_ = fifo;
        const size_t img = (size_t)cfg_.in_width() * cfg_.in_height();
        // key frame f of the call: its block (pool entry or the tail), the block's frame count, its index inside
        auto block_of = [&](int f, const uint8_t*& base, int& cnt, int& idx) {
            const int e = f / MB;
            if (e < full) { base = pool[(first_slot + e) % n_pool]; cnt = MB; idx = f - e * MB; }
            else { base = tail; cnt = rem; idx = f - full * MB; }
        };
        std::vector<const uint8_t*> up, down;
        std::vector<int> upn, downn;
        int f0 = 0;
        for (int s = 0; s < n_units; ++s) {
            const int m = sizes[s];
            Lane* lane = (recut || s < full) ? lanes_[s % lanes_.size()].get() : tail_lane;
            if (pend_lane_ == lane) check(omni_shard_rows_consumed(shard_), "omni_shard_rows_consumed");      // its row buffer is the exchange's input
            lane->t_enqueue = std::chrono::steady_clock::now();
            omni_trace_push("host: unit enqueue (upload + launches)");
            lane->meta.clear();
            const int want = recut ? m : lane->mb;
            if (lane->cur != want) { lane->cam.set_active(nd * want); lane->cur = want; }     // (the streaming intake or a recut run may have left another size)
            chain(lane, fifo);
            lane->seq_first = next_seq_; next_seq_ += m;            // (run()'s key frames are handed over in id order)
            unit_poses(lane, want, first_msg_id + f0);
            if (compressed()) {
                // pool[e] / tail: JpegFile[2 * cnt] (PINHOLE_DEPTH: [cnt]) -- the block's left (raw fisheye: up) files, then its right (down) files; a unit takes
                // its frames' files wherever the blocks are cut
                if (!from_host) throw std::invalid_argument("run: compressed_images takes files in host memory");
                std::vector<const uint8_t*> fp[2];
                std::vector<int64_t> fs[2];
                for (int f = f0; f < f0 + m; ++f) {
                    const uint8_t* base; int cnt, idx;
                    block_of(f, base, cnt, idx);
                    const JpegFile* jf = reinterpret_cast<const JpegFile*>(base);
                    for (int c = 0; c < (cfg_.stereo() ? 2 : 1); ++c) { fp[c].push_back(jf[c * cnt + idx].data); fs[c].push_back(jf[c * cnt + idx].size); }
                }
                enqueue_files(lane, fp, fs);
            } else if (recut) {
                up.clear(); down.clear(); upn.clear(); downn.clear();
                for (int f = f0; f < f0 + m;) {                                  // maximal runs of frames inside one block
                    const uint8_t* base; int cnt, idx;
                    block_of(f, base, cnt, idx);
                    const int take = std::min(cnt - idx, f0 + m - f);
                    up.push_back(base + (size_t)idx * nd * img); upn.push_back(take * nd);
                    if (cfg_.stereo()) { down.push_back(base + ((size_t)cnt + idx) * nd * img); downn.push_back(take * nd); }
                    f += take;
                }
                if (cfg_.resized()) lane->cam.enqueue_raw_host_parts(lane->resize->handle(), up, upn, down, downn, cfg_.src_width);
                else lane->cam.enqueue_host_parts(up, upn, down, downn, cfg_.masked());
            } else {
                const uint8_t* src = s < full ? pool[(first_slot + s) % n_pool] : tail;
                if (cfg_.fisheye_raw()) {                                                     // the block's up frames, then its down frames, of the fisheye camera's size
                    if (from_host) lane->cam.enqueue_fisheye_host(flatten_[0]->handle(), flatten_[1]->handle(), src, src + (size_t)want * img, cfg_.fisheye_src_width, want, cfg_.fisheye_first_view, true);
                    else lane->cam.enqueue_fisheye_dev(flatten_[0]->handle(), flatten_[1]->handle(), src, src + (size_t)want * img, cfg_.fisheye_src_width, want, cfg_.fisheye_first_view, true);
                }
                else if (cfg_.resized()) {                                                    // the block's left frames, then its right frames, at the camera's size
                    if (from_host) lane->cam.enqueue_raw_host(lane->resize->handle(), src, src + (size_t)want * img, cfg_.src_width, want);
                    else lane->cam.enqueue_raw_dev(lane->resize->handle(), src, src + (size_t)want * img, cfg_.src_width, want);
                }
                else if (from_host) lane->cam.enqueue_host(src, cfg_.width, cfg_.masked());   // loop_cam.cpp:536: only STEREO_FISHEYE blanks rows
                else lane->cam.enqueue_dev(src, cfg_.width, cfg_.masked());
            }
            host_ms_[0] += since(lane->t_enqueue);
            omni_trace_pop();
            pending.emplace_back(lane, first_msg_id + f0);
            f0 += m;
            if (pending.size() >= lanes_.size()) { hits += finish_timed(*pending.front().first, pending.front().second); pending.pop_front(); }
        }
        while (!pending.empty()) { hits += finish_timed(*pending.front().first, pending.front().second); pending.pop_front(); }
        hits += collect_exchange();
        hits += collect_detector();
        drain_geometry();
        return hits;
    }
    // the sizes of the units a run of n key frames is cut into (each <= MB, sum = n); plan 1: ceil(n / MB) units of equal size (+- 1, the larger ones first);
    // plan 2: the same with half a unit in front, so that the first kernels start behind half an upload
    static std::vector<int> plan_units(int n, int MB, int plan) {
        std::vector<int> out;
        if (n <= 0) return out;
        int head = 0;
        if (plan == 2 && n > MB) { head = std::max(1, MB / 2); out.push_back(head); n -= head; }
        const int k = (n + MB - 1) / MB;
        for (int i = 0; i < k; ++i) out.push_back(n / k + (i < n % k ? 1 : 0));
        return out;
    }

    // latency of every micro-batch processed so far: from the start of its upload to the end of its detector / geometry step (milliseconds;
    // every key frame of a micro-batch shares it).  The reference is batch-1 and serial (tensorrt_generic.cpp:58-75): a key frame there waits for
    // nothing but its own 12 engine calls; here it waits for its micro-batch and for the micro-batches in flight before it.
    const std::vector<double>& latencies_ms() const { return latencies_ms_; }
    void clear_latencies() { latencies_ms_.clear(); }

    void sync() { for (auto& l : lanes_) l->sync(); for (auto& t : tail_lanes_) t.second->sync(); check(omni_ctx_sync(index_ctx_.get()), "sync"); }

    // one key frame as SwarmLoop::VIOKF_callback hands it on (swarm_loop.cpp:140-170): the flattened views -- images[0..dirs) = up cameras, images[dirs..2*dirs)
    // = down cameras (PINHOLE_DEPTH: the one gray image; STEREO_PINHOLE: images[0] = the left frame, images[1] = the right frame, of the camera's size when
    // Config::src_width is set; the raw-fisheye mode: images[0] = the up frame, images[1] = the down frame of the fisheye camera's size), each Config::in_height() rows of `stride` bytes -- the key-frame id and stamp (StereoFrame::keyframe_id,
    // ::stamp), VIO's pose, and prevent_adding_db (:156: a non-key frame that moved less than min_movement_keyframe is matched but not added);
    // depth: PINHOLE_DEPTH's 16-bit depth image (rows packed), borrowed until the key frame's unit is finished -- with device_depth_landmarks it is copied before
    // push_keyframe returns, like the images
    struct KeyframeIn {
        const uint8_t* const* images = nullptr; int stride = 0;
        int64_t msg_id = 0; double stamp = 0; PoseMsg pose_drone; bool prevent_adding_db = false;
        const uint16_t* depth = nullptr;
        const int64_t* sizes = nullptr;                  // compressed(): images[i] is a JPEG file of sizes[i] bytes (copied before the call returns); `stride` is not read
    };
private:
    struct SlotMeta { int64_t msg_id = 0; double stamp = 0; PoseMsg pose; bool prevent_adding_db = false; const uint16_t* depth = nullptr; };
public:
    // The streaming intake (what a ROS callback calls per key frame; KeyframeIntake::extract in keyframe_intake.hpp): the images are packed into the
    // open micro-batch's pinned block and the call returns; the `microbatch`-th key frame sends the unit to the GPU (one upload, SuperPoint,
    // MobileNetVLAD, up/down match, one download) and, when `pipelines` units are in flight, finishes the oldest (detector, geometry).  Returns the
    // loop candidates found by the units this call finished.  The reference handles one key frame at a time, synchronously (tensorrt_generic.cpp:58-75).
    int push_keyframe(const KeyframeIn& k) {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (shard_) throw std::runtime_error("push_keyframe: the sharded database is driven through run()");
        const bool jpg = compressed();
        if (jpg && (!k.images || !k.sizes)) throw std::invalid_argument("push_keyframe: compressed_images is set: no files / no sizes");
        if (!jpg && k.sizes) throw std::invalid_argument("push_keyframe: JPEG files for a pipeline that takes pixels (compressed_images is off, or ignored in this mode)");
        if (!jpg && (!k.images || k.stride < cfg_.in_width())) throw std::invalid_argument("push_keyframe: no images / a row stride below the image width");
        const int MB = cfg_.microbatch, nd = cfg_.frames_per_camera(), cams = cfg_.stereo() ? 2 : 1;      // nd: images per camera and key frame
        for (int i = 0; i < cfg_.frames_per_keyframe(); ++i) if (!k.images[i] || (jpg && k.sizes[i] < 0)) throw std::invalid_argument("push_keyframe: a null image pointer");
        const size_t img = (size_t)cfg_.in_width() * cfg_.in_height();
        if (cfg_.camera_configuration == 0) first_keyframe_seen_ = true;      // (set_stereo_extrinsics is refused from here on)
        any_keyframe_seen_ = true;
        int hits = carried_hits_; carried_hits_ = 0;
        // whatever throws below: the candidates counted so far are not lost -- they go back into carried_hits_ and the next call returns them
        struct Carry { int& hits; int& carried; bool ok = false; ~Carry() { if (!ok) carried += hits; } } carry{hits, carried_hits_};
        hits += reap_ready();                                   // units the GPU has finished meanwhile (non-blocking): "idle" below is then the truth
        if (!open_) {
            // round robin over the lanes: with fewer than `pipelines` units in flight the next lane is free (a poll() may have sent a partial unit without
            // finishing the oldest -- it never waits --, so that is made sure of here)
            while (stream_pending_.size() >= lanes_.size()) { Lane* l = stream_pending_.front(); stream_pending_.pop_front(); hits += finish_timed(*l, 0); }
            Lane* l = lanes_[next_lane_++ % lanes_.size()].get();
            l->meta.clear();
            for (auto& f : l->jfiles) f.clear();
            if (!jpg && !l->stage) {
                l->stage_bytes = (size_t)cams * nd * MB * img;
                l->stage = static_cast<uint8_t*>(omni_host_alloc(l->stage_bytes));
                if (!l->stage) throw std::runtime_error(std::string("omni_host_alloc: ") + omni_last_error());
            }
            l->t_enqueue = std::chrono::steady_clock::now();
            l->seq_first = next_seq_;
            open_ = l;
        }
        const int m = (int)open_->meta.size();
        if (m >= MB) throw std::logic_error("push_keyframe: the open micro-batch is already full");      // (cannot happen: a full unit leaves below, whatever throws)
        for (int c = 0; c < cams && jpg; ++c) open_->jfiles[c].emplace_back(k.images[c], k.images[c] + k.sizes[c]);      // (nd = 1 wherever files are taken)
        for (int c = 0; c < cams && !jpg; ++c)
            for (int d = 0; d < nd; ++d) {
                uint8_t* dst = open_->stage + ((size_t)c * nd * MB + (size_t)nd * m + d) * img;
                const uint8_t* src = k.images[c * nd + d];
                for (int y = 0; y < cfg_.in_height(); ++y) std::memcpy(dst + (size_t)y * cfg_.in_width(), src + (size_t)y * k.stride, (size_t)cfg_.in_width());
            }
        SlotMeta sm; sm.msg_id = k.msg_id; sm.stamp = k.stamp; sm.pose = k.pose_drone; sm.prevent_adding_db = k.prevent_adding_db; sm.depth = k.depth;
        if (k.depth && device_depth_landmarks()) {                // the unit reads the frame when it leaves for the GPU: the lane's own copy, not the caller's buffer
            const size_t dimg = (size_t)cfg_.width * cfg_.height;
            if (open_->depth_stage.size() < dimg * MB) open_->depth_stage.resize(dimg * MB);
            std::memcpy(open_->depth_stage.data() + dimg * m, k.depth, dimg * sizeof(uint16_t));
            sm.depth = open_->depth_stage.data() + dimg * m;
        }
        open_->meta.push_back(sm);
        ++next_seq_;                                            // handed over: a remote frame queued from now on comes behind this key frame
        const bool full = (int)open_->meta.size() == MB;
        const bool idle = cfg_.dispatch_when_idle && stream_pending_.empty();
        const bool aged = cfg_.max_wait_ms >= 0 && since(open_->t_enqueue) >= cfg_.max_wait_ms;
        if (full || idle || aged) {
            dispatch_open();
            while (stream_pending_.size() >= lanes_.size()) { Lane* l = stream_pending_.front(); stream_pending_.pop_front(); hits += finish_timed(*l, 0); }
        }
        carry.ok = true;
        return hits;
    }
    // The latency bound of the streaming intake, to be called from a timer (or after every push): never waits for a CNN unit.  (1) a partly filled
    // micro-batch older than Config::max_wait_ms leaves for the GPU as it is; (2) every unit the GPU has finished goes through the detector; (3) when no
    // unit is in flight any more, the detector step enqueued last (reported one unit later otherwise: OMNI_DETECTOR_ASYNC) and its geometry are
    // collected -- a short wait for searches that run on an otherwise idle GPU.  Returns the loop candidates found.
    int poll() {
        std::lock_guard<std::mutex> lk(intake_mu_);
        if (shard_) return 0;
        int hits = carried_hits_; carried_hits_ = 0;
        hits += reap_ready();
        if (open_ && !open_->meta.empty() && cfg_.max_wait_ms >= 0 && since(open_->t_enqueue) >= cfg_.max_wait_ms) dispatch_open();
        begin_remote_batch();                                   // queued remote frames with no local key frame in front of them do not wait for one
        return hits;
    }
    // everything pushed so far through the detector (and the geometry stage): a partial micro-batch runs as its own, smaller unit
    int flush() {
        std::lock_guard<std::mutex> lk(intake_mu_);
        return flush_locked();
    }
private:
    int flush_locked() {
        int hits = carried_hits_; carried_hits_ = 0;
        std::exception_ptr first;
        try { if (open_ && !open_->meta.empty()) dispatch_open(); } catch (...) { first = std::current_exception(); }
        open_ = nullptr;
        while (!stream_pending_.empty()) {
            Lane* l = stream_pending_.front(); stream_pending_.pop_front();
            try { hits += finish_timed(*l, 0); } catch (...) { if (!first) first = std::current_exception(); }      // the other units are still finished
        }
        try { hits += collect_detector(); drain_geometry(); } catch (...) { if (!first) first = std::current_exception(); }
        // the queue is drained completely: every local key frame is through (or was dropped with a failed unit), what is left goes as batches of remote frames
        begun_seq_ = next_seq_;
        try {
            while (!remote_queue_.empty()) { begin_remote_batch(); if (!det_pending_.active) break; hits += collect_detector(); drain_geometry(); }
        } catch (...) { if (!first) first = std::current_exception(); }
        if (first) std::rethrow_exception(first);
        return hits;
    }
public:
    // the streaming intake's settings after construction (what the C entry point omni_pipeline_set_latency sets)
    void set_latency(double max_wait_ms, bool dispatch_when_idle) { std::lock_guard<std::mutex> lk(intake_mu_); cfg_.max_wait_ms = max_wait_ms; cfg_.dispatch_when_idle = dispatch_when_idle; }

    // creates (once) the smaller unit a run of n_keyframes needs for its trailing n_keyframes % microbatch key frames, so that the first
    // timed run does not pay for it
    Lane* prepare(int n_keyframes) {
        const int rem = n_keyframes % cfg_.microbatch;
        if (!rem) return nullptr;
        auto it = tail_lanes_.find(rem);
        if (it == tail_lanes_.end()) { it = tail_lanes_.emplace(rem, std::make_unique<Lane>(cfg_, rem)).first; apply_stereo_model(*it->second); apply_jpeg(*it->second); apply_fit_pca(*it->second); }
        return it->second.get();
    }

private:
    struct Lane {                                      // one micro-batch in flight: its own streams, networks and result block
        Lane(const Config& c, int mb_)
            : mb(mb_), one_stream(cfg_int("OMNI_PIPELINE_ONE_STREAM") != 0), sp_ctx(c.device), vlad_ctx(one_stream ? nullptr : std::make_unique<Context>(c.device)),
              sp(sp_ctx, c.sp_weights, c.pca_comp, c.pca_mean, c.width, c.height, c.thres, c.max_num, false, c.precision, (c.stereo() ? 2 : 1) * c.dirs() * mb_),
              vlad(vlad_stream_ctx(), c.vlad_weights, c.width, c.height, false, c.dirs() * mb_),
              cam(sp_ctx, sp, vlad_stream_ctx(), vlad, c.dirs() * mb_, c.max_num, c.width, c.height, !c.stereo()) {
            check(omni_vlad_dev_output(vlad.handle(), &rows_dev), "omni_vlad_dev_output");
            if (c.resized()) resize = std::make_unique<ResizeHIP>(sp_ctx, c.src_width, c.src_height, c.width, c.height);
            cur = mb_;
        }
        void sync() { check(omni_ctx_sync(sp_ctx.get()), "sync"); if (vlad_ctx) check(omni_ctx_sync(vlad_ctx->get()), "sync"); }
        std::chrono::steady_clock::time_point t_enqueue;
        int mb;                                        // key frames the unit was created for
        int64_t seq_first = 0;                         // hand-over number of the unit's first key frame (remote_in_stream: the unit covers [seq_first, seq_first + cur))
        int cur = 0;                                   // ... and of the unit in flight (a partly filled micro-batch of the streaming intake: omni_cam_set_active)
        std::vector<SlotMeta> meta;                    // streaming intake (push_keyframe): what each key frame of the unit came with; empty = run()'s numbering
        std::vector<std::vector<uint8_t>> jfiles[2];   // streaming intake with compressed_images: the unit's JPEG files, left then right camera, copied at the push
        int jpeg_frames = 0;                           // > 0: the unit in flight came as that many JPEG files (their statuses are read when it is finished)
        uint8_t* stage = nullptr;                      // pinned block the streaming intake packs the unit's images into
        std::vector<uint16_t> depth_stage;             // streaming intake with device_depth_landmarks: the unit's depth frames [mb][height][width], copied at the push
        size_t stage_bytes = 0;
        ~Lane() { if (fit) (void)omni_sp_set_pcafit(sp.handle(), nullptr); if (stage) omni_host_free(stage); }
        bool one_stream;                               // MobileNetVLAD behind SuperPoint on ONE stream (OMNI_PIPELINE_ONE_STREAM) instead of next to it on its own
        Context sp_ctx;
        std::unique_ptr<Context> vlad_ctx;             // MobileNetVLAD's own stream: made only when it is used (an idle stream takes a hardware-queue slot too, csrc/stream_plan.h)
        Swarm::SuperPointHIP sp;
        Context& vlad_stream_ctx() { return one_stream ? sp_ctx : *vlad_ctx; }
        Swarm::MobileNetVLADHIP vlad;
        LoopCamHIP cam;
        std::unique_ptr<ResizeHIP> resize;             // STEREO_PINHOLE with camera-size frames: the tables of the resize that runs inside the unit
        const float* rows_dev = nullptr;
        std::unique_ptr<PcaFitX> fit;                  // Config::fit_pca: the lane's own accumulator, attached to sp (declared last: it goes before the handle and its context do)
    };

    // The open unit of the streaming intake leaves for the GPU, full or not (a partial one: the down cameras' block moves up behind the up cameras' and the
    // unit runs with fewer directions, omni_cam_set_active -- no second set of networks).  Exception-safe: open_ is cleared FIRST, so whatever throws
    // below the next push starts a fresh unit (a failed unit's key frames are dropped with it: the caller got the exception).
    void dispatch_open() {
        Lane* u = open_;
        open_ = nullptr;
        const int MB = cfg_.microbatch, nd = cfg_.dirs(), nf = cfg_.frames_per_camera(), rem = (int)u->meta.size();
        const size_t img = (size_t)cfg_.in_width() * cfg_.in_height();
        try {
            if (!compressed() && rem < MB && cfg_.stereo()) std::memmove(u->stage + (size_t)nf * rem * img, u->stage + (size_t)nf * MB * img, (size_t)nf * rem * img);
            if (u->cur != rem) { u->cam.set_active(nd * rem); u->cur = rem; }
            chain(u, fifo_cfg_ >= 0 ? fifo_cfg_ : (cfg_.precision == OMNI_PREC_F16 ? 0 : 1));
            unit_poses(u, rem, 0);
            if (compressed()) {
                std::vector<const uint8_t*> fp[2];
                std::vector<int64_t> fs[2];
                for (int c = 0; c < 2; ++c)
                    for (const auto& f : u->jfiles[c]) { fp[c].push_back(f.data()); fs[c].push_back((int64_t)f.size()); }
                enqueue_files(u, fp, fs);
            }
            else if (cfg_.fisheye_raw())
                u->cam.enqueue_fisheye_host(flatten_[0]->handle(), flatten_[1]->handle(), u->stage, u->stage + (size_t)rem * img, cfg_.fisheye_src_width, rem, cfg_.fisheye_first_view, true);
            else if (cfg_.resized()) u->cam.enqueue_raw_host(u->resize->handle(), u->stage, u->stage + (size_t)rem * img, cfg_.src_width, rem);
            else u->cam.enqueue_host(u->stage, cfg_.width, cfg_.masked());
        } catch (...) { u->meta.clear(); throw; }
        stream_pending_.push_back(u);
    }
    // a unit's JPEG files to the GPU: decoded inside the unit, in front of the resize (an empty file would read as a null pointer: it gets a byte to point at)
    void enqueue_files(Lane* u, std::vector<const uint8_t*> (&fp)[2], std::vector<int64_t> (&fs)[2]) {
        static const uint8_t kNothing = 0;
        for (int c = 0; c < 2; ++c)
            for (auto& p : fp[c]) if (!p) p = &kNothing;
        if (cfg_.fisheye_raw()) u->cam.enqueue_fisheye_jpeg_async(flatten_[0]->handle(), flatten_[1]->handle(), fp[0], fs[0], fp[1], fs[1], cfg_.fisheye_first_view, true);
        else u->cam.enqueue_jpeg_async(u->resize ? u->resize->handle() : nullptr, fp[0], fs[0], fp[1], fs[1]);
        u->jpeg_frames = (int)(fp[0].size() + fp[1].size());
    }
    // finishes, oldest first, the units the GPU is done with (never waits for a CNN unit); with nothing left in flight also the detector step enqueued
    // last and its geometry
    int reap_ready() {
        int hits = 0;
        while (!stream_pending_.empty() && stream_pending_.front()->cam.ready()) { Lane* l = stream_pending_.front(); stream_pending_.pop_front(); hits += finish_timed(*l, 0); }
        if (stream_pending_.empty() && det_pending_.active) { hits += collect_detector(); drain_geometry(); }
        return hits;
    }

    // waits for the exchange in flight (if any) and applies the reference's rule (loop_detector.cpp:232: recency + threshold) on GLOBAL row ids
    int collect_exchange() {
        if (!pend_lane_) return 0;
        const int k = LoopDetectorCore::SEARCH_NEAREST_NUM + cfg_.match_index_dist, mb = pend_mb_;
        D_.resize((size_t)mb * k); I_.resize((size_t)mb * k);
        pend_lane_ = nullptr;
        check(omni_shard_step_wait(shard_, D_.data(), I_.data()), "omni_shard_step_wait");
        { float a = 0, b = 0; if (omni_shard_last_exchange_us(shard_, &a, &b) == OMNI_OK) exchange_us_.push_back({a, b}); }
        int hits = 0;
        for (int m = 0; m < mb; ++m) {
            const int64_t nt = pend_base_ + (int64_t)(m + 1) * world_ * cfg_.dirs();          // ntotal as of this key frame's step
            for (int j = 0; j < k; ++j) {
                const int64_t id = I_[(size_t)m * k + j];
                if (id >= 0 && id <= nt - cfg_.match_index_dist && D_[(size_t)m * k + j] > cfg_.inner_product_thres) { ++hits; break; }
            }
        }
        return hits;
    }
    int finish_timed(Lane& lane, int64_t first_id) {
        const int hits = finish(lane, first_id);
        if (shard_) latencies_ms_.push_back(since(lane.t_enqueue));       // (the local path records a unit's latency when its detector step is collected)
        return hits;
    }
    // The detector step of the unit whose batch was begun last: LoopDetectorCore::end_images_batch waits for the copy of its result lists -- enqueued one
    // unit ago, so it ran behind the CNN kernels of the unit that is in flight and the host does not wait here -- and replays the rules; then the unit's
    // geometry.  (The host used to wait for the searches right where it enqueued them: on a GPU kept busy by the next unit's kernels that round trip took
    // 2.9 ms of a 3.8 ms cycle, the next unit was enqueued late and the GPU idled 15 % of the time -- host_times(), DESIGN.md.)
    int collect_detector() {
        if (!det_pending_.active) return 0;
        auto t_a = std::chrono::steady_clock::now();
        omni_trace_push("host: detector collect (result lists, rules) + geometry hand-over");
        struct Pop { ~Pop() { omni_trace_pop(); } } pop_at_exit;
        int hits = 0, fi = 0;
        det_pending_.active = false;                     // first: if end_images_batch() throws (its rollback has dropped the batch), the next unit starts clean
        remote_in_batch_ = 0;
        for (auto& c : det_.end_images_batch()) {
            // (the returned count stays that of LOCAL key frames; a remote frame's candidate is in candidates(), as with on_remote_frame)
            if (c.found) { if (det_pending_.remote.empty() || !det_pending_.remote[(size_t)fi]) ++hits; candidates_.push_back({det_pending_.ids[(size_t)fi], c.old_msg_id, c.direction_new, c.direction_old}); }
            ++fi;
        }
        host_ms_[3] += since(t_a);
        t_a = std::chrono::steady_clock::now();
        // the previous micro-batch's tasks ran meanwhile; this one's run until the next is collected.  The tasks reference this micro-batch's frames:
        // those moved into the database live there (std::map: stable), the others are handed over
        drain_geometry();
        const bool left = start_geometry(&det_.held_frames(), det_pending_.timed ? &det_pending_.t_enqueue : nullptr);
        if (!async_geometry_) drain_geometry();
        det_.held_frames().clear();
        if (!left && det_pending_.timed) latencies_ms_.push_back(since(det_pending_.t_enqueue));        // (otherwise drain_geometry() records it, when the micro-batch's last edge is in)
        host_ms_[4] += since(t_a);
        pcm_feed();                                      // Config::pcm: the edges drained so far enter the stage
        return hits;
    }
    // the micro-batch's key frames reach the detector in order, as one batch; rows and queries are taken from MobileNetVLAD's output
    // buffer in HBM ([4*mb][4096], key-frame major) -- wait() has synchronised with the MobileNetVLAD stream
    int finish(Lane& lane, int64_t first_id) {
        auto t_a = std::chrono::steady_clock::now();
        struct Range { explicit Range(const char* n) { omni_trace_push(n); } ~Range() { omni_trace_pop(); } };
        const omni_cam_result r = [&lane] { Range range_wait("host: wait for the unit's GPU work"); return lane.cam.wait(); }();
        host_ms_[1] += since(t_a); ++host_units_;
        if (lane.jpeg_frames > 0) {
            for (int st : lane.cam.jpegdec_status(lane.jpeg_frames)) jpeg_corrupt_ += st == OMNI_JPEGDEC_CORRUPT;
            lane.jpeg_frames = 0;
        }
        t_a = std::chrono::steady_clock::now();
        Range range_rest("host: messages + detector step of the unit");
        if (shard_) {
            // the exchange of THIS micro-batch is enqueued (two collectives, the scan, the copy of the lists: no host wait) and its results are
            // collected when the NEXT micro-batch gets here (or at the end of run()): meanwhile the host enqueues the next CNN unit
            int hits = collect_exchange();
            const int k = LoopDetectorCore::SEARCH_NEAREST_NUM + cfg_.match_index_dist;
            check(omni_shard_step_enqueue(shard_, lane.cur, cfg_.dirs(), lane.rows_dev, cfg_.masked() ? 1 : 0, k), "omni_shard_step_enqueue");      // the query image: direction 1 of a fisheye key frame, else 0
            pend_lane_ = &lane; pend_mb_ = lane.cur; pend_base_ = omni_shard_ntotal(shard_);
            return hits;
        }
        const int n = r.n_dirs, M = r.max_num, D = r.desc_dim, nd = cfg_.dirs();
        frames_.resize(lane.cur);
        const int G = r.global_dim;
        // Without the geometry stage the detector's plan (which rows are appended, which searches run: LoopDetectorCore::begin_batch) reads counts and ids only:
        // the messages are first built LIGHT (landmark_num, stamps), the detector step is enqueued, and the heavy part -- 75 KB of key points, descriptors and
        // lifted points per image -- is copied into the frames the detector now holds while its searches run on the GPU.  With the geometry stage the landmarks
        // can change landmark_num (generate_gray_depth_image_descriptor drops an image below ACCEPT_MIN_3D_PTS): everything is built first, as before.
        const bool defer_heavy = !cfg_.geometry && !net_;                      // (the wire sends whole messages: they are built first)
        // the unit's own landmarks (Config::device_landmarks): lifted floats, 3-D points and flags of every image, already in the pinned block
        const bool dev_dp = device_depth_landmarks();
        const bool dev_lm = device_landmarks() || dev_dp;
        const omni_cam_landmarks_result lmr = dev_lm ? lane.cam.landmarks() : omni_cam_landmarks_result{};
        // the unit's own JPEG files of its main images (Config::send_img), already in the lane's pinned block
        const bool jpg = send_img();
        const omni_cam_jpeg_result jr = jpg ? lane.cam.jpeg() : omni_cam_jpeg_result{};
        auto heavy = [&](ImageDescriptor& im, int i) {
            if (dev_lm) fill_image_descriptor_device(im, r.kps_xy + (size_t)i * M * 2, r.n_kps[i], r.desc + (size_t)i * M * D, D, r.global_desc + (size_t)i * G, G,
                                                     lmr.norm2d + (size_t)i * M * 2, lmr.landmarks_3d + (size_t)i * M * 3, lmr.landmarks_flag + (size_t)i * M);
            else fill_image_descriptor(im, r.kps_xy + (size_t)i * M * 2, r.n_kps[i], r.desc + (size_t)i * M * D, D, r.global_desc + (size_t)i * G, G, lift64_);
        };
        for (int m = 0; m < lane.cur; ++m) {
            FisheyeFrameDescriptor& f = frames_[m];
            const bool streamed = !lane.meta.empty();
            const int64_t kf_id = streamed ? lane.meta[m].msg_id : first_id + m;
            const double stamp = streamed ? lane.meta[m].stamp : (double)kf_id;
            const PoseMsg pose = streamed ? lane.meta[m].pose : pose_of(kf_id);
            f.prevent_adding_db = streamed && lane.meta[m].prevent_adding_db;
            f.images.resize(nd);
            for (int d = 0; d < nd; ++d) {
                const int i = nd * m + d;                                           // image i of the up cameras
                ImageDescriptor& im = f.images[d];
                // extractor_img_desc_deepnet (loop_cam.cpp:525-585) + the stamps of generate_stereo_image_descriptor (:362-374)
                if (defer_heavy) im.landmark_num = r.n_kps[i]; else heavy(im, i);
                if (jpg) {                                                          // encode_image (loop_cam.cpp:306-308, 463-469; width and height: :67-70)
                    im.image_width = cfg_.width; im.image_height = cfg_.height;
                    if (jr.status[i] == OMNI_JPEG_OK) im.image.assign(jr.bytes + (size_t)i * jr.capacity, jr.bytes + (size_t)i * jr.capacity + jr.sizes[i]);
                    else { im.image.clear(); ++jpeg_truncated_; }
                }
                stamp_image_descriptor(im, stamp, cfg_.self_id, to_msg(view_extrinsic(d, true)), pose, kf_id);
                if (cfg_.geometry && !cfg_.stereo()) {
                    // generate_gray_depth_image_descriptor's landmarks (loop_cam.cpp:260-304): read from the depth image under each key point -- by the unit
                    // itself with device_depth_landmarks (the message is complete as it comes out of the block), else here
                    if (dev_dp) continue;
                    const bool have = streamed ? lane.meta[m].depth != nullptr : (depth_ && kf_id >= depth_base_ && kf_id < depth_base_ + depth_n_);
                    if (have) fill_depth_landmarks(im, streamed ? lane.meta[m].depth : depth_ + (size_t)(kf_id - depth_base_) * cfg_.width * cfg_.height, cfg_.width, cfg_.width, cfg_.height, cfg_.depth_near,
                                                   cfg_.depth_far, cfg_.accept_min_3d_pts, lift64_);
                } else if (cfg_.geometry) {
                    // the stereo half of generate_stereo_image_descriptor (loop_cam.cpp:341-454): the down image of this direction, triangulation
                    // (one task per direction on the geometry pool: ~170 SVD triangulations each; joined before the frames reach the detector)
                    if (downs_.size() < (size_t)nd * lane.cur) downs_.resize((size_t)nd * lane.cur);
                    ImageDescriptor& down = downs_[(size_t)i];
                    down = ImageDescriptor{};
                    const int j = n + i;
                    if (dev_lm) {                                                    // both messages are complete as they come out of the block: no task
                        fill_image_descriptor_device(down, r.kps_xy + (size_t)j * M * 2, r.n_kps[j], nullptr, D, nullptr, 0, lmr.norm2d + (size_t)j * M * 2,
                                                     lmr.landmarks_3d + (size_t)j * M * 3, lmr.landmarks_flag + (size_t)j * M);
                        stamp_image_descriptor(down, stamp, cfg_.self_id, to_msg(view_extrinsic(d, false)), pose, kf_id);
                        continue;
                    }
                    fill_image_descriptor(down, r.kps_xy + (size_t)j * M * 2, r.n_kps[j], nullptr, D, nullptr, 0, lift64_);     // (its descriptors were matched on the device)
                    stamp_image_descriptor(down, stamp, cfg_.self_id, to_msg(view_extrinsic(d, false)), pose, kf_id);
                    auto tri = [this, &im, &down, r, i, M] {
                        // the triangulation lifts the pixels again, in double (loop_cam.cpp:403-407); the message keeps the float points
                        fill_stereo_landmarks(im, down, r.match_up + (size_t)i * M, r.match_down + (size_t)i * M, r.n_matches[i], cfg_.triangle_thres, cfg_.accept_min_3d_pts,
                                              &lift64_);
                    };
                    if (pool_) stereo_tasks_.push_back(pool_->submit(tri)); else tri();
                }
            }
            finish_frame_descriptor(f, stamp, kf_id, pose, cfg_.self_id);             // on_flattened_images (loop_cam.cpp:178-217)
            pcm_note_frame(cfg_.self_id, kf_id, pose);
        }
        {   // join the triangulation tasks; if one throws, the others are still joined (they reference this micro-batch's frames) and the list is
            // emptied before the exception leaves: the next finish() must not meet futures that were already consumed
            std::exception_ptr first;
            for (auto& t : stereo_tasks_) {
                try { t.get(); } catch (...) { if (!first) first = std::current_exception(); }
            }
            stereo_tasks_.clear();
            if (first) std::rethrow_exception(first);
        }
        host_ms_[2] += since(t_a);
        if (net_) {
            t_a = std::chrono::steady_clock::now();
            wire_out(lane);
            wire_ms_ += since(t_a);
        }
        t_a = std::chrono::steady_clock::now();
        int hits = collect_detector();                                          // the unit before this one
        t_a = std::chrono::steady_clock::now();
        det_pending_.ids.resize((size_t)lane.cur);
        for (int m = 0; m < lane.cur; ++m) det_pending_.ids[(size_t)m] = lane.meta.empty() ? first_id + m : lane.meta[(size_t)m].msg_id;
        det_pending_.t_enqueue = lane.t_enqueue; det_pending_.timed = true;
        det_pending_.remote.clear();
        unit_pos_.clear();
        begun_seq_ = lane.seq_first + lane.cur;                                  // (whatever throws below: these key frames will not come again)
        if (!join_remote(lane))
            det_.begin_images_batch(std::move(frames_), lane.rows_dev);         // appends + searches + the copy of the lists: enqueued, not waited for
        det_pending_.active = true;
        frames_.clear();
        // the appends and the query gather read MobileNetVLAD's output buffer: the lane's next unit must not overwrite it before they have
        check(omni_ctx_order_after(lane.vlad_stream_ctx().get(), index_ctx_.get()), "omni_ctx_order_after");
        host_ms_[3] += since(t_a);
        if (defer_heavy) {                                                      // the messages' contents, into the frames the detector holds, under its GPU work
            t_a = std::chrono::steady_clock::now();
            std::vector<FisheyeFrameDescriptor>& held = det_.held_frames();
            // key frames in stripes over the helper threads and this one (OMNI_MESSAGE_THREADS): each message is written by one thread, the result block is
            // only read; what the stripes share is the allocator.  Matters where this is exposed: behind the LAST unit of a run() call
            const int n_kf = std::min(lane.cur, (int)held.size()), parts = msg_pool_ ? std::min(n_kf, msg_pool_->size() + 1) : 1;
            // unit slot m is batch frame unit_pos_[m] when remote frames have joined the batch (join_remote), frame m otherwise
            auto stripe = [&, n_kf, parts](int p) {
                for (int m = p; m < n_kf; m += parts) {
                    FisheyeFrameDescriptor& f = held[unit_pos_.empty() ? (size_t)m : unit_pos_[(size_t)m]];
                    for (int d = 0; d < nd && d < (int)f.images.size(); ++d) heavy(f.images[(size_t)d], nd * m + d);
                }
            };
            std::vector<std::future<void>> helpers;
            for (int p = 1; p < parts; ++p) helpers.push_back(msg_pool_->submit([&stripe, p] { stripe(p); }));
            std::exception_ptr first;
            try { stripe(0); } catch (...) { first = std::current_exception(); }
            for (auto& h : helpers) { try { h.get(); } catch (...) { if (!first) first = std::current_exception(); } }      // (every helper is joined: they reference this frame's locals)
            if (first) std::rethrow_exception(first);
            host_ms_[2] += since(t_a);
        }
        if (!async_detector_) hits += collect_detector();                       // OMNI_DETECTOR_ASYNC=0: wait for it here, as before (A/B)
        return hits;
    }

    // finish(): the queued remote frames that belong in front of, between or right behind the key frames of `lane`'s unit join its batch (host/remote_queue.hpp).
    // false: none do -- the caller begins the unit's batch as it always did.  frames_ and det_pending_.ids hold the unit's key frames on entry
    bool join_remote(Lane& lane) {
        if (!cfg_.remote_in_stream || remote_queue_.empty()) return false;
        std::vector<int64_t> ps;
        for (const QueuedRemote& q : remote_queue_) ps.push_back(q.p);
        int64_t taken = 0;
        const std::vector<RemoteMergeSlot> plan = remote_merge_plan(lane.seq_first, lane.seq_first + lane.cur, ps.data(), (int64_t)ps.size(), &taken);
        if (taken == 0) return false;
        const int nd = cfg_.dirs();
        std::vector<FisheyeFrameDescriptor> batch;
        std::vector<int64_t> first_row, ids;
        batch.reserve(plan.size());
        unit_pos_.assign((size_t)lane.cur, 0);
        for (const RemoteMergeSlot& s : plan) {
            det_pending_.remote.push_back(s.remote ? 1 : 0);
            if (s.remote) { FisheyeFrameDescriptor& f = remote_queue_[(size_t)s.index].f; ids.push_back(f.msg_id); first_row.push_back(-1); batch.push_back(std::move(f)); }
            else { unit_pos_[(size_t)s.index] = batch.size(); ids.push_back(det_pending_.ids[(size_t)s.index]); first_row.push_back((int64_t)nd * s.index); batch.push_back(std::move(frames_[(size_t)s.index])); }
        }
        remote_queue_.erase(remote_queue_.begin(), remote_queue_.begin() + taken);
        det_pending_.ids = std::move(ids);
        remote_stats_[1] += taken;
        det_.begin_images_batch(std::move(batch), lane.rows_dev, (int64_t)nd * lane.cur, first_row);
        remote_in_batch_ = taken;
        return true;
    }
    // A batch of remote frames alone, for those that wait for no local key frame: every local key frame handed over before the oldest queued frame has its batch
    // begun (no open unit and no unit in flight in front of it), and no detector batch is pending.  Collected like a unit's: collect_detector
    void begin_remote_batch() {
        if (!cfg_.remote_in_stream || remote_queue_.empty() || det_pending_.active || remote_queue_.front().p > begun_seq_) return;
        std::vector<int64_t> ps;
        for (const QueuedRemote& q : remote_queue_) ps.push_back(q.p);
        int64_t taken = 0;
        remote_merge_plan(begun_seq_, begun_seq_, ps.data(), (int64_t)ps.size(), &taken);
        std::vector<FisheyeFrameDescriptor> batch;
        det_pending_.ids.clear();
        for (int64_t q = 0; q < taken; ++q) { det_pending_.ids.push_back(remote_queue_[(size_t)q].f.msg_id); batch.push_back(std::move(remote_queue_[(size_t)q].f)); }
        remote_queue_.erase(remote_queue_.begin(), remote_queue_.begin() + taken);
        det_pending_.remote.assign((size_t)taken, 1);
        det_pending_.timed = false;
        unit_pos_.clear();
        ++remote_stats_[2];
        // (nothing is deferred while no batch is pending, and the replay verifies a remote candidate behind everything started earlier: no wait for the geometry here)
        det_.begin_images_batch(std::move(batch), nullptr, 0, std::vector<int64_t>((size_t)taken, -1));
        det_pending_.active = true;
        remote_in_batch_ = taken;
    }

    Config cfg_;
    // cam->liftProjective of the flattened (pinhole) views, then the division by z: in double, as the reference's camera model
    // the camera's lift in double (camera_model.hpp -> csrc/camera_plan.h: the header the unit's landmark kernel runs; the ideal pinhole by default)
    const std::function<geom::Vec2(const Point2f&)> lift64_ = [this](const Point2f& p) { return camera().lift(p); };
    Context index_ctx_;
    LoopDetectorCore det_;
    BFMatcherL2X bf_{index_ctx_};
    LoopGeometry geo_;
    std::vector<double> latencies_ms_;
    struct GeoBatch {                           // the geometry tasks of one micro-batch, in candidate order
        std::vector<std::future<std::pair<bool, LoopEdge>>> futs;
        std::vector<char> self_self;            // per task: a candidate between two frames of the self drone (the detector did not get its verdict)
        std::vector<char> verdict;              // per task: batch_verify's inter-drone candidate, whose verdict the detector's ticket waits for
        std::vector<FisheyeFrameDescriptor> held;
        std::chrono::steady_clock::time_point t_enqueue;
        bool timed = false;
    };
    std::deque<GeoBatch> geo_inflight_;         // (declared before the pool: outlives its threads)
    // ids: one per frame of the batch (a remote frame's own msg_id); remote: per frame, empty = a unit's key frames alone; timed: a unit's batch (its latency is recorded)
    struct DetPending { bool active = false, timed = true; std::vector<int64_t> ids; std::vector<char> remote; std::chrono::steady_clock::time_point t_enqueue; } det_pending_;
    bool async_detector_ = [] { int v = 1; check(omni_config_value("OMNI_DETECTOR_ASYNC", &v), "omni_config_value"); return v != 0; }();
    bool async_geometry_ = [] { int v = 1; check(omni_config_value("OMNI_GEOMETRY_ASYNC", &v), "omni_config_value"); return v != 0; }();
    std::atomic<int> homography_pairs_device_{0}, homography_pairs_host_{0};      // (counted by the geometry tasks; declared before the pool: outlive its threads)
    std::atomic<int> pnp_candidates_device_{0}, pnp_candidates_host_{0};
    int corr_candidates_device_ = 0, corr_candidates_host_ = 0;      // batch_verify: candidates whose correspondences came from the GPU / that the device handed back
    // device_pnp: a context (stream, staging, mutex) of its own -- the geometry tasks block on it for the length of a candidate's RANSAC, and neither the unit
    // enqueues, the detector step nor the matcher round trip of the host thread (the lanes' contexts, index_ctx_) ever wait for that mutex.  Made when the
    // switch is first on, kept until the pipeline goes (declared before the pool: outlives its threads)
    std::unique_ptr<Context> pnp_ctx_;
    std::unique_ptr<PnPRansacX> pnp_;
    void ensure_pnp_context() { if (!pnp_) { pnp_ctx_ = std::make_unique<Context>(cfg_.device, false); pnp_ = std::make_unique<PnPRansacX>(*pnp_ctx_); } }
    std::unique_ptr<TaskPool> pool_;
    std::unique_ptr<TaskPool> msg_pool_ = [] { const int n = cfg_int("OMNI_MESSAGE_THREADS"); return n > 0 ? std::make_unique<TaskPool>(n) : nullptr; }();
    std::vector<ImageDescriptor> downs_;        // the down-camera halves of the micro-batch being finished
    std::vector<std::future<void>> stereo_tasks_;
    struct Deferred { const FisheyeFrameDescriptor *a, *b; int da, db; bool im; bool verdict = false; };
    std::vector<char> verdicts_;                // batch_verify: the verdicts drain_geometry() collected for the resolve that is running
    int64_t verify_deferred_ = 0, verify_round_trips_ = 0, matcher_round_trips_ = 0;
    std::vector<Deferred> deferred_;            // candidates waiting for collect_geometry(): references into the database / the current micro-batch
    std::vector<LoopEdge> edges_;
    std::vector<Candidate> candidates_;
    std::vector<PoseMsg> poses_;
    int64_t pose_base_ = 0;
    const uint16_t* depth_ = nullptr;           // PINHOLE_DEPTH: borrowed depth images (set_depth)
    int64_t depth_base_ = 0, depth_n_ = 0;
    int geometry_calls_ = 0;
    std::unique_ptr<FlattenHIP> flatten_[2];    // the raw-fisheye mode: the up and the down camera's maps, read by every lane's units (declared before the lanes: outlive their streams)
    std::vector<std::unique_ptr<Lane>> lanes_;
    std::map<int, std::unique_ptr<Lane>> tail_lanes_;
    double host_ms_[5] = {0, 0, 0, 0, 0};
    int host_units_ = 0;
    // units in flight run oldest first (omni_cam_order_after): the unit about to be enqueued starts behind the convolution stack of the one enqueued last
    Lane* last_enqueued_ = nullptr;
    int unit_plan_ = cfg_int("OMNI_PIPELINE_UNIT_PLAN");    // how run() cuts a run that is not a whole number of micro-batches (plan_units; 0: the blocks' own cut)
    int fifo_cfg_ = cfg_int("OMNI_PIPELINE_FIFO");          // >= 0: as asked; -1: run() and the streaming intake decide (see run())
    int last_fifo_ = 0;                                      // what the last run() used (reported by the bench line)
    void chain(Lane* lane, int fifo_streams) {
        if (fifo_streams > 0 && last_enqueued_ && last_enqueued_ != lane) lane->cam.order_after(last_enqueued_->cam, fifo_streams);
        last_enqueued_ = lane;
    }
    std::mutex intake_mu_;                                   // push_keyframe / poll / flush may come from different threads (a callback and a timer)
    static int cfg_int(const char* name) { int v = 0; check(omni_config_value(name, &v), "omni_config_value"); return v; }
    static double since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }
    Lane* open_ = nullptr;                      // streaming intake: the micro-batch being filled
    std::deque<Lane*> stream_pending_;          // ... and the units in flight, oldest first
    size_t next_lane_ = 0;
    int carried_hits_ = 0;
    bool first_keyframe_seen_ = false;          // STEREO_PINHOLE: set_stereo_extrinsics is refused from the first key frame on
    std::atomic<int64_t> jpeg_truncated_{0};
    std::atomic<int64_t> jpeg_corrupt_{0};
    bool any_keyframe_seen_ = false;            // set_device_landmarks is refused from the first key frame on
    std::vector<double> pose_stage_;            // unit_poses: the unit's poses on their way into the handle's pinned staging
    std::vector<const uint16_t*> depth_frames_; // ... and its depth frames' addresses
    std::vector<FisheyeFrameDescriptor> frames_;
    // the LoopNet wire: the object, the finished key frames' packets not yet taken, the frames it completed and that are not yet through the detector
    std::unique_ptr<LoopNetWire> net_;
    std::deque<SentFrame> outbox_;
    std::deque<FisheyeFrameDescriptor> inbox_;
    SentFrame* publishing_ = nullptr;           // where broadcast_fisheye_desc's packets go while finish() runs it
    std::vector<omni_wire_image_meta> wire_meta_;
    int64_t remote_frames_ = 0;
    std::vector<LoopEdge> remote_edges_;        // SWARM_LOOP_CONN of other drones, in arrival order
    std::deque<RemoteImage> remote_images_;     // the files of their whole descriptors, at most REMOTE_IMAGES_MAX
    int64_t remote_images_dropped_ = 0;
    // Config::pcm: the stage on a context of its own, the path lengths it reads, how far edges_ / remote_edges_ have entered it, the edges left outside it
    std::unique_ptr<Context> pcm_ctx_;
    std::unique_ptr<LoopOutlierRejection> pcm_;
    struct PcmPath { bool any = false; double last[3] = {0, 0, 0}, length = 0; };
    std::map<int, PcmPath> pcm_path_;
    std::map<std::pair<int, int64_t>, double> pcm_arc_;
    size_t pcm_fed_local_ = 0, pcm_fed_remote_ = 0;
    std::set<int64_t> pcm_outside_;
    int64_t pcm_unknown_ = 0;
    std::vector<omni_pcm_edge> pcm_records_;
    // Config::pose_graph: the window's builder, the solver's handle on a context of its own, and what the last optimize() built and found
    std::unique_ptr<Context> pg_ctx_;
    std::unique_ptr<SwarmPoseGraph> pg_;
    omni_pgo* pg_handle_ = nullptr;
    omni_pgo_params pg_params_ = pgo::default_params();
    SwarmPoseGraph::Problem pg_problem_;
    std::vector<double> pg_solution_;
    PoseGraphStats pg_stats_;
    // remote_in_stream: the queue in arrival order, each frame with p = the local key frames handed over before it; next_seq_: local key frames handed over so far;
    // begun_seq_: every local key frame below it has its detector batch begun; remote_in_batch_: remote frames in the batch that is pending
    struct QueuedRemote { FisheyeFrameDescriptor f; int64_t p; };
    std::deque<QueuedRemote> remote_queue_;
    int64_t next_seq_ = 0, begun_seq_ = 0, remote_in_batch_ = 0;
    int64_t remote_stats_[4] = {0, 0, 0, 0};
    std::vector<size_t> unit_pos_;               // finish(): unit slot -> position in the batch, when remote frames have joined it
    double wire_ms_ = 0;                        // the calling thread's milliseconds in wire_out so far (wire_host_ms)
    std::unique_ptr<IndexFlatIP> shard_index_;
    omni_shard* shard_ = nullptr;
    int world_ = 1;
    Lane* pend_lane_ = nullptr;                 // the micro-batch whose exchange is in flight
    int pend_mb_ = 0;
    int64_t pend_base_ = 0;
    std::vector<float> D_;
    std::vector<int64_t> I_;
    std::vector<std::pair<float, float>> exchange_us_;
};

}  // namespace omni
