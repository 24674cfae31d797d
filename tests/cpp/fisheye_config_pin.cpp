// fisheye_config_pin.cpp -- KeyframePipeline::Config's raw-fisheye mode (host/keyframe_pipeline.hpp) checked alone: what resolved() refuses, and the accessors
// a key frame's layout is read from, for every {camera configuration} x {raw fisheye} x {compressed_images}.  Constructs no pipeline and no GPU object, and calls
// nothing of libomni_hip.so: a stand-alone program (tests/test_fisheye_config_cpu.py builds it with -fsanitize=address,undefined and runs it).
#include <cstdio>
#include <string>

#include "keyframe_pipeline.hpp"

using Config = omni::KeyframePipeline::Config;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// "" when resolved() accepts the configuration, else its message
static std::string refusal(const Config& c) {
    try { omni::KeyframePipeline::resolved(c); return ""; } catch (const std::exception& e) { return e.what(); }
}

// the rig of tests/test_gpu_cam_fisheye.py: 600 x 312 side views at 235 degrees
static Config rig(int configuration, bool raw, bool compressed) {
    Config c;
    c.camera_configuration = configuration; c.width = 600; c.height = 312; c.compressed_images = compressed;
    if (raw) { c.fisheye_src_width = 1280; c.fisheye_src_height = 1024; c.fisheye_fov_deg = 235.0; }
    return c;
}

int main() {
    EXPECT(omni::side_view_height(600, 235.0) == 312);
    EXPECT(omni::side_view_height(600, 180.0) == 0 && omni::side_view_height(600, 120.0) == 0);
    // the helper and the map generator agree (a small rig: the maps themselves are made here)
    {
        omni::MeiCamera mei;
        mei.xi = 1.8; mei.gamma1 = 110; mei.gamma2 = 110; mei.u0 = 64; mei.v0 = 51;
        const omni::FlattenMaps m = omni::generate_all_undist_maps(mei, 56, 235.0, 1);
        EXPECT(m.w.size() == 5 && m.side_height == omni::side_view_height(56, 235.0));
        for (size_t v = 1; v < m.w.size(); ++v) EXPECT(m.w[v] == 56 && m.h[v] == m.side_height && m.xy[v].size() == (size_t)56 * m.side_height * 2);
    }

    // ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
    EXPECT(refusal(rig(1, false, false)).empty() && refusal(rig(1, true, false)).empty() && refusal(rig(1, true, true)).empty());
    { Config c = rig(1, true, false); c.fisheye_src_height = 0; EXPECT(refusal(c).find("both or neither") != std::string::npos); }      // half a source size
    { Config c = rig(1, false, false); c.fisheye_src_height = 1024; EXPECT(refusal(c).find("both or neither") != std::string::npos); }
    for (int configuration : {0, 2}) {                                                                                                  // a source size with another configuration
        Config c = rig(configuration, false, false);
        c.fisheye_src_width = 1280; c.fisheye_src_height = 1024;
        EXPECT(refusal(c).find("camera_configuration 1") != std::string::npos);
    }
    { Config c = rig(1, true, false); c.height = 320; EXPECT(refusal(c).find("600 x 312 but the networks take 600 x 320") != std::string::npos); }      // views of another size
    { Config c = rig(1, true, false); c.width = 608; EXPECT(refusal(c).find("side views are 608 x") != std::string::npos); }
    { Config c = rig(1, true, false); c.fisheye_first_view = 0; EXPECT(refusal(c).find("fisheye_first_view + 4 = 4 views") != std::string::npos); }     // not first_view + 4 views
    { Config c = rig(1, true, false); c.fisheye_first_view = 2; EXPECT(refusal(c).find("views") != std::string::npos); }
    { Config c = rig(1, true, false); c.fisheye_fov_deg = 170.0; EXPECT(refusal(c).find("gives 1") != std::string::npos); }              // no side views at all
    // the resized stereo-pinhole frames keep their own rule
    { Config c = rig(1, false, false); c.src_width = 640; c.src_height = 480; EXPECT(refusal(c).find("camera_configuration 0") != std::string::npos); }
    { Config c = rig(0, false, false); c.src_width = 640; c.src_height = 480; EXPECT(refusal(c).empty()); }

    // ---- the accessors, every combination --------------------------------------------------------------------------------------------------------------------
    for (int configuration = 0; configuration < 3; ++configuration)
        for (int raw = 0; raw < 2; ++raw)
            for (int compressed = 0; compressed < 2; ++compressed) {
                if (raw && configuration != 1) continue;                       // (refused above)
                const Config c = omni::KeyframePipeline::resolved(rig(configuration, raw != 0, compressed != 0));
                const int flattened = configuration == 1 ? 8 : (configuration == 0 ? 2 : 1);
                EXPECT(c.fisheye_raw() == (raw != 0));
                EXPECT(c.frames_per_keyframe() == (raw ? 2 : flattened));
                EXPECT(c.frames_per_camera() == (raw ? 1 : (configuration == 1 ? 4 : 1)));
                EXPECT(c.in_width() == (raw ? 1280 : 600) && c.in_height() == (raw ? 1024 : 312));
                EXPECT(c.raw() == (raw != 0) && !c.resized());
                EXPECT(c.compressed() == (compressed && (configuration != 1 || raw)));      // a flattened-view STEREO_FISHEYE pipeline ignores the switch
                EXPECT(c.dirs() == (configuration == 1 ? 4 : 1) && c.masked() == (configuration == 1));
                std::printf("configuration %d raw %d compressed %d: frames %d, in %d x %d, compressed() %d\n", configuration, raw, compressed, c.frames_per_keyframe(),
                            c.in_width(), c.in_height(), (int)c.compressed());
            }
    // camera-size stereo-pinhole frames: raw() as before, two frames per key frame
    {
        Config c = rig(0, false, true);
        c.src_width = 640; c.src_height = 480;
        EXPECT(c.raw() && c.resized() && !c.fisheye_raw() && c.in_width() == 640 && c.in_height() == 480 && c.frames_per_keyframe() == 2 && c.compressed());
    }
    std::printf(failures ? "FAILED %d\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
