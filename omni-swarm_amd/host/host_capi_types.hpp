// host_capi_types.hpp -- what the C entry points of the host layer share: the handle behind `omni_pipeline*` (host_capi.cpp -> libomni_host.so,
// host_stereo_capi.cpp -> libomni_host_stereo.so; a handle made by one library is used through the other)
#pragma once
#include "keyframe_pipeline.hpp"

extern "C" {
struct omni_pipeline { omni::KeyframePipeline* p; };
}
