// The sizes of the exact top-k (topk.h) that host code plans with: plain C++, no HIP (index_plan.h sizes a search's key buffers from them).
#pragma once

namespace omni {

constexpr int TOPK_CHUNK = 2048;         // keys per workgroup and level
constexpr int TOPK_MAX_K = 1024;
constexpr int TOPK_SEL_MAX_K = 64;       // topk_select_kernel instead of the bitonic sort up to this k

}  // namespace omni
