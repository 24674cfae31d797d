// omni_jpegdec_*: camera frames that arrive as baseline JPEG files (is_compressed_images: cv::imdecode(data, IMREAD_GRAYSCALE), swarm_loop.cpp:72-89) become gray
// images on the GPU.  The arithmetic, the symbol step and the parallel scheme are jpeg_dec_plan.h's -- this file only spreads them over lanes:
//   entropy  ONE workgroup per CHUNK of an image, phases 1-4 of the plan in one launch; grid (most chunks of a picture, images).  A picture without a restart
//            interval is one chunk.  A restart-interval file (OMNI_JPEGDEC_RESTART_WGS = W >= 1, snapshotted by the handle; 0: such files are decoded on the host)
//            is up to W chunks of consecutive intervals: every interval is a stream of its own (byte-aligned, entry state 0, DC predictor 0, first block known), so
//            no workgroup reads what another wrote and NONE WAITS FOR ANOTHER -- they meet only in three atomically combined words per picture (error bits OR,
//            rounds max, chunks that ran) zeroed on the stream; the status is derived once, by the DC kernel.  Inside a chunk:
//            a Huffman stream is sequential: it is cut into subsequences of S bits,
//            every lane decodes subsequences from a guessed state, and relaxation rounds repeat those whose predecessor's exit state changed until a round changes
//            nothing (self-synchronisation; at most N rounds, a fixed point IS the sequential decode).  Exit states, entry states and block counts live in LDS; the
//            round loop is workgroup-uniform (__syncthreads + an LDS flag).  Then the exclusive scan of the block counts, and the write pass: the first component's
//            coefficients straight to global memory (zeroed before), every index checked against the image's block count;
//   plain    a picture WITHOUT a restart interval on a handle whose OMNI_JPEGDEC_PLAIN_WGS is W >= 2 (snapshotted by the handle; 0 or 1: the entropy kernel as
//            above, nothing else launched or allocated) is JD_MODE_SPREAD: no business of the entropy kernel's, whose code stays what it was.  It takes three
//            launches instead, all on the caller's stream:
//              chunk  grid (most chunks of a picture, images): phases 1-2 (jd_relax, the entropy kernel's own) over the chunk's subsequences in LDS, the guess as
//                     the entry of the chunk's first one; exit state, entry used and count of every subsequence go to the handle's state arrays
//                     [image][subsequence]; rounds (max) and chunks that ran (+1) to the picture's flag words;
//              seam   one workgroup per picture: the SAME relaxation over all the picture's subsequences on the state arrays -- a subsequence is decoded again only
//                     when its predecessor's exit differs from the entry it last used, so only what the seams between chunks got wrong is repaired; at most n_sub
//                     rounds, the break workgroup-uniform through LDS; then the exclusive scan of the counts over the picture, in place.  The workgroup's waves
//                     exchange the state through GLOBAL memory across __syncthreads() (one CU, one L1; the arrays are neither const nor __restrict__, so no load is
//                     hoisted over a barrier or sent down the scalar path);
//              write  grid (ceil(most subsequences / JD_THREADS), images), one subsequence per lane: phase 4 from the stored entry and first block.
//            NO WORKGROUP WAITS FOR ANOTHER: the three launches are ordered by the stream alone, every loop has a bound known at launch, every barrier is
//            workgroup-uniform, and a picture's workgroups meet only in the atomically combined flag words;
//   dc       one workgroup per image: the status, then the scan of the DC differences in scan order -- segmented at every restart interval's first block;
//   block    across all images, one 8 x 8 block per lane: dequantise, islow IDCT, clamp, store cropped.  A CORRUPT image is written as zeros; the pixels of a
//            file the host decoded are copied from the uploaded block.
//   unstuff  (OMNI_JPEGDEC_UNSTUFF_DEV = 1, snapshotted by the handle; 0: not launched, nothing allocated) in front of all of them: the scans were uploaded as they
//            stand in the files, and one workgroup per tile of 4096 raw bytes removes the 0xFF00 stuffing and the restart markers (jpeg_dec_plan.h, unstuff_keep)
//            from the clean offset the host's survey found for that tile.  NO WORKGROUP WAITS FOR ANOTHER, none reads what another wrote.
// The host side is jpeg_dec_pack.h's, plain C++ that knows nothing of this file: pack_room sizes a handle's block, pack_parse parses and classifies a batch (and
// refuses it before anything is touched), pack_fill plans every picture and writes the block in one of two layouts (clean scans in upload order; or raw scans with
// the clean areas behind the upload), and a PackResult tells jpegdec_launch the upload's size and the grids.  Here: wait for the last upload, upload once, launch.
// Everything runs on the caller's stream.
#include "common.h"
#include "config.h"
#include "jpeg_dec_pack.h"
#include "jpeg_dec_plan.h"

#define JD_THREADS 256
static_assert(JD_MAX_SUBSEQ == 16 * JD_THREADS, "16 subsequences per lane: the lane's `need` bits");      // per workgroup; more: a longer subsequence
#define JD_BLOCK_THREADS 256

struct omni_jpegdec {
    omni_ctx* ctx = nullptr;
    omni::jd::PackConfig cfg;              // the picture size, the batch, the capacity and the four switches, snapshotted
    omni::jd::PackRoom room;               // what pack_room makes of them: the block's size and the kernels' bounds
    omni::DevMem mem;
    uint8_t* d_in = nullptr;               // the uploaded block (jpeg_dec_pack.h: the two layouts); unstuff_dev: OMNI_JPEGDEC_GUARD_BYTES of 0xA5 behind the last
                                           // clean area in use
    int16_t* d_coef = nullptr;             // [max_images][nyb_max][64] + guard
    int32_t* d_dc = nullptr;               // [max_images][nyb_max] + guard
    int* d_flags = nullptr;                // [flag_words][max_images]: error bits, relaxation rounds, chunks that ran (plain_wgs >= 2: + seam rounds, subsequences
                                           // the seam relaxation changed) -- zeroed in front of every entropy launch
    int flag_words = 3;
    uint8_t* d_state = nullptr;            // plain_wgs >= 2: counts u32 | exit states u16 | entries used u16, each [max_images][state_cap], + guard
    omni::HostBuf hin;
    hipEvent_t ev_upload = nullptr;        // the pinned block is free again
    hipEvent_t ev_t[3] = {nullptr, nullptr, nullptr};      // in front of the upload, behind it, behind the kernels (omni_jpegdec_last_ms)
    bool timed = false;                    // ev_t hold ONE call's three events
    int last_n = 0;
    omni::jd::PackBatch batch;             // the last pack's descriptors as parsed (kept for its allocations)
    omni::jd::PackResult pack;             // what the last pack_fill wrote: the upload's size and the grids of jpegdec_launch
    std::mutex mu;
};

namespace omni {

// exclusive scan of one value per lane over a workgroup of kThreads (mod 2^32); *total = the sum.  lds: kThreads / 64 + 1 words, free again on return
template <int kThreads>
__device__ __forceinline__ uint32_t jd_wg_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = kThreads / 64;
    uint32_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < nw; ++i) { const uint32_t t = lds[i]; lds[i] = run; run += t; }
        lds[nw] = run;
    }
    __syncthreads();
    const uint32_t r = lds[wave] + incl - v;
    *total = lds[nw];
    __syncthreads();
    return r;
}

// The interval table of a picture as the entropy kernel sees it: a planned restart file's own table, or -- no restart interval -- the whole scan as ONE interval
struct JdIntervals {
    const jd::Interval* iv;                                 // null: one interval over the whole scan
    uint32_t total_bits, n_sub, n_blocks;
    __device__ __forceinline__ jd::Interval at(uint32_t k) const {
        if (iv) return iv[k];
        return k == 0 ? jd::Interval{0u, total_bits, 0u, 0u} : jd::Interval{total_bits, total_bits, n_sub, n_blocks};
    }
};

// Phases 1 and 2 over the N subsequences [sub0, sub0 + N) of the intervals [k0, k1), for the whole workgroup: ex / used / of / cnt [N] and *changed (zero on entry)
// in LDS; a barrier stands in front of the call and behind it.  The first subsequence of an interval -- and the first of the N, where the caller starts inside an
// interval: a chunk of a picture without a restart interval -- keeps the entry 0.  Returns the rounds that changed something, the same in every lane
__device__ __forceinline__ int jd_relax(const jd::Tables& T, const uint8_t* scan, uint32_t n_words, uint32_t S, const JdIntervals& ivs, uint32_t k0, uint32_t k1,
                                        uint32_t sub0, uint32_t N, uint16_t* ex, uint16_t* used, uint16_t* of, uint32_t* cnt, int* changed) {
    const int tid = threadIdx.x;
    jd::NoEmit none;
    int e;
    for (uint32_t i = tid; i < N; i += JD_THREADS) {                                        // 1: every subsequence from the guess
        const uint32_t k = ivs.iv ? jd::interval_of(ivs.iv, k0, k1, sub0 + i) : 0u;
        const jd::Interval I = ivs.at(k);
        uint16_t x;
        cnt[i] = jd::decode_subseq_seg(T, scan, n_words, I.bit_begin, I.bit_end, sub0 + i - I.first_sub, S, (uint16_t)0, 0u, 0xffffffffu, none, &x, &e);
        ex[i] = x;
        used[i] = 0;
        of[i] = (uint16_t)(k - k0);
    }
    __syncthreads();
    int rounds = 0;
    for (uint32_t r = 0; r < N; ++r) {                                                      // 2: relaxation; every lane runs the same number of rounds
        uint32_t need = 0;
        for (uint32_t i = tid, k = 0; i < N; i += JD_THREADS, ++k) {
            if (i == 0 || of[i] != of[i - 1]) continue;                                     // the first of its interval: the entry 0 is the true one
            const uint16_t en = ex[i - 1];
            if (en != used[i]) { used[i] = en; need |= 1u << k; }
        }
        __syncthreads();                                                                    // every entry is read before any exit is written
        for (uint32_t i = tid, k = 0; i < N; i += JD_THREADS, ++k) {
            if (!(need >> k & 1u)) continue;
            const jd::Interval I = ivs.at(k0 + of[i]);
            uint16_t x;
            const uint32_t c = jd::decode_subseq_seg(T, scan, n_words, I.bit_begin, I.bit_end, sub0 + i - I.first_sub, S, used[i], 0u, 0xffffffffu, none, &x, &e);
            if (x != ex[i] || c != cnt[i]) { ex[i] = x; cnt[i] = c; *changed = 1; }
        }
        __syncthreads();
        const int ch = *changed;
        __syncthreads();
        if (!ch) break;                                                                     // (uniform)
        if (tid == 0) *changed = 0;
        ++rounds;
    }
    __syncthreads();
    return rounds;
}

// the handle's state arrays (OMNI_JPEGDEC_PLAIN_WGS >= 2), each [max_images][cap]: what the chunk kernel leaves for the seam kernel, and that one for the write kernel
struct JdState {
    uint32_t* cnt;                                          // blocks completed (the seam kernel: + JD_SEAM_* marks; behind it: the first block)
    uint16_t *ex, *used;                                    // exit state; the entry it was last decoded from
    uint32_t cap;
};

// flags: [3][max_images] int32 zeroed on the stream in front of the launch -- error bits (OR), relaxation rounds (max), chunks that ran (+1): a picture's
// workgroups meet nowhere else, and none waits for another
__global__ __launch_bounds__(JD_THREADS) void jpegdec_entropy_kernel(const uint8_t* __restrict__ in, int16_t* __restrict__ coef, int32_t* __restrict__ dcd,
                                                                     uint32_t nyb_max, int* __restrict__ flags, int max_images) {
    __shared__ jd::Tables T;
    __shared__ uint16_t ex[JD_MAX_SUBSEQ], used[JD_MAX_SUBSEQ], of[JD_MAX_SUBSEQ];          // of: a subsequence's interval, counted from the chunk's first
    __shared__ uint32_t cnt[JD_MAX_SUBSEQ];
    __shared__ uint32_t lds[JD_THREADS / 64 + 1];
    __shared__ int changed, errflag;
    const int img = blockIdx.y, tid = threadIdx.x;
    const uint32_t chunk = blockIdx.x;
    const jd::Desc* d = reinterpret_cast<const jd::Desc*>(in) + img;
    if (d->mode != jd::JD_MODE_DECODE) return;                                              // (uniform: the whole workgroup leaves; the DC kernel writes the status)
    const uint32_t n_int = d->n_int, n_chunks = n_int ? d->n_chunks : 1u;
    if (chunk >= n_chunks) return;                                                          // (uniform)
    {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(&d->T);
        uint32_t* t = reinterpret_cast<uint32_t*>(&T);
        for (int i = tid; i < (int)(sizeof(jd::Tables) / 4); i += JD_THREADS) t[i] = s[i];
    }
    if (tid == 0) { changed = 0; errflag = 0; }
    const uint32_t S = d->subseq_bits, total_bits = d->total_bits, n_blocks = d->n_blocks;
    JdIntervals ivs{n_int ? reinterpret_cast<const jd::Interval*>(in + d->tab_off) : nullptr, total_bits, d->n_sub, n_blocks};
    uint32_t k0 = 0, k1 = 1;                                                                // the chunk's intervals [k0, k1)
    if (n_int) {
        const uint32_t* cf = reinterpret_cast<const uint32_t*>(ivs.iv + n_int + 1);
        k0 = cf[chunk]; k1 = cf[chunk + 1];
        if (k1 > n_int) k1 = n_int;
        if (k0 >= k1) return;                                                               // (uniform; the host plans no empty chunk)
    }
    const uint32_t sub0 = ivs.at(k0).first_sub, sub1 = ivs.at(k1).first_sub;
    const uint32_t N = sub1 - sub0 < JD_MAX_SUBSEQ ? sub1 - sub0 : JD_MAX_SUBSEQ;           // (the host made every chunk <= JD_MAX_SUBSEQ; the LDS arrays hold no more)
    const uint8_t* scan = in + d->dev_off;
    const uint32_t n_words = jd::scan_words((int64_t)(total_bits >> 3));
    __syncthreads();
    const int rounds = jd_relax(T, scan, n_words, S, ivs, k0, k1, sub0, N, ex, used, of, cnt, &changed);      // 1, 2
    int e;
    uint32_t carry = 0;                                                                     // 3: counts -> their exclusive prefix over the chunk, in place
    for (uint32_t base = 0; base < N; base += JD_THREADS) {
        const uint32_t i = base + tid;
        uint32_t sum;
        const uint32_t excl = jd_wg_scan<JD_THREADS>(i < N ? cnt[i] : 0u, lds, &sum);
        if (i < N) cnt[i] = carry + excl;
        carry += sum;
    }
    __syncthreads();
    int err = 0;
    for (uint32_t i = tid; i < N; i += JD_THREADS) {                                        // 4: the write pass, every interval bounded to its own blocks
        const uint32_t k = k0 + of[i];
        const jd::Interval I = ivs.at(k), next = ivs.at(k + 1);
        const uint32_t j = sub0 + i - I.first_sub;
        // the first block: the interval's + the counts before the subsequence INSIDE the interval (i - j: the interval's first subsequence, in this chunk)
        const uint32_t fb = I.first_block + (cnt[i] - cnt[i - j]);
        const uint32_t max_blocks = next.first_block < n_blocks ? next.first_block : n_blocks;
        jd::CoefEmit em;
        em.coef = coef + (size_t)img * nyb_max * 64;
        em.dcd = dcd + (size_t)img * nyb_max;
        em.n_yblocks = d->n_yblocks < nyb_max ? d->n_yblocks : nyb_max;
        const uint16_t entry = j == 0 ? (uint16_t)0 : used[i];
        em.start(T, fb, entry >> 12);
        uint16_t x;
        const uint32_t wrote = jd::decode_subseq_seg(T, scan, n_words, I.bit_begin, I.bit_end, j, S, entry, fb, max_blocks, em, &x, &e);
        err |= e;
        if (sub0 + i + 1 == next.first_sub && fb + wrote < max_blocks) err = 1;             // the interval's bits end before its blocks do
    }
    if (err) atomicOr(&errflag, 1);
    __syncthreads();
    if (tid == 0) {
        // (an empty scan completes no block; a chunk above the LDS arrays -- the host plans none -- would be decoded in part: CORRUPT, not OK)
        if (errflag || (N == 0 && n_blocks) || sub1 - sub0 > JD_MAX_SUBSEQ) atomicOr(&flags[img], 1);
        atomicMax(&flags[max_images + img], rounds);
        atomicAdd(&flags[2 * max_images + img], 1);
    }
}

// ---- a picture without a restart interval over several workgroups (OMNI_JPEGDEC_PLAIN_WGS >= 2; jpeg_dec_plan.h, plain) ------------------------------------------
__device__ __forceinline__ void jd_load_tables(jd::Tables* T, const jd::Desc* d) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&d->T);
    uint32_t* t = reinterpret_cast<uint32_t*>(T);
    for (int i = threadIdx.x; i < (int)(sizeof(jd::Tables) / 4); i += JD_THREADS) t[i] = s[i];
}

// chunk: grid (most chunks of a spread picture, images).  Phases 1-2 over the chunk's subsequences; nothing another workgroup wrote is read
__global__ __launch_bounds__(JD_THREADS) void jpegdec_chunk_kernel(const uint8_t* __restrict__ in, JdState st, int* __restrict__ flags, int max_images) {
    __shared__ jd::Tables T;
    __shared__ uint16_t ex[JD_MAX_SUBSEQ], used[JD_MAX_SUBSEQ], of[JD_MAX_SUBSEQ];
    __shared__ uint32_t cnt[JD_MAX_SUBSEQ];
    __shared__ int changed;
    const int img = blockIdx.y, tid = threadIdx.x;
    const jd::Desc* d = reinterpret_cast<const jd::Desc*>(in) + img;
    const uint32_t C = d->spread_chunks;
    if (d->mode != jd::JD_MODE_SPREAD || blockIdx.x >= C) return;                           // (uniform)
    const uint32_t n_sub = d->n_sub < st.cap ? d->n_sub : st.cap;                           // (the host plans no more; the seam kernel reports more as an error)
    const uint32_t sub0 = jd::plain_chunk_begin(blockIdx.x, n_sub, C), sub1 = jd::plain_chunk_begin(blockIdx.x + 1, n_sub, C);
    const uint32_t N = sub1 - sub0 < JD_MAX_SUBSEQ ? sub1 - sub0 : JD_MAX_SUBSEQ;           // (the host made every chunk <= JD_MAX_SUBSEQ; the LDS arrays hold no more)
    jd_load_tables(&T, d);
    if (tid == 0) changed = 0;
    const uint32_t total_bits = d->total_bits;
    const JdIntervals ivs{nullptr, total_bits, d->n_sub, d->n_blocks};                      // the whole scan as one interval; the chunk starts inside it
    __syncthreads();
    const int rounds = jd_relax(T, in + d->dev_off, jd::scan_words((int64_t)(total_bits >> 3)), d->subseq_bits, ivs, 0u, 1u, sub0, N, ex, used, of, cnt, &changed);
    const size_t at = (size_t)img * st.cap + sub0;
    for (uint32_t i = tid; i < N; i += JD_THREADS) {
        st.ex[at + i] = ex[i];
        st.used[at + i] = used[i];
        st.cnt[at + i] = cnt[i];
    }
    if (tid == 0) {
        if (sub1 - sub0 > JD_MAX_SUBSEQ) atomicOr(&flags[img], 1);                          // decoded in part: CORRUPT, not OK
        atomicMax(&flags[max_images + img], rounds);
        atomicAdd(&flags[2 * max_images + img], 1);
    }
}

// seam: one workgroup per picture, behind every workgroup of the chunk kernel (the stream orders them).  The relaxation of phase 2 over ALL the picture's
// subsequences, on the state arrays: after a round, only the subsequences behind one that changed can need another decode, so a round looks at [lo, hi) alone
// -- the same rounds and the same fixed point as looking at all of them.  The arrays are exchanged between the workgroup's waves across __syncthreads(): plain
// pointers, neither const nor __restrict__
__global__ __launch_bounds__(JD_THREADS) void jpegdec_seam_kernel(const uint8_t* __restrict__ in, uint32_t* cnt_all, uint16_t* ex_all, uint16_t* used_all, uint32_t cap,
                                                                  int* __restrict__ flags, int max_images) {
    __shared__ jd::Tables T;
    __shared__ uint32_t lds[JD_THREADS / 64 + 1];
    __shared__ int changed;
    __shared__ uint32_t lo_next, hi_next, n_moved;
    const int img = blockIdx.x, tid = threadIdx.x;
    const jd::Desc* d = reinterpret_cast<const jd::Desc*>(in) + img;
    if (d->mode != jd::JD_MODE_SPREAD) return;                                              // (uniform)
    const uint32_t N = d->n_sub < cap ? d->n_sub : cap;
    uint32_t* cnt = cnt_all + (size_t)img * cap;
    uint16_t* ex = ex_all + (size_t)img * cap;
    uint16_t* used = used_all + (size_t)img * cap;
    jd_load_tables(&T, d);
    if (tid == 0) { changed = 0; lo_next = 0xffffffffu; hi_next = 0u; n_moved = 0u; }
    const uint32_t S = d->subseq_bits, total_bits = d->total_bits;
    const uint8_t* scan = in + d->dev_off;
    const uint32_t n_words = jd::scan_words((int64_t)(total_bits >> 3));
    __syncthreads();
    jd::NoEmit none;
    int e, rounds = 0;
    uint32_t lo = 1u, hi = N;                                                               // the subsequences whose predecessor may have changed
    for (uint32_t r = 0; r < N; ++r) {                                                      // at most N rounds; every lane runs the same number
        for (uint32_t i = lo + tid; i < hi; i += JD_THREADS) {
            const uint16_t en = ex[i - 1];
            if (en != used[i]) { used[i] = en; cnt[i] |= JD_SEAM_NEED; }
        }
        __syncthreads();                                                                    // every entry is read before any exit is written
        for (uint32_t i = lo + tid; i < hi; i += JD_THREADS) {
            const uint32_t c0 = cnt[i];
            if (!(c0 & JD_SEAM_NEED)) continue;
            uint16_t x;
            const uint32_t c = jd::decode_subseq(T, scan, n_words, total_bits, i, S, used[i], 0u, 0xffffffffu, none, &x, &e) & JD_SEAM_COUNT;
            if (x != ex[i] || c != (c0 & JD_SEAM_COUNT)) {
                ex[i] = x;
                cnt[i] = c | JD_SEAM_CHANGED;
                changed = 1;
                atomicMin(&lo_next, i);
                atomicMax(&hi_next, i);
            } else {
                cnt[i] = c0 & ~JD_SEAM_NEED;
            }
        }
        __syncthreads();
        const int ch = changed;
        const uint32_t first = lo_next, last = hi_next;
        __syncthreads();
        if (!ch) break;                                                                     // (uniform)
        if (tid == 0) { changed = 0; lo_next = 0xffffffffu; hi_next = 0u; }
        lo = first + 1u;                                                                    // (first <= last < N)
        hi = last + 2u < N ? last + 2u : N;
        ++rounds;
    }
    __syncthreads();
    uint32_t carry = 0, moved = 0;                                                          // 3: counts -> their exclusive prefix over the picture, in place
    for (uint32_t base = 0; base < N; base += JD_THREADS) {
        const uint32_t i = base + tid, v = i < N ? cnt[i] : 0u;
        moved += v >> 30 & 1u;
        uint32_t sum;
        const uint32_t excl = jd_wg_scan<JD_THREADS>(v & JD_SEAM_COUNT, lds, &sum);
        if (i < N) cnt[i] = carry + excl;
        carry += sum;
    }
    if (moved) atomicAdd(&n_moved, moved);
    __syncthreads();
    if (tid == 0) {
        if (d->n_sub > cap) atomicOr(&flags[img], 1);                                       // (the host plans no such picture)
        atomicAdd(&flags[max_images + img], rounds);                                        // behind the chunk kernel's maximum: the picture's rounds
        flags[3 * max_images + img] = rounds;
        flags[4 * max_images + img] = (int)n_moved;
    }
}

// write: grid (ceil(most subsequences of a spread picture / JD_THREADS), images), one subsequence per lane: phase 4 from the stored entry and first block
__global__ __launch_bounds__(JD_THREADS) void jpegdec_write_kernel(const uint8_t* __restrict__ in, int16_t* __restrict__ coef, int32_t* __restrict__ dcd, uint32_t nyb_max,
                                                                   const uint32_t* __restrict__ first_all, const uint16_t* __restrict__ used_all, uint32_t cap,
                                                                   int* __restrict__ flags) {
    __shared__ jd::Tables T;
    const int img = blockIdx.y;
    const jd::Desc* d = reinterpret_cast<const jd::Desc*>(in) + img;
    if (d->mode != jd::JD_MODE_SPREAD) return;                                              // (uniform)
    const uint32_t N = d->n_sub < cap ? d->n_sub : cap;
    if (blockIdx.x * JD_THREADS >= N) return;                                               // (uniform)
    jd_load_tables(&T, d);
    __syncthreads();
    const uint32_t i = blockIdx.x * JD_THREADS + threadIdx.x;
    if (i >= N) return;                                                                     // (no barrier below)
    const uint32_t total_bits = d->total_bits, n_blocks = d->n_blocks, fb = first_all[(size_t)img * cap + i];
    const uint16_t entry = i ? used_all[(size_t)img * cap + i] : (uint16_t)0;
    jd::CoefEmit em;
    em.coef = coef + (size_t)img * nyb_max * 64;
    em.dcd = dcd + (size_t)img * nyb_max;
    em.n_yblocks = d->n_yblocks < nyb_max ? d->n_yblocks : nyb_max;
    em.start(T, fb, entry >> 12);
    uint16_t x;
    int e;
    const uint32_t wrote = jd::decode_subseq(T, in + d->dev_off, jd::scan_words((int64_t)(total_bits >> 3)), total_bits, i, d->subseq_bits, entry, fb, n_blocks, em, &x, &e);
    if (e || (i + 1 == N && fb + wrote < n_blocks)) atomicOr(&flags[img], 1);               // an error on the true chain, or the scan ends before the picture's last block
}

// one workgroup per image: the status, once, behind every workgroup of the entropy kernel; then the scan of the DC differences in scan order -- with a restart
// interval a segmented one: the running sum starts again every restart * ny blocks
__global__ __launch_bounds__(JD_THREADS) void jpegdec_dc_kernel(const uint8_t* __restrict__ in, int32_t* __restrict__ dcd, uint32_t nyb_max, const int* __restrict__ flags,
                                                                int* __restrict__ status) {
    __shared__ uint32_t lds[JD_THREADS / 64 + 1];
    __shared__ uint32_t tile[JD_THREADS];
    const jd::Desc* d = reinterpret_cast<const jd::Desc*>(in) + blockIdx.x;
    const bool dec = d->mode == jd::JD_MODE_DECODE || d->mode == jd::JD_MODE_SPREAD;
    if (threadIdx.x == 0) status[blockIdx.x] = dec && flags[blockIdx.x] ? OMNI_JPEGDEC_CORRUPT : d->status;
    if (!dec) return;
    const uint32_t n = d->n_yblocks < nyb_max ? d->n_yblocks : nyb_max;
    const uint32_t L = d->n_int ? (uint32_t)d->restart * (uint32_t)d->T.ny : 0u;            // blocks per segment (0: one segment)
    int32_t* v = dcd + (size_t)blockIdx.x * nyb_max;
    uint32_t carry = 0;                                                                     // the sum from the start of the segment that holds `base` up to base - 1
    for (uint32_t base = 0; base < n; base += JD_THREADS) {                                 // (uniform trip count: every lane reaches the barriers)
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < n ? (uint32_t)v[i] : 0u;
        uint32_t sum;
        const uint32_t incl = jd_wg_scan<JD_THREADS>(x, lds, &sum) + x;
        tile[threadIdx.x] = incl;
        __syncthreads();
        const uint32_t s = L ? i / L * L : 0u;                                              // the first block of i's segment
        if (i < n) v[i] = (int32_t)(s <= base ? carry + incl : incl - tile[s - 1 - base]);
        const uint32_t nb = base + JD_THREADS, sn = L ? nb / L * L : 0u;                    // the next tile's first block and its segment's start
        carry = sn <= base ? carry + sum : sum - tile[sn - 1 - base];
        __syncthreads();
    }
}

__global__ __launch_bounds__(JD_BLOCK_THREADS) void jpegdec_block_kernel(const uint8_t* __restrict__ in, const int16_t* __restrict__ coef, const int32_t* __restrict__ dcv,
                                                                         uint32_t nyb_max, const int* __restrict__ status, int w, int h, uint8_t* __restrict__ out,
                                                                         int64_t out_stride) {
    const int img = blockIdx.y;
    const uint32_t y = blockIdx.x * JD_BLOCK_THREADS + threadIdx.x;
    const jd::Desc* d = reinterpret_cast<const jd::Desc*>(in) + img;
    uint8_t* o = out + (int64_t)img * out_stride * h;
    if ((d->mode == jd::JD_MODE_DECODE || d->mode == jd::JD_MODE_SPREAD) && d->w == w && d->h == h) {
        if (y >= d->n_yblocks || y >= nyb_max) return;
        jd::block_out(*d, coef + (size_t)img * nyb_max * 64, dcv + (size_t)img * nyb_max, y, status[img] == OMNI_JPEGDEC_CORRUPT, o, out_stride);
        return;
    }
    // a picture that comes as pixels (decoded on the host), or as zeros: block y of the w x h picture in raster order
    const int bw = (w + 7) / 8, bh = (h + 7) / 8;
    if (y >= (uint32_t)(bw * bh)) return;
    const int bx = (int)(y % (uint32_t)bw), by = (int)(y / (uint32_t)bw);
    const uint8_t* px = d->mode == jd::JD_MODE_PIXELS ? in + d->dev_off : nullptr;
    for (int j = 0; j < 8 && by * 8 + j < h; ++j)
        for (int i = 0; i < 8 && bx * 8 + i < w; ++i) {
            const int64_t yy = by * 8 + j, xx = bx * 8 + i;
            o[yy * out_stride + xx] = px ? px[yy * w + xx] : (uint8_t)0;
        }
}

// ---- unstuffing on the device (OMNI_JPEGDEC_UNSTUFF_DEV = 1; jpeg_dec_plan.h, unstuff_keep / survey) ------------------------------------------------------------
// grid (most tiles of a scan, scans with a job); one workgroup compacts ONE tile of JD_UNSTUFF_TILE raw bytes, 16 per lane from one aligned 128-bit load: keep
// masks from unstuff_keep (the neighbour across a lane's edge from the adjacent lane, across a wave's or the tile's edge from global memory), popcounts, an
// exclusive scan over the workgroup, the kept bytes into LDS at the position their dwords have in global memory, then whole dwords where all four bytes are
// this tile's and single bytes for the ragged first and last dword -- the neighbouring tile's workgroup writes the other bytes of those.  The tile's clean
// offset is the host's (survey): no scan across workgroups, no atomics, no flags, NO WORKGROUP WAITS FOR ANOTHER, every loop has a constant trip count.  The
// workgroup of a scan's last tile also writes the JD_SCAN_PAD zero bytes (the clean area holds the last call's bytes).  Every store is checked against the
// scan's clean bytes, and a job that does not lie inside the block is not run at all.  `block` is read (jobs, tables, raw scans) and written (clean areas): no
// __restrict__, no const
#define JD_UNSTUFF_ROUNDS ((JD_UNSTUFF_TILE / 4 + 2 + JD_THREADS - 1) / JD_THREADS)
static_assert(JD_UNSTUFF_TILE == 16 * JD_THREADS, "16 raw bytes per lane");
__global__ __launch_bounds__(JD_THREADS) void jpegdec_unstuff_kernel(uint8_t* block, int64_t jobs_off, int64_t block_bytes) {
    __shared__ uint32_t lds[JD_THREADS / 64 + 1];
    __shared__ uint32_t stage[JD_UNSTUFF_TILE / 4 + 2];                                     // up to 3 bytes of the dword the tile's first clean byte lies in + the tile
    const jd::UnstuffJob J = reinterpret_cast<const jd::UnstuffJob*>(block + jobs_off)[blockIdx.y];
    const int64_t raw_end = J.raw_bytes, tile = blockIdx.x;
    if (raw_end < 0 || raw_end > block_bytes || J.clean_bytes < 0 || J.clean_bytes > raw_end) return;       // (uniform, as every return below)
    const int64_t n_tiles = ((raw_end > 1 ? raw_end : 1) + JD_UNSTUFF_TILE - 1) / JD_UNSTUFF_TILE, raw_room = (raw_end + 15) & ~(int64_t)15;
    if (tile >= n_tiles) return;
    if (J.raw_off < 0 || (J.raw_off & 15) || J.raw_off > block_bytes - raw_room || J.clean_off < 0 || (J.clean_off & 3) ||
        J.clean_off > block_bytes - J.clean_bytes - JD_SCAN_PAD || J.tile_off < 0 || (J.tile_off & 3) || J.tile_off > block_bytes - n_tiles * 4)
        return;                                                                             // (the host builds no such job)
    const uint8_t* raw = block + J.raw_off;
    uint8_t* clean = block + J.clean_off;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t base = tile * JD_UNSTUFF_TILE + tid * 16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (base < raw_end) {                                                                   // (16 bytes inside the zero-padded scan)
        const uint4 v = *reinterpret_cast<const uint4*>(raw + base);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    uint32_t prev = __shfl_up(w[3] >> 24, 1, 64), next = __shfl_down(w[0] & 255u, 1, 64);
    if (lane == 0) prev = base > 0 && base - 1 < raw_end ? raw[base - 1] : (uint32_t)JD_UNSTUFF_OUTSIDE;
    if (lane == 63) next = base + 16 < raw_end ? raw[base + 16] : (uint32_t)JD_UNSTUFF_OUTSIDE;
    uint32_t keep = 0;
    JP_UNROLL
    for (int b = 0; b < 16; ++b) {
        const uint32_t cur = w[b >> 2] >> (8 * (b & 3)) & 255u;
        const uint32_t p = b ? w[(b - 1) >> 2] >> (8 * ((b - 1) & 3)) & 255u : prev;
        const uint32_t nx = b < 15 ? w[(b + 1) >> 2] >> (8 * ((b + 1) & 3)) & 255u : next;
        const int64_t x = base + b;
        if (x < raw_end && jd::unstuff_keep((uint8_t)p, (uint8_t)cur, x + 1 < raw_end ? (uint8_t)nx : (uint8_t)JD_UNSTUFF_OUTSIDE)) keep |= 1u << b;
    }
    uint32_t total;
    const uint32_t excl = jd_wg_scan<JD_THREADS>((uint32_t)__popc(keep), lds, &total);
    const int64_t o0 = (int64_t)reinterpret_cast<const uint32_t*>(block + J.tile_off)[tile];
    const uint32_t a = (uint32_t)(o0 & 3), e = a + total;                                  // the tile's clean bytes are the staged bytes [a, e), e <= 3 + JD_UNSTUFF_TILE
    uint8_t* sb = reinterpret_cast<uint8_t*>(stage);
    uint32_t pos = a + excl;
    JP_UNROLL
    for (int b = 0; b < 16; ++b)
        if (keep >> b & 1u) sb[pos++] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    __syncthreads();
    const int64_t g0 = o0 - a;                                                              // the clean offset of staged byte 0: a multiple of 4
    JP_UNROLL
    for (int r = 0; r < JD_UNSTUFF_ROUNDS; ++r) {
        const uint32_t j = (uint32_t)(r * JD_THREADS + tid), lo = 4u * j, hi = lo + 4u;
        if (lo >= e) continue;
        if (lo >= a && hi <= e && g0 + hi <= J.clean_bytes) {
            *reinterpret_cast<uint32_t*>(clean + g0 + lo) = stage[j];
        } else {
            for (uint32_t k = lo > a ? lo : a; k < (hi < e ? hi : e); ++k)
                if (g0 + k < J.clean_bytes) clean[g0 + k] = sb[k];
        }
    }
    if (tile == n_tiles - 1 && tid < JD_SCAN_PAD) clean[J.clean_bytes + tid] = 0;
}

// The stage on `stream`; the caller holds d->mu, has checked the arguments, and d_in holds the block of n_images images
static int jpegdec_launch(omni_jpegdec* d, hipStream_t stream, int n_images, uint8_t* out_dev, int out_stride, int* status_dev) {
    if (d->cfg.unstuff_dev) {                                                               // the raw scans -> the clean areas behind the uploaded range, and the guard behind those
        OMNI_HIP_TRY(hipMemsetAsync(d->d_in + d->pack.clean_end, 0xA5, OMNI_JPEGDEC_GUARD_BYTES, stream));
        if (d->pack.n_jobs) {
            hipLaunchKernelGGL(jpegdec_unstuff_kernel, dim3((unsigned)d->pack.job_tiles, (unsigned)d->pack.n_jobs), dim3(JD_THREADS), 0, stream, d->d_in,
                               (int64_t)d->pack.jobs_off, (int64_t)d->pack.clean_end);
            OMNI_LAUNCH_CHECK();
        }
    }
    OMNI_HIP_TRY(hipMemsetAsync(d->d_coef, 0, (size_t)n_images * d->room.nyb_max * 64 * sizeof(int16_t), stream));
    OMNI_HIP_TRY(hipMemsetAsync(d->d_dc, 0, (size_t)n_images * d->room.nyb_max * sizeof(int32_t), stream));
    OMNI_HIP_TRY(hipMemsetAsync(d->d_flags, 0, (size_t)d->flag_words * d->cfg.max_images * sizeof(int), stream));
    if (d->pack.unspread) {                                                                 // (always, unless OMNI_JPEGDEC_PLAIN_WGS spread every picture of the batch)
        hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3(d->pack.max_chunks, n_images), dim3(JD_THREADS), 0, stream, d->d_in, d->d_coef, d->d_dc, d->room.nyb_max, d->d_flags,
                           d->cfg.max_images);
        OMNI_LAUNCH_CHECK();
    }
    if (d->pack.spread_chunks) {                                                            // pictures without a restart interval over several workgroups
        const size_t subs = (size_t)d->cfg.max_images * d->room.state_cap;
        JdState st{reinterpret_cast<uint32_t*>(d->d_state), reinterpret_cast<uint16_t*>(d->d_state + subs * 4), reinterpret_cast<uint16_t*>(d->d_state + subs * 6),
                   d->room.state_cap};
        hipLaunchKernelGGL(jpegdec_chunk_kernel, dim3(d->pack.spread_chunks, n_images), dim3(JD_THREADS), 0, stream, d->d_in, st, d->d_flags, d->cfg.max_images);
        OMNI_LAUNCH_CHECK();
        hipLaunchKernelGGL(jpegdec_seam_kernel, dim3(n_images), dim3(JD_THREADS), 0, stream, d->d_in, st.cnt, st.ex, st.used, st.cap, d->d_flags, d->cfg.max_images);
        OMNI_LAUNCH_CHECK();
        hipLaunchKernelGGL(jpegdec_write_kernel, dim3(cdiv((int)d->pack.spread_sub, JD_THREADS), n_images), dim3(JD_THREADS), 0, stream, d->d_in, d->d_coef, d->d_dc,
                           d->room.nyb_max, st.cnt, st.used, st.cap, d->d_flags);
        OMNI_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(jpegdec_dc_kernel, dim3(n_images), dim3(JD_THREADS), 0, stream, d->d_in, d->d_dc, d->room.nyb_max, d->d_flags, status_dev);
    OMNI_LAUNCH_CHECK();
    const int raster = cdiv(d->cfg.w, 8) * cdiv(d->cfg.h, 8);
    const int per_image = (int)d->room.nyb_max > raster ? (int)d->room.nyb_max : raster;
    hipLaunchKernelGGL(jpegdec_block_kernel, dim3(cdiv(per_image, JD_BLOCK_THREADS), n_images), dim3(JD_BLOCK_THREADS), 0, stream, d->d_in, d->d_coef, d->d_dc,
                       d->room.nyb_max, status_dev, d->cfg.w, d->cfg.h, out_dev, (int64_t)out_stride);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

// Parses the files and fills the handle's pinned block (jpeg_dec_pack.h: pack_parse, pack_fill -> d->pack).  The parse overlaps the last upload; nothing is
// touched when a file is refused
static int jpegdec_pack(omni_jpegdec* d, const uint8_t* const* files, const int64_t* sizes, int n_images) {
    jd::PackRefusal no;
    if (jd::pack_parse(d->cfg, d->room, files, sizes, n_images, &d->batch, &no)) { set_error("%s", no.message.c_str()); return no.code; }
    if (d->ev_upload) OMNI_HIP_TRY(hipEventSynchronize(d->ev_upload));                        // the last upload has left the pinned block
    if (jd::pack_fill(d->cfg, d->room, d->batch, files, d->hin.as<uint8_t>(), &d->pack, &no)) { set_error("%s", no.message.c_str()); return no.code; }
    return OMNI_OK;
}

}  // namespace omni

extern "C" omni_jpegdec* omni_jpegdec_create(omni_ctx* ctx, int width, int height, int max_images, int64_t capacity_per_image) {
    using namespace omni;
    if (!ctx) { set_error("null context"); return nullptr; }
    if (width < 1 || height < 1 || width > 65535 || height > 65535) { set_error("omni_jpegdec_create: %dx%d outside 1..65535", width, height); return nullptr; }
    const int64_t nyb = jd::pack_nyb(width, height);
    if (nyb > (1 << 20)) { set_error("omni_jpegdec_create: %dx%d is more than 2^20 blocks", width, height); return nullptr; }
    if (max_images < 1 || max_images > 65535) { set_error("omni_jpegdec_create: max_images=%d outside [1, 65535]", max_images); return nullptr; }
    if (capacity_per_image < 1024 || capacity_per_image > (1 << 28)) {
        set_error("omni_jpegdec_create: a capacity of %lld bytes outside [1024, 2^28]", (long long)capacity_per_image);
        return nullptr;
    }
    Config cfg;
    if (config_resolve(&cfg) != OMNI_OK) return nullptr;
    const int S = cfg[CFG_JPEGDEC_SUBSEQ_BITS];
    if (S & (S - 1)) { set_error("OMNI_JPEGDEC_SUBSEQ_BITS=%d: expected a power of two", S); return nullptr; }
    const int W = cfg[CFG_JPEGDEC_RESTART_WGS], PW = cfg[CFG_JPEGDEC_PLAIN_WGS];
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    omni_jpegdec* d = new omni_jpegdec();
    d->ctx = ctx;
    d->cfg.w = width; d->cfg.h = height; d->cfg.max_images = max_images; d->cfg.capacity = capacity_per_image;
    d->cfg.subseq_bits = S; d->cfg.restart_wgs = W; d->cfg.plain_wgs = PW; d->cfg.unstuff_dev = cfg[CFG_JPEGDEC_UNSTUFF_DEV];
    d->room = jd::pack_room(d->cfg);
    // OMNI_JPEGDEC_UNSTUFF_DEV = 1: the guard stands behind the last clean area in use
    if (d->cfg.unstuff_dev) d->pack.clean_end = d->room.in_bytes;
    const size_t in_guard = d->cfg.unstuff_dev ? OMNI_JPEGDEC_GUARD_BYTES : 0;
    const size_t coef_bytes = (size_t)max_images * nyb * 64 * sizeof(int16_t), dc_bytes = (size_t)max_images * nyb * sizeof(int32_t);
    // OMNI_JPEGDEC_PLAIN_WGS >= 2: the state arrays of the spread path (8 bytes per subsequence) and two more flag words per picture; otherwise neither
    if (PW >= 2) d->flag_words = 5;
    const size_t state_bytes = (size_t)max_images * d->room.state_cap * 8;
    auto make = [&]() -> int {
        int rc;
        if ((rc = d->mem.alloc(&d->d_in, d->room.in_bytes + in_guard)) ||(rc = d->mem.alloc(&d->d_coef, coef_bytes + OMNI_JPEGDEC_GUARD_BYTES)) ||
            (rc = d->mem.alloc(&d->d_dc, dc_bytes + OMNI_JPEGDEC_GUARD_BYTES)) || (rc = d->mem.alloc(&d->d_flags, (size_t)d->flag_words * max_images * sizeof(int))))
            return rc;
        if (state_bytes) {
            if ((rc = d->mem.alloc(&d->d_state, state_bytes + OMNI_JPEGDEC_GUARD_BYTES))) return rc;
            OMNI_HIP_TRY(hipMemset(d->d_state + state_bytes, 0xA5, OMNI_JPEGDEC_GUARD_BYTES));
        }
        if (in_guard) OMNI_HIP_TRY(hipMemset(d->d_in + d->room.in_bytes, 0xA5, in_guard));
        OMNI_HIP_TRY(hipMemset(reinterpret_cast<uint8_t*>(d->d_coef) + coef_bytes, 0xA5, OMNI_JPEGDEC_GUARD_BYTES));
        OMNI_HIP_TRY(hipMemset(reinterpret_cast<uint8_t*>(d->d_dc) + dc_bytes, 0xA5, OMNI_JPEGDEC_GUARD_BYTES));
        OMNI_HIP_TRY(hipMemset(d->d_flags, 0, (size_t)d->flag_words * max_images * sizeof(int)));
        if ((rc = d->hin.ensure(d->room.in_bytes))) return rc;
        OMNI_HIP_TRY(hipEventCreateWithFlags(&d->ev_upload, hipEventDisableTiming));
        for (hipEvent_t& e : d->ev_t) OMNI_HIP_TRY(hipEventCreate(&e));
        return OMNI_OK;
    };
    if (make() != OMNI_OK) {
        d->mem.release_all(); d->hin.release();
        if (d->ev_upload) (void)hipEventDestroy(d->ev_upload);
        for (hipEvent_t e : d->ev_t)
            if (e) (void)hipEventDestroy(e);
        delete d;
        return nullptr;
    }
    return d;
}

extern "C" void omni_jpegdec_destroy(omni_jpegdec* d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipDeviceSynchronize();
    d->mem.release_all();
    d->hin.release();
    if (d->ev_upload) (void)hipEventDestroy(d->ev_upload);
    for (hipEvent_t e : d->ev_t)
        if (e) (void)hipEventDestroy(e);
    delete d;
}

namespace omni {
// The whole stage on `stream` (cam.hip: the unit's SuperPoint stream; the caller serialises its use of that stream): parse + pack under the handle's own lock,
// then upload + kernels.  Refusals come before anything is enqueued.
int jpegdec_enqueue_on(omni_jpegdec* d, hipStream_t stream, const uint8_t* const* files, const int64_t* sizes, int n_images, uint8_t* out_dev, int out_stride,
                       int* status_dev) {
    OMNI_REQUIRE(d && files && sizes && out_dev && status_dev, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(n_images >= 1 && n_images <= d->cfg.max_images, OMNI_ERR_INVALID, "omni_jpegdec: %d images, the handle holds 1..%d", n_images, d->cfg.max_images);
    OMNI_REQUIRE(out_stride >= d->cfg.w, OMNI_ERR_INVALID, "omni_jpegdec: out_stride %d for pictures %d wide", out_stride, d->cfg.w);
    std::lock_guard<std::mutex> lk(d->mu);
    (void)hipSetDevice(d->ctx->device);
    int rc;
    if ((rc = jpegdec_pack(d, files, sizes, n_images))) return rc;
    d->timed = false;                                                                       // (until this call's three events are all recorded)
    OMNI_HIP_TRY(hipEventRecord(d->ev_t[0], stream));
    OMNI_HIP_TRY(hipMemcpyAsync(d->d_in, d->hin.p, d->pack.upload_bytes, hipMemcpyHostToDevice, stream));
    OMNI_HIP_TRY(hipEventRecord(d->ev_upload, stream));
    OMNI_HIP_TRY(hipEventRecord(d->ev_t[1], stream));
    d->last_n = n_images;
    if ((rc = jpegdec_launch(d, stream, n_images, out_dev, out_stride, status_dev))) return rc;
    OMNI_HIP_TRY(hipEventRecord(d->ev_t[2], stream));
    d->timed = true;
    return OMNI_OK;
}
}  // namespace omni

extern "C" int omni_jpegdec_enqueue_host(omni_jpegdec* d, const uint8_t* const* files, const int64_t* sizes, int n_images, uint8_t* out_dev, int out_stride,
                                         int* status_dev) {
    OMNI_REQUIRE(d, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("jpeg decode (camera frames)");
    return omni::jpegdec_enqueue_on(d, d->ctx->stream, files, sizes, n_images, out_dev, out_stride, status_dev);
}

extern "C" int omni_jpegdec_last_ms(omni_jpegdec* d, float* upload_ms, float* kernels_ms, int64_t* uploaded_bytes) {
    OMNI_REQUIRE(d && upload_ms && kernels_ms && uploaded_bytes, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(d->mu);
    OMNI_REQUIRE(d->last_n > 0 && d->timed, OMNI_ERR_INVALID, "omni_jpegdec_last_ms: no enqueue of this handle has run to its end");
    (void)hipSetDevice(d->ctx->device);
    OMNI_HIP_TRY(hipEventSynchronize(d->ev_t[2]));
    OMNI_HIP_TRY(hipEventElapsedTime(upload_ms, d->ev_t[0], d->ev_t[1]));
    OMNI_HIP_TRY(hipEventElapsedTime(kernels_ms, d->ev_t[1], d->ev_t[2]));
    *uploaded_bytes = (int64_t)d->pack.upload_bytes;
    return OMNI_OK;
}

extern "C" int omni_jpegdec_last_stats(omni_jpegdec* d, int* rounds, int* n_subseq, int* subseq_bits) {
    OMNI_REQUIRE(d, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(d->mu);
    (void)hipSetDevice(d->ctx->device);
    OMNI_HIP_TRY(hipDeviceSynchronize());                                                     // (the last enqueue may have run on a unit's stream)
    if (rounds && d->last_n) OMNI_HIP_TRY(hipMemcpy(rounds, d->d_flags + d->cfg.max_images, (size_t)d->last_n * sizeof(int), hipMemcpyDeviceToHost));
    const omni::jd::Desc* descs = d->hin.as<omni::jd::Desc>();                                // (the pinned block still holds the last enqueue's descriptors)
    for (int i = 0; i < d->last_n; ++i) {
        const bool dec = descs[i].mode == omni::jd::JD_MODE_DECODE || descs[i].mode == omni::jd::JD_MODE_SPREAD;
        if (n_subseq) n_subseq[i] = dec ? (int)descs[i].n_sub : 0;
        if (subseq_bits) subseq_bits[i] = dec ? (int)descs[i].subseq_bits : 0;
    }
    return OMNI_OK;
}

extern "C" int omni_jpegdec_last_chunks(omni_jpegdec* d, int* chunks) {
    OMNI_REQUIRE(d && chunks, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(d->mu);
    (void)hipSetDevice(d->ctx->device);
    OMNI_HIP_TRY(hipDeviceSynchronize());
    if (d->last_n) OMNI_HIP_TRY(hipMemcpy(chunks, d->d_flags + 2 * (size_t)d->cfg.max_images, (size_t)d->last_n * sizeof(int), hipMemcpyDeviceToHost));
    return OMNI_OK;
}

extern "C" int omni_jpegdec_last_seam(omni_jpegdec* d, int* seam_rounds, int* seam_changed) {
    OMNI_REQUIRE(d, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(d->mu);
    (void)hipSetDevice(d->ctx->device);
    OMNI_HIP_TRY(hipDeviceSynchronize());
    int* const out[2] = {seam_rounds, seam_changed};
    for (int k = 0; k < 2; ++k) {
        if (!out[k] || !d->last_n) continue;
        if (d->flag_words < 5) memset(out[k], 0, (size_t)d->last_n * sizeof(int));            // (the switch is off: no picture has a seam)
        else OMNI_HIP_TRY(hipMemcpy(out[k], d->d_flags + (size_t)(3 + k) * d->cfg.max_images, (size_t)d->last_n * sizeof(int), hipMemcpyDeviceToHost));
    }
    return OMNI_OK;
}

extern "C" int omni_jpegdec_debug_state_buffer(omni_jpegdec* d, void** state_dev, int64_t* state_bytes) {
    OMNI_REQUIRE(d && state_dev && state_bytes, OMNI_ERR_INVALID, "null argument");
    *state_dev = d->d_state; *state_bytes = (int64_t)d->cfg.max_images * d->room.state_cap * 8;
    return OMNI_OK;
}

extern "C" int omni_jpegdec_last_unstuff(omni_jpegdec* d, int* device_pictures, int64_t* raw_bytes, int64_t* clean_bytes) {
    OMNI_REQUIRE(d && device_pictures && raw_bytes && clean_bytes, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(d->mu);
    *device_pictures = d->cfg.unstuff_dev ? d->pack.n_jobs : 0;
    *raw_bytes = d->cfg.unstuff_dev ? d->pack.raw_bytes : 0;
    *clean_bytes = d->cfg.unstuff_dev ? d->pack.clean_bytes : 0;
    return OMNI_OK;
}

extern "C" int omni_jpegdec_debug_in_buffer(omni_jpegdec* d, void** clean_end_dev, int64_t* guard_bytes) {
    OMNI_REQUIRE(d && clean_end_dev && guard_bytes, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(d->mu);
    *clean_end_dev = d->cfg.unstuff_dev ? d->d_in + d->pack.clean_end : nullptr;
    *guard_bytes = d->cfg.unstuff_dev ? OMNI_JPEGDEC_GUARD_BYTES : 0;
    return OMNI_OK;
}

// survey, upload, jpegdec_unstuff_kernel alone, download: a block of its own -- job | tile table | raw scan | clean area | guard -- filled with 0xA5 beforehand
extern "C" int omni_jpegdec_unstuff_dev(omni_ctx* ctx, const uint8_t* scan, int64_t n, uint8_t* out_host, int64_t out_cap, int64_t* n_clean) {
    using namespace omni;
    OMNI_REQUIRE(ctx && scan && out_host && n_clean, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(n >= 0 && n <= (1 << 28), OMNI_ERR_INVALID, "omni_jpegdec_unstuff_dev: a scan of %lld bytes outside [0, 2^28]", (long long)n);
    std::vector<uint32_t> tiles((size_t)(n / JD_UNSTUFF_TILE + 1));
    const jd::Survey v = jd::survey(scan, n, tiles.data(), (int64_t)tiles.size(), nullptr, 0);
    OMNI_REQUIRE(out_cap >= v.n_clean + JD_SCAN_PAD, OMNI_ERR_INVALID, "omni_jpegdec_unstuff_dev: room for %lld bytes, %lld clean bytes + %d", (long long)out_cap,
                 (long long)v.n_clean, JD_SCAN_PAD);
    const size_t tiles_off = jd::pack_align16(sizeof(jd::UnstuffJob)), raw_off = tiles_off + jd::pack_align16((size_t)v.n_tiles * sizeof(uint32_t)), clean_off = raw_off + jd::pack_align16((size_t)v.raw_end);
    const size_t clean_end = clean_off + jd::pack_align16((size_t)v.n_clean + JD_SCAN_PAD);
    std::vector<uint8_t> host(clean_off, 0);
    const jd::UnstuffJob job{(int64_t)raw_off, v.raw_end, (int64_t)clean_off, v.n_clean, (int64_t)tiles_off};
    memcpy(host.data(), &job, sizeof(job));
    memcpy(host.data() + tiles_off, tiles.data(), (size_t)v.n_tiles * sizeof(uint32_t));
    if (v.raw_end) memcpy(host.data() + raw_off, scan, (size_t)v.raw_end);
    std::vector<uint8_t> back(clean_end - clean_off + OMNI_JPEGDEC_GUARD_BYTES);
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    DevMem mem;
    uint8_t* block = nullptr;
    auto run = [&]() -> int {
        int rc;
        if ((rc = mem.alloc(&block, clean_end + OMNI_JPEGDEC_GUARD_BYTES))) return rc;
        OMNI_HIP_TRY(hipMemsetAsync(block, 0xA5, clean_end + OMNI_JPEGDEC_GUARD_BYTES, ctx->stream));
        OMNI_HIP_TRY(hipMemcpyAsync(block, host.data(), clean_off, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(jpegdec_unstuff_kernel, dim3((unsigned)v.n_tiles, 1), dim3(JD_THREADS), 0, ctx->stream, block, (int64_t)0, (int64_t)clean_end);
        OMNI_LAUNCH_CHECK();
        OMNI_HIP_TRY(hipMemcpyAsync(back.data(), block + clean_off, back.size(), hipMemcpyDeviceToHost, ctx->stream));
        OMNI_HIP_TRY(hipStreamSynchronize(ctx->stream));
        return OMNI_OK;
    };
    const int rc = run();
    if (block) (void)hipStreamSynchronize(ctx->stream);
    mem.release_all();
    if (rc) return rc;
    for (size_t i = clean_end - clean_off; i < back.size(); ++i)
        OMNI_REQUIRE(back[i] == 0xA5, OMNI_ERR_HIP, "omni_jpegdec_unstuff_dev: the kernel wrote behind the clean area (guard byte %zu)", i - (clean_end - clean_off));
    for (size_t i = (size_t)v.n_clean + JD_SCAN_PAD; i < clean_end - clean_off; ++i)
        OMNI_REQUIRE(back[i] == 0xA5, OMNI_ERR_HIP, "omni_jpegdec_unstuff_dev: the kernel wrote behind the padding (byte %zu)", i);
    memcpy(out_host, back.data(), (size_t)v.n_clean + JD_SCAN_PAD);
    *n_clean = v.n_clean;
    return OMNI_OK;
}

extern "C" int omni_jpegdec_debug_buffers(omni_jpegdec* d, void** coef_dev, int64_t* coef_bytes, void** dc_dev, int64_t* dc_bytes) {
    OMNI_REQUIRE(d && coef_dev && coef_bytes && dc_dev && dc_bytes, OMNI_ERR_INVALID, "null argument");
    *coef_dev = d->d_coef; *coef_bytes = (int64_t)d->cfg.max_images * d->room.nyb_max * 64 * (int64_t)sizeof(int16_t);
    *dc_dev = d->d_dc; *dc_bytes = (int64_t)d->cfg.max_images * d->room.nyb_max * (int64_t)sizeof(int32_t);
    return OMNI_OK;
}
