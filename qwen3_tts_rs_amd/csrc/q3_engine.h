// q3_engine.h — what the translation units of the engine share (not part of the C ABI; include/q3tts.h is).
// Round 6: q3_engine.hip (3 800 lines: model, arena, KV pool, session, graph capture, batcher, test entry points) was split into
//   q3_model.hip     errors, synthetic tensors, the weight manifest / arena, q3_model_* (create, set_tensor, finalize, KV pool API)
//   q3_prefix_cache.hip the prefix cache: prefilled instruct pages shared across requests (q3_prefix_cache.h)
//   q3_codec_run.hip device-memory cache, the vocoder pipeline (codec_decode_dev) and q3_decode_codes
//   q3_codec_stream.hip the codec stream: the vocoder with per-row state, many rows per pass
//   q3_pcm_stage.hip the output stage, per row a chain of steps: silence trim and pause cap -> speaking rate
//                    (WSOLA) -> pitch in cents (varispeed) -> BS.1770 loudness meter / normaliser -> level (gain and look-ahead peak
//                    limiter) -> resampling to a requested rate as f32, PCM16 or G.711 bytes
//   q3_intake.hip    the reference-audio intake: a clip in its on-disk sample format -> 24 kHz mono f32 on the device in one launch,
//                    where both encoders read it
//   q3_session.hip   sessions: KV paging, the talker / code-predictor step, frame capture + own-queue submission, prefill, generate,
//                    streaming chunks, q3_session_run / decode / get
//   q3_batcher.hip   continuous batching: q3_session_replace (side prefill + transplant) and the native batcher q3_batcher_*
//   q3_row_state.hip a running row's state as an object: k_row_move, q3_session_park_row / _resume_row, q3_parked_* 
//   q3_testapi.hip   low-level entry points of the parity tests and of bench.py's roofline replays
// Together they are the host side of libq3tts.so: weight arena, sessions (KV pages, RNG streams, penalty masks), the per-frame
// launch sequence (captured once, replayed from the library's own AQL queue), the codec-decoder pipeline and the C ABI declared in
// include/q3tts.h. Layer map of the reference they replace (paths relative to the reference repo):
//   src/lib.rs:530-656 generate_codes, 425-501 synthesize_with_timing, 718-784 / 1484-1541 per-call state, 1484-1782 StreamingSession
//   src/models/talker.rs:451-627 prefill builders, 716-736 generate_step_with_embed
//   src/models/code_predictor.rs:320-416 generate_acoustic_codes
//   src/models/codec/decoder_12hz.rs:411-505 decode
// No behaviour change: the functions moved as they were; the ones another unit calls lost their `static` and are declared below
// (hidden visibility: the .so exports exactly what include/q3tts.h declares).
#pragma once
#include "../../include/q3tts.h"
#include "q3_kernels.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "q3_internal.h"
#include "q3_aql.h"

using namespace q3;
#define Q3_HIDDEN __attribute__((visibility("hidden")))

// ------------------------------------------------------------------------------------------------
// errors (q3_model.hip): thread-local message behind q3_last_error()
// ------------------------------------------------------------------------------------------------
Q3_HIDDEN q3_status set_err(q3_status st, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// Every host thread that calls into the engine runs its HIP calls in RELAXED stream-capture mode: a session captures its frame
// (kernel launches only, on its own non-blocking stream) while other threads — the batcher's prefill worker, a server's other
// sessions — allocate, hipMemcpy and synchronise; with the default (global) thread mode this HIP runtime fails THOSE calls with
// "operation not permitted when stream is capturing" whatever mode the capture itself was begun in.
static inline void q3_relax_capture_mode() {
    static thread_local bool done = false;
    if (!done) { hipStreamCaptureMode m = hipStreamCaptureModeRelaxed; (void)hipThreadExchangeStreamCaptureMode(&m); done = true; }
}
// ... and that is not enough on this runtime: an operation on the LEGACY (null) stream — a synchronous hipMemcpy, the zero-fills of
// DevPool, hipDeviceSynchronize — issued by one thread while another thread's stream is capturing fails with "operation would
// make the legacy stream depend on a capturing blocking stream" (and invalidates the capture), non-blocking capturing stream and
// relaxed modes notwithstanding (tests/test_frame_submission.py: two sessions on two threads). So the two exclude each other:
// a capture (q3_session.hip frame_capture: ~1 ms of kernel launches, once per session) holds this lock exclusively, every
// legacy-stream operation of the engine holds it shared (the q3_hip* wrappers below; the engine's units call nothing else).
#include "q3_capture_lock.h"
#define HIPC(expr)                                                                                        \
    do {                                                                                                  \
        q3_relax_capture_mode();                                                                          \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return set_err(Q3_HIP_ERROR, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                           __LINE__);                                                                     \
    } while (0)
#define Q3C(expr)                         \
    do {                                  \
        q3_status s_ = (expr);            \
        if (s_ != Q3_OK) return s_;       \
    } while (0)

// token ids (talker.rs:30-55)
enum { IM_START = 151644, ASSISTANT = 77091, NEWLINE = 198, TTS_PAD = 151671, TTS_BOS = 151672, TTS_EOS = 151673 };
enum { CODEC_PAD = 2148, CODEC_BOS = 2149, CODEC_EOS = 2150, CODEC_THINK = 2154, CODEC_THINK_BOS = 2156, CODEC_THINK_EOS = 2157 };

static inline uint16_t f32_to_bf16_host(float f) {
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32_host(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }

// ------------------------------------------------------------------------------------------------
// model
// ------------------------------------------------------------------------------------------------
enum SlotKind { SK_PLAIN = 0, SK_TRANSCONV = 1, SK_TILED = 2 };
struct Slot {
    std::string name; int64_t n = 0; int stored = Q3_DTYPE_F32; size_t offset = 0; bool loaded = false;
    int kind = SK_PLAIN; int tc_cin = 0, tc_cout = 0, tc_k = 0, tc_stride = 0;
    int rows = 0, cols = 0;      // SK_TILED: logical [rows][cols]; 16-row-tile image at `offset`,
    size_t offset2 = 0; bool dual = false;   // plus a 4-row-tile image at `offset2` when the projection is narrow
};
// a GEMV weight: 16-row-tile image (t1) and, for narrow projections, a 4-row-tile image (t2)
struct TW { const uint16_t* t1 = nullptr; const uint16_t* t2 = nullptr; };
struct LayerW {
    const float *in_ln, *q_norm, *k_norm, *post_ln;
    TW qkv, o, gate, up, down;
};

struct DecLayerW { const float *in_ln, *q, *k, *v, *o, *attn_scale, *post_ln, *gate, *up, *down, *mlp_scale; };
struct ResUnitW { const float *a1, *ib1, *c1w, *c1b, *a2, *ib2, *c2w, *c2b; };
struct DecBlockW { const float *a, *ib, *tw, *tb; ResUnitW res[3]; int cin, cout, rate; };
struct UpW { const float *tw, *tb, *dww, *dwb, *nw, *nb, *p1w, *p1b, *p2w, *p2b, *gamma; int ratio; };

// ------------------------------------------------------------------------------------------------
// Paged talker KV (north_star: "in-place paged KV in 288 GB HBM3E"; replaces the per-call preallocated cache of
// kv_cache.rs:234-310 and its overflow bail :293-300). One pool per model: pages of KV_PAGE_POS positions x every layer
// and KV head (q3_kernels.h), carved from 32-page slabs that are hipMalloc'ed on demand and kept for the model's lifetime. Sessions
// take pages as their rows cross page boundaries and hand them back when a row is replaced or the session ends, so a
// 4k-position prompt and a ten-position prompt draw on the same memory, and a continuous-batching swap RELINKS the
// prefilled pages of the side session into the row instead of copying extents. Pages are never cleared: the attention
// kernels read a position only after it was written.
// ------------------------------------------------------------------------------------------------
// One page budget for both pools of a model (q3_model_kv_pool_limit), in UNITS of half an f32 page: an f32 page costs 2, a
// bf16 page (same geometry, 2-byte elements) 1 — so the documented limit, the Q3_KV_OVERFLOW bail and the occupancy figures hold
// for bf16 sessions and for the f32 pages their prompts are prefilled into alike.
struct KvBudget {
    std::mutex mu;
    long limit = 0, used = 0, peak = 0;            // units; limit 0 = bounded by HBM only
    bool fits(long units) { std::lock_guard<std::mutex> g(mu); return limit <= 0 || used + units <= limit; }
};
struct KvPool {
    // Slab layout (layer-major, so that ONE layer's K/V of every page of a slab sits in one contiguous run — the attention
    // launch of a layer touches SLAB_SLOTS x 512 KB = 16 MB runs instead of one 64 KB run per (page, head) spread 29 MB
    // apart, which cost ~1 us of address translation per launch at B = 8: the frame was 0.9 % slower than with contiguous
    // extents):   slab[n_layers][2 (K, V)][SLAB_SLOTS][nkv][KV_PAGE_POS][HEAD_DIM] f32 (+ padding, below).
    // A page = one slot of a slab, named by the address of its layer-0 K run; layer l is `l * layer_stride()` floats further,
    // V `v_delta()` floats behind K.
    static constexpr int SLAB_SLOTS = 32;
    std::mutex mu;
    size_t run_floats = 0; int n_layers = 0;       // run = nkv * KV_PAGE_POS * HEAD_DIM ELEMENTS (one layer's K of one page)
    size_t elem_bytes = sizeof(float);              // 4, or 2 for the pool of bf16 sessions (same geometry in elements)
    std::vector<void*> slabs; std::vector<float*> free_pages;
    int total = 0, in_use = 0;                      // pages of this pool
    KvBudget* budget = nullptr; int unit = 2;       // the model's shared budget and what one page of this pool costs of it
    // K -> V and layer -> layer distances are kept OFF powers of two (17 KB of padding behind every region): a lane asks for
    // the K row and the V row of a position together, and at exactly 16 MB apart the two requests meet in the same memory
    // channel (k_attn_fused 7.6 vs 6.9 us per launch at B = 8 against the contiguous caches, whose distance is arbitrary)
    static constexpr size_t PAD_FLOATS = 17 * 256;
    size_t page_bytes() const { return (size_t)2 * n_layers * run_floats * elem_bytes; }
    size_t v_delta() const { return (size_t)SLAB_SLOTS * run_floats + PAD_FLOATS; }
    size_t layer_stride() const { return 2 * v_delta(); }
    size_t slab_bytes() const { return (size_t)n_layers * layer_stride() * elem_bytes; }
    // n pages or none: hipErrorOutOfMemory when the limit (q3_model_kv_pool_limit) or the device says no
    hipError_t take(int n, std::vector<float*>& out) {
        std::lock_guard<std::mutex> g(mu);
        if (n <= 0) return hipSuccess;
        {
            std::lock_guard<std::mutex> gb(budget->mu);
            if (budget->limit > 0 && budget->used + (long)n * unit > budget->limit) return hipErrorOutOfMemory;
        }
        while ((int)free_pages.size() < n) {          // whole slabs (~1 GB at 28 layers x 8 KV heads), kept for the model's lifetime: no hipMalloc in steady state
            void* slab = nullptr;
            if (hipMalloc(&slab, slab_bytes()) != hipSuccess) { (void)hipGetLastError(); return hipErrorOutOfMemory; }
            slabs.push_back(slab);
            for (int i = SLAB_SLOTS - 1; i >= 0; --i) free_pages.push_back((float*)((char*)slab + (size_t)i * run_floats * elem_bytes));
            total += SLAB_SLOTS;
        }
        for (int i = 0; i < n; ++i) { out.push_back(free_pages.back()); free_pages.pop_back(); }
        in_use += n;
        std::lock_guard<std::mutex> gb(budget->mu);      // (sessions of one model may run on several host threads: two takers can
        budget->used += (long)n * unit;                  //  overshoot the limit by one request between the check and here; the
        if (budget->used > budget->peak) budget->peak = budget->used;      // limit is an admission bound, not a hard allocator wall)
        return hipSuccess;
    }
    // Shared pages (the prefix cache, q3_prefix_cache.h): `shared[p]` = how many holders page p has, kept only while there is
    // more than one — a page without an entry has exactly one. share() adds a holder; give() takes one away and returns the page
    // to the free list when the last one goes. A shared page is counted ONCE in in_use and in the budget: by take(), until then.
    std::unordered_map<float*, int> shared;
    void share(float* p) {
        std::lock_guard<std::mutex> g(mu);
        auto it = shared.find(p);
        if (it == shared.end()) shared.emplace(p, 2); else it->second += 1;
    }
    bool is_shared(float* p) { std::lock_guard<std::mutex> g(mu); return shared.count(p) != 0; }
    bool is_shared_locked(float* p) const { return shared.count(p) != 0; }      // the caller holds mu (one lock for a scan over many pages)
    void give(std::vector<float*>& pages) {
        std::lock_guard<std::mutex> g(mu);
        int freed = 0;
        for (float* p : pages) {
            auto it = shared.find(p);
            if (it != shared.end()) { if (--it->second <= 1) shared.erase(it); continue; }      // another holder keeps it
            free_pages.push_back(p); ++freed;
        }
        in_use -= freed;
        { std::lock_guard<std::mutex> gb(budget->mu); budget->used -= (long)freed * unit; }
        pages.clear();
    }
    // slabs none of whose pages is held go back to the device (q3_model_kv_pool_trim); returns the bytes freed
    size_t trim() {
        std::lock_guard<std::mutex> g(mu);
        size_t freed = 0;
        for (size_t i = 0; i < slabs.size();) {
            char* lo = (char*)slabs[i]; char* hi = lo + (size_t)SLAB_SLOTS * run_floats * elem_bytes;      // the slab's layer-0 K runs name its pages
            int n_free = 0;
            for (float* p : free_pages) n_free += ((char*)p >= lo && (char*)p < hi) ? 1 : 0;
            if (n_free < SLAB_SLOTS) { ++i; continue; }
            free_pages.erase(std::remove_if(free_pages.begin(), free_pages.end(), [&](float* p) { return (char*)p >= lo && (char*)p < hi; }), free_pages.end());
            (void)hipFree(slabs[i]); slabs.erase(slabs.begin() + (long)i);
            total -= SLAB_SLOTS; freed += slab_bytes();
        }
        return freed;
    }
    // the first slab ahead of the first request (q3_model_finalize): its hipMalloc (~1 GB) is then not on a session's time to first audio
    hipError_t prewarm() {
        std::vector<float*> one;
        {
            std::lock_guard<std::mutex> g(mu);
            if (!slabs.empty()) return hipSuccess;
        }
        const hipError_t e = take(1, one);
        if (e == hipSuccess) give(one);
        return e;
    }
    ~KvPool() { for (void* s : slabs) (void)hipFree(s); }
};

struct PrefixCache;
struct q3_model {
    q3_config cfg{};
    int device = 0;
    int codec_planes = 3;  // q3_model_set_codec_planes: 3 = f32-exact bf16x3 products in the vocoder's convs, 2 = the two leading planes
    KvBudget kv_budget;    // one limit / occupancy for both pools below, in half-f32-page units
    KvPool kv_pool;
    KvPool kv_pool16;      // pages of bf16 sessions (q3_session_set_kv_dtype): the same geometry with 2-byte elements
    PrefixCache* prefix = nullptr;      // prefilled instruct pages shared across requests (q3_prefix_cache.h; created with a device model, off until sized)
    // sessions hold pages, streams and weights of their model: the handle itself is ONE reference and every live session another;
    // whoever drops the count to zero destroys the model (q3_model_free with sessions still alive only gives up the handle's
    // reference — a host that tears down in the wrong order must not crash — and nobody touches *m after its own decrement)
    std::atomic<int> refs{1};
    std::vector<Slot> slots;
    std::unordered_map<std::string, int> index;
    char* arena = nullptr; size_t arena_bytes = 0;
    bool finalized = false;
    // derived device buffers
    float *rope_cos = nullptr, *rope_sin = nullptr; int rope_len = 0;      // talker/CP (theta, hd 128)
    float* derived = nullptr;                                              // codebooks + snake tables
    // bf16x3-packed copies of the vocoder's conv / linear weights (launch_pack_conv_w), keyed by the f32 pointer
    std::unordered_map<const float*, const void*> wpk; void* wpk_arena = nullptr;
    const void* pk(const float* w) const { auto it = wpk.find(w); return it == wpk.end() ? nullptr : it->second; }
    // frame-loop streams of freed sessions, reused by the next q3_session_create: creating a priority stream costs 1.6 ms and
    // destroying one 1.1 ms — 8 % of a streaming session's time to first audio, more than its whole prefill
    std::mutex stream_mu; std::vector<hipStream_t> idle_streams;
    const float* first_cb = nullptr; const float** rest_cbs_dev = nullptr; // device array of 15 pointers
    const uint16_t** cp_embs_dev = nullptr;                                // device array of 15 pointers
    // 1.7B: small_to_mtp_projection applied once to every row of the 15 acoustic embedding tables and of the talker's
    // codec embedding (code_predictor.rs:337-345, 386-396 project the gathered row on every pass): f32 [rows][cp_hidden]
    float* proj_tabs = nullptr; const float* cp_proj[15] = {}; const float* sem_proj = nullptr;
    // layer-0 q|k|v of every such row (input RMSNorm + qkv projection of code-predictor layer 0): f32 [rows][qkv dim]
    float* qkv0_tabs = nullptr; const float* cp_qkv0[15] = {}; const float* sem_qkv0 = nullptr;
    // resolved pointers
    const uint16_t *text_emb, *codec_emb;
    TW fc1w, fc2w, codec_head, mtp_w;
    const float *fc1b, *fc2b, *norm, *mtp_b, *cp_norm;
    std::vector<LayerW> tl, cl;
    std::vector<const uint16_t*> cp_emb; std::vector<TW> cp_head;
    const float *first_proj, *rest_proj, *pre_w, *pre_b, *inp_w, *inp_b, *outp_w, *outp_b, *dec_norm;
    std::vector<DecLayerW> dl;
    UpW up[2]; const float *init_w, *init_b; DecBlockW blk[4];
    const float *fin_a, *fin_ib, *fin_w, *fin_b;
};

static inline int up16(int v) { return (v + 15) & ~15; }
static inline int up32(int v) { return (v + 31) & ~31; }
static inline int up4(int v) { return (v + 3) & ~3; }
static inline int up128(int v) { return (v + 127) & ~127; }
// Narrow projections (fewer than 4096 output rows) keep BOTH tilings resident — HBM capacity is not the
// constraint, launch latency is: the 4-row-tile kernel fills the chip for M <= 2 tokens (and for N <= 1024 up
// to M = 8), the 16-row-tile kernel is cheaper per token for larger batches.
static inline bool dual_tiled(int n_total) { return n_total < 4096; }
static inline int kpad_for(int mode, int K) { return mode == 2 ? up128(K) : up32(K); }
static inline size_t tiled_elems(int mode, int rows, int cols) {
    return mode == 2 ? (size_t)up4(rows) * up128(cols) : (size_t)up16(rows) * up32(cols);
}

// short K with many rows (code-predictor / 0.6B gate-up 3072 x 1024, lm_head 2048 x 1024): the 16-row kernel already has
// one whole-slice group per wave and >= 128 workgroups, and beats the 4-row tiles even at M = 1 (gate/up 5.3 vs 6.5 us)
static inline bool short_k_wide(int N, int K) { return K <= 1024 && N >= 2048; }
static inline int pick_mode(const TW& w, int M, int N, int K) {
    static const bool no4 = getenv("Q3_GEMV_NO_MFMA4") != nullptr;     // tuning aid: 16-row tiles wherever both images exist (M > 2)
    if (w.t2 && !w.t1) return 2;
    if (M > 16 && w.t1) return 1;             // wide batches: k_gemv_wide works on the 16-row tiles
    if (no4 && w.t1 && M > 2) return 1;
    if (w.t2 && !short_k_wide(N, K) && (M <= 2 || (N <= 1024 && M <= 8))) return 2;
    return 1;
}
static inline void set_w(LinArgs& a, const TW& w, int M, int N, int K) {
    a.tiled = pick_mode(w, M, N, K); a.W = a.tiled == 2 ? w.t2 : w.t1; a.Kpad = kpad_for(a.tiled, K);
}
static inline void set_w2(LinArgs& a, const TW& w, const TW& w2, int M, int N, int K) {
    set_w(a, w, M, N, K); a.W2 = a.tiled == 2 ? w2.t2 : w2.t1;
}
// session-lifetime device blocks from the per-device size-class cache (q3_codec_run.hip)
Q3_HIDDEN hipError_t dev_malloc(void** p, size_t bytes);
Q3_HIDDEN void dev_free(void* p);

struct DevPool {
    std::vector<void*> ptrs;
    // lazy: the zero-fills of a run of allocations are only ISSUED (null stream, in order with the synchronous hipMemcpy
    // uploads that may follow) and settle() waits for all of them once — a session is ~45 buffers, and a memset + a device
    // synchronisation each was 2-3 ms of every q3_session_create (the side session of a continuous-batching swap)
    bool lazy = false;
    hipError_t settle() { return q3_null_stream_sync(); }
    template <typename T> hipError_t alloc(T** p, size_t count) {
        void* q = nullptr;
        hipError_t e = dev_malloc(&q, (count ? count : 1) * sizeof(T));
        if (e != hipSuccess) return e;
        ptrs.push_back(q); *p = (T*)q;
        // zero-fill on the null stream and WAIT for it: the users launch on non-blocking streams, which the null stream
        // does not order against — a memset still in flight would wipe what their first kernels write (seen once the
        // blocks started coming from the cache instead of a slow hipMalloc)
        return q3_null_stream_memset(q, (count ? count : 1) * sizeof(T), !lazy);
    }
    void release_all() {
        if (lazy) (void)q3_null_stream_sync();      // a creation that failed midway: no zero-fill may outlive its block's ownership
        for (void* p : ptrs) dev_free(p);
        ptrs.clear(); lazy = false;
    }
    ~DevPool() { release_all(); }
};

// ------------------------------------------------------------------------------------------------
// codec decoder pipeline
// ------------------------------------------------------------------------------------------------
// Left context (frames) the convolutional stack needs for its output to be independent of where it was started:
// propagating the causal receptive field back from the PCM (final k7: 6 samples; per block 6*(1+3+9) = 78 samples
// of residual units + 1 input sample of the 2-tap polyphase transposed conv; decoder.0 k7; two ConvNeXt dwconv7
// + 1-tap transposed convs) gives 29 @640/frame -> 28 @160 -> 23 @32 -> 14 @4 -> 20 -> 26 @4 -> 13 @2 -> 19 -> 10 frames.
constexpr int CODEC_CTX_FRAMES = 12;

struct CodecWS {
    int cap_frames = 0;        // frames the convolutional stack can take in one call
    int cap_front = 0;         // frames the quantiser / pre-transformer front can take (>= cap_frames)
    float *bufA = nullptr, *bufB = nullptr, *bufC = nullptr, *bufF = nullptr, *bufD = nullptr, *bufE = nullptr;
    float *cs = nullptr, *sn = nullptr;
    uint32_t* frames = nullptr; float* pcm = nullptr;
    void release() {
        dev_free(bufA); dev_free(bufB); dev_free(bufC); dev_free(bufF); dev_free(bufD); dev_free(bufE); dev_free(cs); dev_free(sn); dev_free(frames); dev_free(pcm);
        bufA = bufB = bufC = bufF = bufD = bufE = cs = sn = pcm = nullptr; frames = nullptr; cap_frames = 0; cap_front = 0;
    }
};

// ------------------------------------------------------------------------------------------------
// session
// ------------------------------------------------------------------------------------------------
struct LmBuf { float *X, *SUM, *QKV, *Q, *ATT, *ACT, *PART; };
struct LmDims { int H, I, nh, nkv, layers; float eps; };

// a request with its arrays owned (queued tickets of the batcher; the rows of a ragged first batch until they are prefilled)
struct BatReq {
    q3_request r{}; std::vector<uint32_t> text, instruct, ref_codes, ref_text; std::vector<float> xvec;
    void own(const q3_request& q, int hidden) {
        r = q;
        text.assign(q.text_ids, q.text_ids + (q.text_ids ? q.n_text : 0));
        instruct.assign(q.instruct_ids, q.instruct_ids + (q.instruct_ids ? q.n_instruct : 0));
        ref_codes.assign(q.ref_codes, q.ref_codes + (q.ref_codes ? (size_t)q.n_ref * 16 : 0));
        ref_text.assign(q.ref_text_ids, q.ref_text_ids + (q.ref_text_ids ? q.n_ref_text : 0));
        if (q.xvector) xvec.assign(q.xvector, q.xvector + hidden);
        fix();
    }
    void fix() {      // pointers into this object's own storage (after a move of the object)
        r.text_ids = text.empty() ? nullptr : text.data(); r.n_text = (int32_t)text.size();
        r.instruct_ids = instruct.empty() ? nullptr : instruct.data(); r.n_instruct = (int32_t)instruct.size();
        r.ref_codes = ref_codes.empty() ? nullptr : ref_codes.data(); r.n_ref = (int32_t)(ref_codes.size() / 16);
        r.ref_text_ids = ref_text.empty() ? nullptr : ref_text.data(); r.n_ref_text = (int32_t)ref_text.size();
        r.xvector = xvec.empty() ? nullptr : xvec.data();
    }
};
struct SeqInfo {
    q3_request req; std::vector<uint32_t> text, instruct, ref_codes, ref_text; std::vector<float> xvec; bool icl = false;
    int prefill_len = 0, trailing_len = 0, row_base = 0, n_rows = 0, trail_base = 0, pad_row = 0;
    int n_frames = 0; bool done = false;
    // rows end at different frames: a row generates at most `limit` frames (its own max_length) counted from session frame
    // `start_run` (0, or the session's frame count when the row was swapped in: q3_session_replace)
    int start_run = 0, limit = 0, stream_pos = 0;
    int reused = 0;         // prompt positions whose K/V pages came from the model's prefix cache (q3_session_prefix_info)
    bool idle = false;      // frozen by session_idle_row: holds one page (the one its frozen position lies in), takes no more
    int max_length_req = 0; // the request's own max_length (an ICL row's length cap is applied to it: `limit`)
    // open text (q3_session_open_text): the row's text arrives in pieces (q3_session_append_text). Its trailing
    // rows live in the row's replacement slot (trail_base), n_trail of them so far; `ready` = frames the text allows (INT_MAX
    // once closed) = text_ready[b] on the device; `committed` = frames the row has committed (the device frame_idx, predicted
    // by the host between two reads). An opened row's frames are counted from `committed`, never from frames_run - start_run.
    bool opened = false, text_closed = true;
    std::vector<uint32_t> text_all;       // every text token received so far (the request's own first)
    int n_trail = 0, ready = 0x7fffffff, committed = 0;
    // the row's request pointing at the row's own vectors (as BatReq::fix; an ICL row stays one with an empty transcript: the
    // predicate reads the pointer)
    q3_request request() const {
        static const uint32_t none[1] = {0};
        q3_request r = req;
        r.text_ids = text.data(); r.n_text = (int32_t)text.size();
        r.instruct_ids = instruct.empty() ? nullptr : instruct.data(); r.n_instruct = (int32_t)instruct.size();
        r.ref_codes = ref_codes.empty() ? nullptr : ref_codes.data(); r.n_ref = (int32_t)(ref_codes.size() / 16);
        r.ref_text_ids = !ref_text.empty() ? ref_text.data() : icl ? none : nullptr; r.n_ref_text = (int32_t)ref_text.size();
        r.xvector = xvec.empty() ? nullptr : xvec.data();
        return r;
    }
};

struct ProfAcc { double ms = 0; double bytes = 0; long launches = 0; };
// Park / resume (q3_row_state.hip): the device blocks of a session's records. A block a resumed or freed record no longer needs
// stays on the session's shelf for the next park — the park path then allocates nothing —; once the session is gone (a record
// may outlive it) blocks go back to the device-memory cache instead. Blocks are powers of two from 64 KB on.
struct ParkShelf { std::mutex mu; bool alive = true; std::vector<std::pair<void*, size_t>> blocks; };
enum { PARK_MAX_SEGS = 24, PARK_PAYLOAD_INTS = 8 };      // one k_row_move launch of a park / resume: descriptors + host-made values
constexpr size_t PARK_DESC_BYTES = (size_t)PARK_MAX_SEGS * 32 + (size_t)PARK_PAYLOAD_INTS * 16;
struct ProfShape { int M, N, K, epi, rms, produce, tiled, count; };

// What one row of an output stage has been asked for (Settings): the one value a stage row, a session row and a
// batcher ticket hold. The defaults are a row with every step off. It changes through the checked edits (out_set_*, further down)
// alone and reaches a stage row through pcm_stage_apply. (pause_ms: the silence step's range starts at 20, on or off.)
struct OutSettings {
    uint32_t rate = 24000; int fmt = Q3_PCM_F32;              // the resampler and the format
    int tempo = 1000, cents = 0;                              // permille, 1000: off; cents, 0: off
    int gain_mB = 0, ceil_mB = 0;                             // the level; 0 / 0: off
    int loud = Q3_LOUD_OFF, target_mB = -1900, prior_mB = 0;
    int sil_mB = 0, edge_ms = 0, pause_ms = 20;               // the silence step's threshold, 0: off
    uint64_t mark_key = 0; int mark_mB = Q3_MARK_STRENGTH_DEFAULT;               // the mark step's key, 0: off; its strength
    // 24 kHz f32 with every step off: the samples leave as they are, and no stage is needed
    bool plain() const {
        return rate == 24000 && fmt == Q3_PCM_F32 && tempo == 1000 && cents == 0 && gain_mB == 0 && ceil_mB == 0 && loud == Q3_LOUD_OFF && sil_mB == 0 &&
               mark_key == 0;
    }
    size_t sample_bytes() const { return fmt == Q3_PCM_F32 ? 4 : fmt == Q3_PCM_S16 ? 2 : 1; }
};

struct q3_session {
    q3_model* m = nullptr; int B = 0;
    hipStream_t stream = nullptr; bool owns_stream = true;     // the side session of a swap borrows its host's stream
    DevPool pool;
    std::vector<SeqInfo> seq;
    q3_options opts{};
    int max_frames = 0, max_seq = 0, prefill_len = 0, n_splits = 1;
    int* limit = nullptr;                 // [B] per-row frame limits on the device (SampleArgs::limit)
    SampleRow* sample_rows = nullptr;     // [B] per-row sampling options on the device (SampleArgs::rows)
    int row_cap = 0, repl_base = 0;       // text-row slots of replacement rows: slot b = rows repl_base + b*row_cap .. (q3_session_replace)
    LmBuf tb{}, cb{};
    float *LASTH = nullptr, *LOGITS = nullptr, *CP_IN = nullptr, *CP_LOGITS = nullptr;
    float* wide_ws = nullptr; size_t wide_ws_bytes = 0;       // slice sums of the wide-session GEMM (B > 16; q3_kernels_wide.hip)
    float *kcache = nullptr, *vcache = nullptr, *ckcache = nullptr, *cvcache = nullptr;
    size_t kv_layer_stride = 0, ckv_layer_stride = 0;
    // paged talker KV (the default; Q3_KV_CONTIGUOUS=1 keeps one extent per row: A/B aid): kv_table[b][KV_MAX_PAGES] page
    // pointers on the device (what the attention kernels read), kv_rows[b] = the pages row b holds, in position order
    bool paged = false; unsigned long long* kv_table = nullptr; std::vector<std::vector<float*>> kv_rows;
    // ragged first batch (q3_session_create with rows of different prefill lengths / prompt kinds): the session was opened on
    // idle rows, these are the real requests; q3_session_prefill prefills them in groups of equal prefill length and moves each
    // row in (transplant_row), exactly as a continuous-batching swap would
    std::vector<BatReq> ragged;
    int prefill_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // q3_session_prefill_info: what the ragged prefill ran (packed passes)
    bool regrouped = false;              // prefix cache: a one-length session whose rows were prefilled in groups (prefix_regroup); transplant_row then also fills embeds
    bool prefix_common = false;           // prefix cache: rows that hit differently stay in this session (a group prefill_ragged formed)
    int kv_overflow_row = -1;             // the row whose page request the pool refused (kv_reserve_row): the batcher fails that row alone
    // bf16 K/V (opt-in, q3_session_set_kv_dtype; the reference GPU path's cache dtype): the prompt is prefilled into f32 pages
    // as always, converted once into pages of the bf16 pool (kv_in_bf16 from then on), and the decode attention reads / appends bf16
    bool kv_bf16 = false, kv_in_bf16 = false; unsigned long long* kv_conv = nullptr;      // kv_conv: [2][B * KV_MAX_PAGES] page lists of the conversion launch
    float *rows = nullptr, *embeds = nullptr, *xvec = nullptr; int n_rows_total = 0;
    // prefill scratch, session-lifetime (no hipMalloc / hipFree and no extra stream syncs on the time-to-first-audio path)
    uint32_t* ids_dev = nullptr; int *tr_dev = nullptr, *ci_dev = nullptr; float *proj_e = nullptr, *proj_h = nullptr;
    uint32_t* ref_codes_dev = nullptr;
    int *trail_base = nullptr, *trail_len = nullptr, *pad_row = nullptr;
    // open text rows: text_ready[b] (SampleArgs::text_ready; nullptr until a row is opened — the frame's kernels then
    // take their closed-text paths) and the scratch of the one projection path appended tokens take (8-row GEMV groups)
    int* text_ready = nullptr;
    uint32_t* app_ids = nullptr; float *app_e = nullptr, *app_h = nullptr, *app_out = nullptr;
    int* flush_buf = nullptr; size_t flush_cap = 0;       // the batcher's text flush (session_append_many): [ids | destination rows | entries to publish]
    uint32_t* tok = nullptr; uint8_t* seen = nullptr; int *frame_idx = nullptr, *pos = nullptr, *token_count = nullptr;
    float* U = nullptr; uint32_t* codes = nullptr;
    float* logits_hist = nullptr; float* cp_logits_hist = nullptr; bool debug = false;
    bool prefilled = false; int frames_run = 0;
    // park / resume (q3_row_state.hip): what a record names its session by (never reused, unlike the address), and the device table
    // of one k_row_move launch — descriptors and a few host-made values, one upload (allocated with a paged session) —, and the
    // shelf its records' device blocks come from and go back to
    uint64_t uid = 0; char* park_desc = nullptr; std::shared_ptr<ParkShelf> shelf;
    hipGraphExec_t graph_exec = nullptr; hipGraph_t graph = nullptr;
    // the captured frame as a packet program on the library's own AQL queue (q3_aql.cpp); nullptr: frames replay through
    // hipGraphLaunch.  aql_mode: 0 = off, 1 = HIP's header policy (agent-scope fences on every packet), 2 = no fences
    q3::AqlProgram* aql = nullptr; int aql_mode = 0; bool aql_tried = false, aql_failed = false;
    bool precapture = false;       // q3_session_prefill captures the frame while the prompt's kernels run (set by the callers that will replay it)
    CodecWS cws;
    q3_codec_stream* cstream = nullptr;   // q3_session_next_chunks, stream mode 1: per-row vocoder state (created on the first call)
    // q3_session_next_chunks_out: its stage, one row per session row (created on the first such call: out_started, after which
    // q3_session_set_output is refused), and what each row has been asked for (q3_session_set_*): a row's entry stays with it across
    // q3_session_replace, and reaches the stage's row when the stage is created or, once it exists, with the setter
    q3_pcm_stage* ostage = nullptr; bool out_started = false;
    std::vector<OutSettings> out;
    // overlapped segment decode (q3_session_run): vocoder segments run on their own stream while the frame loop continues
    hipStream_t dec_stream = nullptr; hipEvent_t dec_ev = nullptr;
    std::vector<CodecWS> par_ws; std::vector<hipStream_t> par_streams;     // q3_session_run: utterances vocoded side by side
    CodecWS seg_ws;                                          // q3_session_run: segments vocoded beside the frame loop
    std::vector<uint32_t> codes_host; bool codes_host_valid = false;
    int stream_mode = 0;  // 0 = context-free chunk decode (reference behaviour), 1 = continuous (left context re-run: seamless)
    bool profile = false; ProfAcc prof_linear;
    bool legacy_attn = getenv("Q3_LEGACY_ATTN") != nullptr;   // A/B aid: three-kernel attention path
    bool proj_tables = getenv("Q3_NO_PROJ_TABLES") == nullptr;   // A/B aid: set to project the gathered embedding on every pass
    bool qkv_tables = getenv("Q3_NO_QKV_TABLES") == nullptr;     // A/B aid: set to run the layer-0 qkv GEMV on every pass
    bool ksplit = getenv("Q3_NO_KSPLIT") == nullptr;          // A/B aid: set to keep o-proj / down-proj on the unsplit kernels
    bool cp_attn = getenv("Q3_NO_CP_ATTN") == nullptr;        // A/B aid: set to run the code predictor on the generic k_attn_fused
    bool no_chunk = getenv("Q3_NO_CHUNK") != nullptr;         // A/B aid: one position per prefill step, 16-pass code predictor
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events; std::vector<double> prof_event_bytes;
    std::vector<hipEvent_t> prof_pool; size_t prof_pool_next = 0;
    std::vector<ProfShape> prof_shapes;
#ifdef Q3_TRACE
    // development builds only (q3_kernels.h, Q3_TRACE): per-node stamp slices of the captured frame graph
    unsigned long long* trace_buf = nullptr; int trace_node = 0, trace_cap = 0;
    struct TraceMeta { int kind, a, b, c, d, e, f; };       // kind 0 linear (M, N, K, epi, rms, tiled) / 1 attn_cp / 2 attn_fused / 3 attn_merge (B, nh, splits, pos)
    std::vector<TraceMeta> trace_meta;
    unsigned long long* trace_next(int kind, int a, int b, int c, int d = 0, int e = 0, int f = 0) {
        if (!trace_buf || trace_node >= trace_cap) return nullptr;
        trace_meta.push_back({kind, a, b, c, d, e, f});
        return trace_buf + (size_t)(trace_node++) * TRACE_NODE;
    }
#endif
    ~q3_session();
};


// ------------------------------------------------------------------------------------------------
// functions one unit defines and another calls
// ------------------------------------------------------------------------------------------------
// q3_model.hip
Q3_HIDDEN void model_destroy(q3_model* m);
Q3_HIDDEN void retile_bf16(const uint16_t* src, int N, int K, uint16_t* dst, int mode);
// q3_codec_run.hip
Q3_HIDDEN q3_status codec_reserve(const q3_model* m, CodecWS& ws, int T, int Tf = 0);
Q3_HIDDEN int samples_per_frame(const q3_config& c);
// resident: residency cap of this decode's matrix-core launches (ConvArgs::resident): 0 = none; n >= 1 = at most n workgroups of a
// launch per CU — for a decode that runs beside the frame loop (q3_session_run) and must leave every CU room for a frame workgroup
Q3_HIDDEN q3_status codec_decode_dev(const q3_model* m, CodecWS& ws, int T, hipStream_t st, float** taps, int c0 = 0, int resident = 0);
// The range decode every vocoding entry goes through: frames [a, e) of one row, the convolutional stack started at frame c0
// (0, or vocode_ctx_start(a) = max(0, a - CODEC_CTX_FRAMES): the one statement of the rule). Enqueued on st, waits for nothing.
struct VocodeSrc { const uint32_t* prefix_host; int n_prefix;      // frames in front of the row's own (ICL reference frames), or none
                   const uint32_t* codes; bool codes_on_host; };   // the row's frames [0, e), from its first
struct VocodePcm { const float* dev; size_t n; };                  // in the workspace; valid once st has drained
Q3_HIDDEN int vocode_ctx_start(int a);
Q3_HIDDEN q3_status vocode_enqueue(const q3_model* m, CodecWS& ws, hipStream_t st, const VocodeSrc& src, int a, int e, int c0, int resident, VocodePcm* out);
// n: the count; host: the samples, "pcm buffer too small" below pcm.n. st null: a synchronous copy (after the caller's wait)
Q3_HIDDEN q3_status vocode_copy_out(const VocodePcm& pcm, float* host, size_t cap, size_t* n, hipStream_t st);
// the stages of codec_decode_dev, for the codec stream (q3_codec_stream.hip). A CodecScope must be alive on the calling thread
// while they run: it names the model (packed weights), the bf16 planes (q3_model_set_codec_planes) and the residency cap of their launches.
struct Q3_HIDDEN CodecScope { int planes, resident; explicit CodecScope(const q3_model* m, int resident = 0); ~CodecScope(); CodecScope(const CodecScope&) = delete; };
using CodecAttnFn = std::function<q3_status(int layer, float* q, float* k, float* v, float* ao)>;
Q3_HIDDEN q3_status codec_rope_table(const q3_config& c, int n, float* cs_dev, float* sn_dev);
Q3_HIDDEN q3_status codec_front_quant(const q3_model* m, CodecWS& ws, int T, hipStream_t st);
Q3_HIDDEN q3_status codec_front_preconv(const q3_model* m, const float* x, float* y, int L, hipStream_t st);
Q3_HIDDEN q3_status codec_front_transformer(const q3_model* m, CodecWS& ws, int T, hipStream_t st, const CodecAttnFn& rope_attn);
Q3_HIDDEN q3_status codec_stack_dev(const q3_model* m, CodecWS& ws, float* cur, int L, hipStream_t st, float** taps, const CodecScope& scope);
// q3_codec_stream.hip
// n new frames of one row, codes on the host OR the device; the first `skip` of them only catch the row's state up (no samples)
// With an output stage (q3_pcm_stage.hip): the samples of the n - skip delivered frames go through row ps_row of `ps` on the
// stream's stream before they are copied to the host — out_host receives *n_out samples in that row's rate and format, the tail
// included when `last` is set — and pcm_host is not used. Every row of a push names the same stage. Without one: today's path.
struct CsPush {
    int row; int n; int skip; const uint32_t* host; const uint32_t* dev; float* pcm_host;
    q3_pcm_stage* ps = nullptr; int ps_row = -1; int last = 0; void* out_host = nullptr; size_t* n_out = nullptr;
};
// block_frames > 0: block-allocated state (a multiple of 32), at most max_blocks blocks (0 = no limit)
Q3_HIDDEN q3_status codec_stream_create(q3_model* m, int rows, int max_frames, hipStream_t st, q3_codec_stream** out, int block_frames = 0,
                                        int max_blocks = 0);
Q3_HIDDEN q3_status codec_stream_push(q3_codec_stream* cs, const std::vector<CsPush>& pushes);
Q3_HIDDEN int codec_stream_pos(const q3_codec_stream* cs, int row);
Q3_HIDDEN void codec_stream_blocks(const q3_codec_stream* cs, int row, int upto, int* held, int* need);
Q3_HIDDEN void codec_stream_reset(q3_codec_stream* cs, int row);
// q3_pcm_stage.hip
// n samples of 24 kHz f32 on the device for stage row `row`; last: the row's input ends here (its tail is flushed)
struct PsSeg { int row; const float* dev; size_t n; int last; };
// one row of a pass of k_pcm_stage (device-visible, 8-byte aligned)
struct PsDesc {
    const float* src; const float* tail_in; float* tail_out; const float* taps; void* out;
    long long base, i0;                     // input samples the row had consumed, first output index of this pass
    int n_new, n_out, L, M, fmt, pad;
};
// The public part of a push's plan: the resampler's descriptors of the rows that run, and per segment the byte offset into the
// stage's staging buffer and the samples it returns. late: a row has a silence step, so the plan is made by pcm_stage_run, behind
// that step's pre-pass. What the other steps of the chain need for the push is the stage's own business.
struct PsPlan { std::vector<PsDesc> desc; std::vector<size_t> off, count; size_t bytes = 0; bool late = false; };
// q3_resample's filter as a table for output / input = L / M in lowest terms, out[L][128] (taps_of): the output stage's at
// L / M = sr_out / 24000, the intake's (q3_intake.hip) at L / M = 24000 / sr_in
Q3_HIDDEN void resampler_taps(int L, int M, std::vector<float>& out);
// the counter hash of q3_synth_fill (q3_model.hip) and its hash of a name: the mark's carrier derives its phases from them
Q3_HIDDEN uint64_t synth_hash(uint64_t x);
Q3_HIDDEN uint64_t synth_name_hash(const char* s);
// the mark's carrier of a key as q3_mark_carrier builds it, c[4096] (q3_pcm_stage.hip); the intake's detector stages it
Q3_HIDDEN void mark_carrier(uint64_t key, float* c);
// the detector's score and offset from the 4096 correlations (f64 on the host, whoever computed rho)
Q3_HIDDEN q3_status mark_score_f32(const float* rho, double* score, int* offset);
Q3_HIDDEN int pcm_stage_rows(const q3_pcm_stage* ps);
Q3_HIDDEN void pcm_stage_reset(q3_pcm_stage* ps, int row);
Q3_HIDDEN q3_status pcm_stage_check_rows(const q3_pcm_stage* ps, const char* who, int n_rows, const int* rows);
Q3_HIDDEN size_t pcm_stage_count(const q3_pcm_stage* ps, int row, size_t n, int last);
// The checked edits, one per public setter of every layer: the only way an OutSettings changes. Each validates the new values
// against the rest of the setting (a tempo and a pitch have to admit each other) and writes them on success alone; a refusal
// starts with `who`.
Q3_HIDDEN q3_status out_set_output(const char* who, OutSettings& o, uint32_t sample_rate, int format);
Q3_HIDDEN q3_status out_set_tempo(const char* who, OutSettings& o, int tempo_permille);
Q3_HIDDEN q3_status out_set_pitch(const char* who, OutSettings& o, int cents);
Q3_HIDDEN q3_status out_set_level(const char* who, OutSettings& o, int gain_mB, int ceiling_mB);
Q3_HIDDEN q3_status out_set_loudness(const char* who, OutSettings& o, int mode, int target_mB, int prior_mB);
Q3_HIDDEN q3_status out_set_silence(const char* who, OutSettings& o, int threshold_mB, int edge_ms, int pause_ms);
Q3_HIDDEN q3_status out_set_mark(const char* who, OutSettings& o, uint64_t key, int strength_mB);
// The only writer of a row's step settings: what the steps that `o` turns on need on the device, the values derived from `o`,
// and the row's restart. All or nothing (but see the silence step's state there). pcm_stage_settings: what the row was given last.
Q3_HIDDEN q3_status pcm_stage_apply(q3_pcm_stage* ps, int row, const char* who, const OutSettings& o);
Q3_HIDDEN const OutSettings& pcm_stage_settings(const q3_pcm_stage* ps, int row);
// What a row that has taken no sample reads: its loudness step stands at the prior gain with no block, its silence step at five zeros
Q3_HIDDEN void out_loudness_at_rest(const OutSettings& o, float* mean_square, float* gain, int* blocks, int* gated);
Q3_HIDDEN void out_silence_at_rest(int64_t* n_in, int64_t* n_out, int64_t* lead_cut, int64_t* pause_cut, int64_t* trail_cut);
// A push of segments that are on the device, in three calls (one push per stage at a time; the rows move on in the last one alone):
// begin   checks the segments and, unless a row has a silence step (plan.late), makes the plan: a caller with a descriptor block of
//         its own can then carry plan.desc in it
// run     on `st`, which has the samples: where the plan is late, the silence step's pre-pass (a wait for `st`: its kept counts come
//         back), the plan, and plan.desc into the stage's own staging; then every step's launch, and the copy of the converted bytes
//         to the stage's pinned buffer. desc_dev: where the caller has put plan.desc on the device (null: the stage uploads it)
// finish  after the caller's wait for `st`: segment i's plan.count[i] samples to out_host[i] (may be null), the counts to n_samples
//         (may be null), and the commit
Q3_HIDDEN q3_status pcm_stage_begin(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, PsPlan& plan);
Q3_HIDDEN q3_status pcm_stage_run(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, PsPlan& plan, const PsDesc* desc_dev, hipStream_t st);
Q3_HIDDEN void pcm_stage_finish(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, const PsPlan& plan, void* const* out_host, size_t* n_samples);
// the three in a row, with the wait (st null: the stage's own stream)
Q3_HIDDEN q3_status pcm_stage_push_dev(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, hipStream_t st, void* const* out_host, size_t* n_samples);
// q3_session.hip
Q3_HIDDEN hipError_t sync_frames(q3_session* s);
Q3_HIDDEN q3_status kv_reserve_row(q3_session* s, int b, int n_pos);
Q3_HIDDEN q3_status kv_reserve_frames(q3_session* s, int frames);
Q3_HIDDEN void kv_release_row(q3_session* s, int b);
Q3_HIDDEN LmDims talker_dims(const q3_config& c);
Q3_HIDDEN LmDims cp_dims(const q3_config& c);
Q3_HIDDEN q3_status talker_step(q3_session* s, const int* pos_dev, int pos_static, bool with_head, int rows_per_seq = 1,
                                const int* text_ready = nullptr);
Q3_HIDDEN SampleRow sample_row(const q3_options& o);
// Prompt layout (DESIGN "Prompt layout"): everything a request's prompt kind and lengths decide, in one record (q3_prompt_shape_rec,
// include/q3tts.h) made by one pure function. n_text: the text counted — the request's own, or what an open row has received so far
// (prefill_len, n_rows and the row indices of a session row are those of its text at creation). The lengths must not be negative.
using PromptShape = q3_prompt_shape_rec;
Q3_HIDDEN int icl_frame_cap(int n_text);
Q3_HIDDEN PromptShape prompt_shape(const q3_request& r, int n_text);
static inline PromptShape prompt_shape(const q3_request& r) { return prompt_shape(r, r.n_text); }
// per prefill position of a row whose text rows start at row_base: the text row and the codec embedding (-1: none, -2: the x-vector, -3 - i: reference frame i)
Q3_HIDDEN void prompt_positions(const PromptShape& sh, const q3_request& r, int row_base, int* text_row, int* codec_id);
Q3_HIDDEN long row_worst_units(int prefill_len, int limit, bool bf16);
Q3_HIDDEN q3_request idle_request(int chunk_frames);
Q3_HIDDEN q3_status session_create(q3_model* m, const q3_request* reqs, int batch, int frame_budget, int prompt_budget, q3_session** out,
                                   hipStream_t borrow = nullptr);
Q3_HIDDEN q3_status lm_layer(q3_session* s, const LmDims& d, const LayerW& w, LmBuf& b, float* kc, float* vc, int max_seq,
                             const int* pos_dev, int pos_static, int n_splits, int rows_per_seq = 1, bool skip_qkv = false,
                             const CpGatherArgs* fold = nullptr, int paged_layer = -1);
// open text through the batcher: switch the hold path on; one flush over many rows; a row's progress
struct TextPiece { int b; const uint32_t* ids; int n; bool last; };      // n tokens for open row b; last: its text closes
Q3_HIDDEN q3_status session_text_enable(q3_session* s);
Q3_HIDDEN q3_status session_append_many(q3_session* s, const std::vector<TextPiece>& pieces);
Q3_HIDDEN int session_row_remaining(const q3_session* s, int b);
Q3_HIDDEN int session_row_committed(const q3_session* s, int b);
Q3_HIDDEN q3_status session_refresh_codes(q3_session* s);      // the host copy of the codes, every row's n_frames / done
// q3_row_state.hip
// one run of bytes of a k_row_move launch (device-visible, 32 bytes): copied src -> dst, or exchanged
enum { ROW_MOVE_COPY = 0, ROW_MOVE_EXCHANGE = 1 };
struct RowSeg { void* src; void* dst; unsigned long long bytes; int mode; int pad; };
Q3_HIDDEN hipError_t launch_row_move(const RowSeg* segs_dev, int n_segs, size_t max_bytes, hipStream_t st);
Q3_HIDDEN int parked_frames(const q3_parked* p, const uint32_t** codes);      // frames (cut at an EOS) and the host copy of the codes
Q3_HIDDEN int parked_committed(const q3_parked* p);
Q3_HIDDEN int parked_pages(const q3_parked* p);
Q3_HIDDEN bool parked_done(const q3_parked* p);
Q3_HIDDEN const SeqInfo& parked_seq(const q3_parked* p);
// q3_prefix_cache.hip: see q3_prefix_cache.h
// q3_batcher.hip
Q3_HIDDEN q3_status transplant_row(q3_session* s, int b, q3_session* side, int j, int limit);
// n requests prefilled in a side session so that their rows can enter `host` (transplant_row): the side session and, per row, the
// limit resolved from limit_req[j] (which the caller has checked against the host's frame budget). open_text: one request, taken
// with its text open (closed: and closed again before the prefill); prefix_common: the rows link what their shortest cached chain
// allows; borrow: the stream to prefill on (null: one of its own); created: called once the side session stands, before the
// checks and the prefill. Of `host` it reads what never changes under a running frame (the stage worker calls it on its thread).
// staged_only: the side session is left checked but NOT prefilled — a packed pass runs its layers with other rows' (prefill_ragged).
Q3_HIDDEN q3_status side_prefill(q3_session* host, const q3_request* reqs, const int* limit_req, int n, bool open_text, bool closed,
                                 bool prefix_common, hipStream_t borrow, std::unique_ptr<q3_session>* side_out, int* limit_out,
                                 const std::function<void()>& created = nullptr, bool staged_only = false);
