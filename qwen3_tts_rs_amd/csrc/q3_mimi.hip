// q3_mimi.hip — the speech-tokenizer ENCODER on gfx950: 24 kHz reference audio -> 12.5 Hz frames of 16 codebook indices,
// the `ref_codes` of an ICL voice-clone prompt (reference: Encoder12Hz, src/models/codec/encoder_12hz.rs:34-144, called by
// create_voice_clone_prompt, src/lib.rs:1172-1178). The reference builds it from candle-transformers' Mimi modules over the
// HF-format `encoder.*` keys of speech_tokenizer/model.safetensors; the algorithm is the published Mimi encoder (Hugging
// Face transformers models/mimi/modeling_mimi.py): SEANet conv encoder -> 8-layer transformer -> stride-2 conv -> split
// residual vector quantiser (nearest neighbour per layer). oracle/q3_oracle_mimi.c restates it for the parity tests.
//
// Once-per-utterance work (~16 GFLOP for 5 s of audio), so it rides the vocoder's kernels instead of growing its own GEMMs:
//   * stride-1 causal convs  -> launch_conv1d (bf16x3 matrix-core implicit GEMM where the channel counts allow);
//   * strided convs (kernel 2r, stride r) -> the input is FOLDED r samples into channels (k_mimi_fold, with the ELU that
//     precedes every such conv applied on the way), which turns the conv into a 2-tap stride-1 causal conv with cin*r
//     input channels — the weights are re-laid once at upload: w'[co][ci*r + p][j] = w[co][ci][j*r + p];
//   * transformer layers on the [C][T] layout as 1x1 convs + channel LayerNorm + rotate-half RoPE, attention with the
//     250-frame causal window in k_mimi_attn;
//   * k_mimi_rvq: one workgroup per frame walks the quantiser layers (distance to 2048 entries, first minimum, subtract).
// Many clips per call (q3_mimi_encode_refs): the same launches once over all clips laid side by side, each in a slot with a guard
// frame, the elementwise kernels as clip-aware instances (k_mimi_*_p) — bit-equal per clip to the clip alone.
#include "../../include/q3tts.h"
#include "q3_kernels.h"
#include "q3_capture_lock.h"
#include "q3_internal.h"

#include <math.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

namespace q3 {

// y = ELU(x) (alpha 1)
__global__ __launch_bounds__(256) void k_mimi_elu(const float* __restrict__ x, float* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const float v = x[i]; y[i] = v > 0.0f ? v : expf(v) - 1.0f; }
}
hipError_t launch_mimi_elu(const float* x, float* y, size_t n, hipStream_t st) {
    if (n < 1 || (n + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mimi_elu, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, n);
    return hipGetLastError();
}
// fold r consecutive samples into channels: y[(c*r + p)][lead + tau] = f(x[c][tau*r + p]) (0 beyond L), f = ELU or identity.
// lead = 1 (replicate mode): column 0 holds x[c][0] for every phase — the replicate left padding of the downsample conv —
// and samples beyond L repeat x[c][L-1].
__global__ __launch_bounds__(256) void k_mimi_fold(const float* __restrict__ x, float* __restrict__ y, int L, int r, int Lf, int elu, int replicate) {
    const int col = blockIdx.x * 256 + threadIdx.x, cp = blockIdx.y;     // cp = c*r + p
    const int lead = replicate ? 1 : 0, W = Lf + lead;
    if (col >= W) return;
    const int c = cp / r, p = cp % r;
    const float* xr = x + (size_t)c * L;
    float v;
    if (replicate && col == 0) v = xr[0];
    else {
        const int i = (col - lead) * r + p;
        v = i < L ? xr[i] : (replicate ? xr[L - 1] : 0.0f);
    }
    if (elu) v = v > 0.0f ? v : expf(v) - 1.0f;
    y[(size_t)cp * W + col] = v;
}
hipError_t launch_mimi_fold(const float* x, float* y, int C, int L, int r, int Lf, int elu, int replicate, hipStream_t st) {
    if (C < 1 || r < 1 || L < 1 || Lf < 1 || (long long)C * r > 65535) return hipErrorInvalidValue;
    // plain mode: the last column starts inside the signal (i = (Lf - 1) * r + p as an int); replicate mode clamps
    if (!replicate && (long long)(Lf - 1) * r >= L) return hipErrorInvalidValue;
    if ((long long)Lf * r > 0x7fffffffLL) return hipErrorInvalidValue;
    const int W = Lf + (replicate ? 1 : 0);
    hipLaunchKernelGGL(k_mimi_fold, dim3((W + 255) / 256, C * r), dim3(256), 0, st, x, y, L, r, Lf, elu, replicate);
    return hipGetLastError();
}
// causal sliding-window MHA on [nh*64][T] tensors: one 64-lane wave per (query t, head h), keys j in (t - window, t]
// (query column t of head h against the keys j0 .. t, 64 per step from j0 on: the body of k_mimi_attn and of its packed instance)
__device__ __forceinline__ void mimi_attn_col(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                              float* __restrict__ o, int T, int t, int j0, int h, float scale) {
    const int lane = threadIdx.x;
    const size_t hb = (size_t)h * 64 * T;
    const float qd = q[hb + (size_t)lane * T + t];
    float m = -INFINITY, l = 0.0f, acc = 0.0f;
    for (int jb = j0; jb <= t; jb += 64) {
        const int j = jb + lane; const bool ok = j <= t;
        float s = 0.0f;
        for (int d = 0; d < 64; ++d) s = fmaf(__shfl(qd, d), ok ? k[hb + (size_t)d * T + j] : 0.0f, s);
        s = ok ? s * scale : -INFINITY;
        float cm = s;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cm = fmaxf(cm, __shfl_xor(cm, off));
        const float mn = fmaxf(m, cm), corr = expf(m - mn), p = ok ? expf(s - mn) : 0.0f;
        float ps = p;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) ps += __shfl_xor(ps, off);
        l = l * corr + ps; acc *= corr;
        for (int d = 0; d < 64; ++d) {
            float c = ok ? p * v[hb + (size_t)d * T + j] : 0.0f;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
            if (lane == d) acc += c;
        }
        m = mn;
    }
    o[hb + (size_t)lane * T + t] = acc / l;
}
__global__ __launch_bounds__(64) void k_mimi_attn(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                  float* __restrict__ o, int T, int window, float scale) {
    const int t = blockIdx.x;
    int j0 = t - window + 1; if (j0 < 0) j0 = 0;
    mimi_attn_col(q, k, v, o, T, t, j0, blockIdx.y, scale);
}
hipError_t launch_mimi_attn(const float* q, const float* k, const float* v, float* o, int nh, int hd, int T, int window, float scale,
                            hipStream_t st) {
    if (hd != 64 || nh <= 0 || T <= 0 || window <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mimi_attn, dim3(T, nh), dim3(64), 0, st, q, k, v, o, T, window, scale);
    return hipGetLastError();
}
// codebook = embed_sum / max(cluster_usage, 1e-5)  (MimiEuclideanCodebook.embed)
__global__ __launch_bounds__(256) void k_mimi_codebook(const float* __restrict__ esum, const float* __restrict__ usage, float* __restrict__ out, int dim) {
    const int e = blockIdx.x;
    const float u = fmaxf(usage[e], 1e-5f);
    for (int d = threadIdx.x; d < dim; d += 256) out[(size_t)e * dim + d] = esum[(size_t)e * dim + d] / u;
}
hipError_t launch_mimi_codebook(const float* esum, const float* usage, float* out, int CB, int dim, hipStream_t st) {
    if (CB < 1 || dim < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mimi_codebook, dim3(CB), dim3(256), 0, st, esum, usage, out, dim);
    return hipGetLastError();
}
// MimiResidualVectorQuantizer.encode for one group: proj [CD][T] (input_proj output), books = n_layers tables [CB][CD];
// codes[t*n_q + q0 + l] = argmin_e |r - e|^2 (first minimum), r -= e. One workgroup per frame.
__global__ __launch_bounds__(256) void k_mimi_rvq(const float* __restrict__ proj, int T, const float* __restrict__ books, int n_layers, int CB, int CD,
                                                  uint32_t* __restrict__ codes, int n_q, int q0) {
    __shared__ float r[256];
    __shared__ float bd[256]; __shared__ int bi[256];
    const int t = blockIdx.x, tid = threadIdx.x;
    if (tid < CD) r[tid] = proj[(size_t)tid * T + t];
    __syncthreads();
    for (int l = 0; l < n_layers; ++l) {
        const float* book = books + (size_t)l * CB * CD;
        float best = INFINITY; int bidx = 0x7fffffff;
        for (int e = tid; e < CB; e += 256) {
            const float* ev = book + (size_t)e * CD;
            float d2 = 0.0f;
            for (int d = 0; d < CD; ++d) { const float df = sub_rn(r[d], ev[d]); d2 = add_rn(d2, mul_rn(df, df)); }
            if (d2 < best) { best = d2; bidx = e; }            // ascending e per thread: the first minimum stays
        }
        bd[tid] = best; bi[tid] = bidx;
        __syncthreads();
        for (int s = 128; s >= 1; s >>= 1) {
            if (tid < s) {
                const float ob = bd[tid + s]; const int oi = bi[tid + s];
                if (ob < bd[tid] || (ob == bd[tid] && oi < bi[tid])) { bd[tid] = ob; bi[tid] = oi; }
            }
            __syncthreads();
        }
        const int win = bi[0];
        if (tid == 0) codes[(size_t)t * n_q + q0 + l] = (uint32_t)win;
        if (tid < CD) r[tid] = sub_rn(r[tid], book[(size_t)win * CD + tid]);
        __syncthreads();
    }
}
hipError_t launch_mimi_rvq(const float* proj, int T, const float* books, int n_layers, int CB, int CD, uint32_t* codes, int n_q, int q0,
                           hipStream_t st) {
    // the residual lives in r[256]; a layer's column q0 + l must lie inside a frame's n_q codes
    if (CD < 1 || CD > 256 || CB < 1 || n_layers < 1 || q0 < 0 || (long long)q0 + n_layers > n_q || T < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mimi_rvq, dim3(T), dim3(256), 0, st, proj, T, books, n_layers, CB, CD, codes, n_q, q0);
    return hipGetLastError();
}

// ---- packed instances (q3_mimi_encode_refs): n clips side by side along the time axis of the [C][W] tensors. Clip i
// owns a slot of `slot` columns from column `start`; its signal fills the first `len` of them, the rest — at least one 12.5 Hz
// frame — is its guard. These kernels write exact zeros into every slot column outside [start, start + len): the zeros the
// causal convs pad with when the clip is alone. One table entry per (stage, clip); the grid's z is the clip.
struct MimiClip { int start, len, slot, out; };        // out: the clip's first frame in the dense [C][sum of T] tensors behind the guards
__global__ __launch_bounds__(256) void k_mimi_elu_p(const MimiClip* __restrict__ tab, const float* __restrict__ x, float* __restrict__ y, int W) {
    const MimiClip cl = tab[blockIdx.z];
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= cl.slot) return;
    const size_t i = (size_t)blockIdx.y * W + cl.start + col;
    float r = 0.0f;
    if (col < cl.len) { const float v = x[i]; r = v > 0.0f ? v : expf(v) - 1.0f; }
    y[i] = r;
}
// x [C][W] -> y [C*r][W / r] (slot starts and widths are multiples of r): y[(c*r + p)][start/r + tau] = f(x[c][start + tau*r + p]), 0 beyond len
__global__ __launch_bounds__(256) void k_mimi_fold_p(const MimiClip* __restrict__ tab, const float* __restrict__ x, float* __restrict__ y, int W, int r, int elu) {
    const MimiClip cl = tab[blockIdx.z];
    const int col = blockIdx.x * 256 + threadIdx.x, cp = blockIdx.y;
    if (col >= cl.slot / r) return;
    const int c = cp / r, p = cp % r;
    const int i = col * r + p;
    float v = i < cl.len ? x[(size_t)c * W + cl.start + i] : 0.0f;
    if (elu) v = v > 0.0f ? v : expf(v) - 1.0f;
    y[(size_t)cp * (W / r) + cl.start / r + col] = v;
}
// the replicate-padded fold by 2 in front of the 12.5 Hz down-sampling conv: x [C][W] -> y [2C][W / 2], the clip's slot being
// len/2-rounded-up + 1 columns wide: column 0 of the slot holds x[c][start] for both phases, samples beyond len repeat the last one
__global__ __launch_bounds__(256) void k_mimi_fold_rep_p(const MimiClip* __restrict__ tab, const float* __restrict__ x, float* __restrict__ y, int W) {
    const MimiClip cl = tab[blockIdx.z];
    const int col = blockIdx.x * 256 + threadIdx.x, cp = blockIdx.y;
    if (col >= cl.slot / 2) return;
    const int c = cp / 2, p = cp % 2;
    const float* xr = x + (size_t)c * W + cl.start;
    float v;
    if (col == 0) v = xr[0];
    else {
        const int i = (col - 1) * 2 + p;
        v = i < cl.len ? xr[i] : xr[cl.len - 1];
    }
    y[(size_t)cp * (W / 2) + cl.start / 2 + col] = v;
}
// dst[c][out + t] = src[c][start + 1 + t], t < len: drops each slot's lead column and closes the guards (src [C][W], dst [C][Wd])
__global__ __launch_bounds__(256) void k_mimi_cols_p(const MimiClip* __restrict__ tab, const float* __restrict__ src, int W, float* __restrict__ dst, int Wd) {
    const MimiClip cl = tab[blockIdx.z];
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < cl.len) dst[(size_t)blockIdx.y * Wd + cl.out + t] = src[(size_t)blockIdx.y * W + cl.start + 1 + t];
}
// k_mimi_attn over the packed 25 Hz columns: first[t] = the first column of the clip that owns column t (-1: a guard column, whose
// output is zero), so the window starts at max(t - window + 1, first[t]) and the keys fall on the lanes as they do for the clip alone
__global__ __launch_bounds__(64) void k_mimi_attn_p(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                    float* __restrict__ o, int W, const int* __restrict__ first, int window, float scale) {
    const int t = blockIdx.x, s0 = first[t];
    if (s0 < 0) { o[((size_t)blockIdx.y * 64 + threadIdx.x) * W + t] = 0.0f; return; }
    int j0 = t - window + 1; if (j0 < s0) j0 = s0;
    mimi_attn_col(q, k, v, o, W, t, j0, blockIdx.y, scale);
}

}  // namespace q3

using namespace q3;

namespace {
struct MSlot { std::string name; int64_t n = 0; size_t offset = 0; bool loaded = false; int fold_r = 0, cout = 0, cin = 0, k = 0; };
struct MConv { const float* w = nullptr; const float* b = nullptr; const void* wpk = nullptr; int cin = 0, cout = 0, k = 1; };
struct MLayer { const float *ln1w, *ln1b, *ln2w, *ln2b, *sa, *sm; MConv q, k, v, o, f1, f2; };
std::string fm(const char* f, int a, int b = 0) { char buf[192]; snprintf(buf, sizeof buf, f, a, b); return buf; }
}  // namespace

struct q3_speech_encoder {
    q3_mimi_config cfg{};
    int device = 0;
    std::vector<MSlot> slots;
    std::unordered_map<std::string, int> index;
    char* arena = nullptr; size_t arena_bytes = 0;
    void* wpk_arena = nullptr;
    float* books[2] = {nullptr, nullptr};           // normalised codebooks per group
    bool finalized = false;
    hipStream_t st = nullptr;
    MConv c0, res1[4], res2[4], down[4], last, dsamp, qproj[2];
    std::vector<MLayer> layers;
    float* ws = nullptr; size_t ws_floats = 0;
    float *cs = nullptr, *sn = nullptr; int rope_T = 0;
    uint32_t* codes_dev = nullptr; int codes_cap = 0;
};

#define M_HIP(expr)                                                                                              \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) return q3i_set_err(Q3_HIP_ERROR, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static void m_add(q3_speech_encoder* e, const std::string& name, int64_t n, int fold_r = 0, int cout = 0, int cin = 0, int k = 0) {
    MSlot s; s.name = name; s.n = n; s.fold_r = fold_r; s.cout = cout; s.cin = cin; s.k = k;
    s.offset = (e->arena_bytes + 255) & ~(size_t)255;
    e->arena_bytes = s.offset + (size_t)n * 4;
    e->index[name] = (int)e->slots.size();
    e->slots.push_back(s);
}

extern "C" q3_status q3_mimi_config_default(q3_mimi_config* out) {
    if (!out) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_config_default: null");
    q3_mimi_config c{};
    c.n_filters = 64; c.hidden = 512; c.ratios[0] = 4; c.ratios[1] = 5; c.ratios[2] = 6; c.ratios[3] = 8;
    c.kernel = 7; c.res_kernel = 3; c.last_kernel = 3; c.compress = 2;
    c.n_layers = 8; c.n_heads = 8; c.head_dim = 64; c.inter = 2048; c.window = 250;
    c.cb_size = 2048; c.cb_dim = 256; c.n_q = 16; c.n_sem = 1; c.norm_eps = 1e-5f; c.rope_theta = 1e4f;
    *out = c;
    return Q3_OK;
}

extern "C" void q3_mimi_free(q3_speech_encoder* e) {
    if (!e) return;
    if (e->device >= 0) {
        (void)hipSetDevice(e->device);
        if (e->st) { (void)hipStreamSynchronize(e->st); (void)hipStreamDestroy(e->st); }
        (void)hipFree(e->arena); (void)hipFree(e->wpk_arena); (void)hipFree(e->books[0]); (void)hipFree(e->books[1]);
        (void)hipFree(e->ws); (void)hipFree(e->cs); (void)hipFree(e->sn); (void)hipFree(e->codes_dev);
    }
    delete e;
}

extern "C" q3_status q3_mimi_create(const q3_mimi_config* cfg, int device, q3_speech_encoder** out) {
    if (!cfg || !out) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_create: null argument");
    const q3_mimi_config& c = *cfg;
    if (c.n_filters < 1 || c.hidden < 1 || c.compress < 1 || c.n_filters % c.compress || c.kernel < 1 || c.res_kernel < 1 || c.last_kernel < 1 ||
        c.n_layers < 0 || c.n_heads < 1 || c.inter < 1 || c.window < 1 || c.cb_size < 2 || c.cb_dim < 1 || c.cb_dim > 256 || c.n_q < 1 ||
        c.n_sem < 1 || c.n_sem > c.n_q || c.n_q > 64)
        return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_create: bad config");
    for (int i = 0; i < 4; ++i) if (c.ratios[i] < 1 || c.ratios[i] > 16) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_create: bad ratio");
    if (c.head_dim != 64) return q3i_set_err(Q3_UNSUPPORTED, "speech encoder head_dim %d unsupported (64)", c.head_dim);
    if (c.n_heads * c.head_dim != c.hidden) return q3i_set_err(Q3_UNSUPPORTED, "speech encoder: n_heads * head_dim must equal hidden");
    auto* e = new q3_speech_encoder();
    e->cfg = c; e->device = device;
    const int F = c.n_filters, H = c.hidden;
    auto conv = [&](const std::string& p, int cout, int cin, int k, bool bias, int fold_r = 0) {
        m_add(e, p + ".weight", (int64_t)cout * cin * k, fold_r, cout, cin, k);
        if (bias) m_add(e, p + ".bias", cout);
    };
    conv("encoder.encoder.layers.0.conv", F, 1, c.kernel, true);
    int dim = F, li = 1;
    for (int s = 0; s < 4; ++s) {
        conv(fm("encoder.encoder.layers.%d.block.1.conv", li), dim / c.compress, dim, c.res_kernel, true);
        conv(fm("encoder.encoder.layers.%d.block.3.conv", li), dim, dim / c.compress, 1, true);
        conv(fm("encoder.encoder.layers.%d.conv", li + 2), 2 * dim, dim, 2 * c.ratios[s], true, c.ratios[s]);
        dim *= 2; li += 3;
    }
    conv(fm("encoder.encoder.layers.%d.conv", li + 1), H, dim, c.last_kernel, true);
    for (int l = 0; l < c.n_layers; ++l) {
        const std::string p = fm("encoder.encoder_transformer.layers.%d", l);
        conv(p + ".self_attn.q_proj", H, H, 1, false); conv(p + ".self_attn.k_proj", H, H, 1, false);
        conv(p + ".self_attn.v_proj", H, H, 1, false); conv(p + ".self_attn.o_proj", H, H, 1, false);
        conv(p + ".mlp.fc1", c.inter, H, 1, false); conv(p + ".mlp.fc2", H, c.inter, 1, false);
        m_add(e, p + ".input_layernorm.weight", H); m_add(e, p + ".input_layernorm.bias", H);
        m_add(e, p + ".post_attention_layernorm.weight", H); m_add(e, p + ".post_attention_layernorm.bias", H);
        m_add(e, p + ".self_attn_layer_scale.scale", H); m_add(e, p + ".mlp_layer_scale.scale", H);
    }
    conv("encoder.downsample.conv", H, H, 4, false, 2);
    for (int g = 0; g < 2; ++g) {
        const std::string p = std::string("encoder.quantizer.") + (g ? "acoustic" : "semantic") + "_residual_vector_quantizer";
        conv(p + ".input_proj", c.cb_dim, H, 1, false);
        const int nl = g ? c.n_q - c.n_sem : c.n_sem;
        for (int l = 0; l < nl; ++l) {
            m_add(e, p + fm(".layers.%d.codebook.embed_sum", l), (int64_t)c.cb_size * c.cb_dim);
            m_add(e, p + fm(".layers.%d.codebook.cluster_usage", l), c.cb_size);
        }
    }
    if (device >= 0) {
        hipError_t he = hipSetDevice(device);
        if (he == hipSuccess) he = hipMalloc((void**)&e->arena, e->arena_bytes);
        if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking);
        if (he != hipSuccess) { q3_mimi_free(e); return q3i_set_err(Q3_HIP_ERROR, "q3_mimi_create: %s", hipGetErrorString(he)); }
    }
    *out = e;
    return Q3_OK;
}

extern "C" q3_status q3_mimi_get_config(const q3_speech_encoder* e, q3_mimi_config* out) {
    if (!e || !out) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_get_config: null");
    *out = e->cfg;
    return Q3_OK;
}
extern "C" int q3_mimi_n_tensors(const q3_speech_encoder* e) { return e ? (int)e->slots.size() : 0; }
extern "C" q3_status q3_mimi_tensor_info(const q3_speech_encoder* e, int i, const char** name, int64_t* n) {
    if (!e || i < 0 || i >= (int)e->slots.size()) return q3i_set_err(Q3_INVALID_ARG, "speech-encoder tensor index out of range");
    if (name) *name = e->slots[i].name.c_str();
    if (n) *n = e->slots[i].n;
    return Q3_OK;
}

extern "C" q3_status q3_mimi_set_tensor(q3_speech_encoder* e, const char* name, const void* data, int src_dtype, int64_t n) {
    if (!e || !name || !data) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_set_tensor: null argument");
    if (e->device < 0) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_set_tensor: manifest-only handle");
    auto it = e->index.find(name);
    if (it == e->index.end()) return q3i_set_err(Q3_INVALID_ARG, "unknown speech-encoder tensor %s", name);
    MSlot& s = e->slots[it->second];
    if (s.n != n) return q3i_set_err(Q3_INVALID_ARG, "tensor %s: expected %lld elements, got %lld", name, (long long)s.n, (long long)n);
    M_HIP(hipSetDevice(e->device));
    std::vector<float> tmp((size_t)n);
    if (src_dtype == Q3_DTYPE_F32) memcpy(tmp.data(), data, (size_t)n * 4);
    else if (src_dtype == Q3_DTYPE_BF16) {
        const uint16_t* h = (const uint16_t*)data;
        for (int64_t i = 0; i < n; ++i) { uint32_t u = (uint32_t)h[i] << 16; memcpy(&tmp[(size_t)i], &u, 4); }
    } else return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_set_tensor: unsupported source dtype %d", src_dtype);
    if (s.fold_r > 0) {
        // strided conv [cout][cin][2r] -> folded 2-tap causal conv [cout][cin*r][2]: w'[co][ci*r + p][j] = w[co][ci][j*r + p]
        const int r = s.fold_r, cout = s.cout, cin = s.cin;
        std::vector<float> f((size_t)n);
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int j = 0; j < 2; ++j)
                    for (int p = 0; p < r; ++p)
                        f[(((size_t)co * cin + ci) * r + p) * 2 + j] = tmp[((size_t)co * cin + ci) * 2 * r + (size_t)j * r + p];
        tmp.swap(f);
    }
    M_HIP(q3_hipMemcpy(e->arena + s.offset, tmp.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    s.loaded = true; e->finalized = false;
    return Q3_OK;
}

static MConv m_conv(q3_speech_encoder* e, const std::string& prefix, int cout, int cin, int k, bool bias) {
    MConv c; c.cout = cout; c.cin = cin; c.k = k;
    c.w = (const float*)(e->arena + e->slots[e->index[prefix + ".weight"]].offset);
    c.b = bias ? (const float*)(e->arena + e->slots[e->index[prefix + ".bias"]].offset) : nullptr;
    return c;
}
static const float* m_vec(q3_speech_encoder* e, const std::string& name) { return (const float*)(e->arena + e->slots[e->index[name]].offset); }

extern "C" q3_status q3_mimi_finalize(q3_speech_encoder* e) {
    if (!e) return q3i_set_err(Q3_INVALID_ARG, "null speech encoder");
    if (e->device < 0) return q3i_set_err(Q3_UNSUPPORTED, "manifest-only handle cannot be finalized");
    for (auto& s : e->slots) if (!s.loaded) return q3i_set_err(Q3_MISSING_WEIGHT, "Missing weight: %s", s.name.c_str());
    M_HIP(hipSetDevice(e->device));
    const q3_mimi_config& c = e->cfg;
    const int F = c.n_filters, H = c.hidden;
    e->c0 = m_conv(e, "encoder.encoder.layers.0.conv", F, 1, c.kernel, true);
    int dim = F, li = 1;
    for (int s = 0; s < 4; ++s) {
        e->res1[s] = m_conv(e, fm("encoder.encoder.layers.%d.block.1.conv", li), dim / c.compress, dim, c.res_kernel, true);
        e->res2[s] = m_conv(e, fm("encoder.encoder.layers.%d.block.3.conv", li), dim, dim / c.compress, 1, true);
        e->down[s] = m_conv(e, fm("encoder.encoder.layers.%d.conv", li + 2), 2 * dim, dim * c.ratios[s], 2, true);      // folded form
        dim *= 2; li += 3;
    }
    e->last = m_conv(e, fm("encoder.encoder.layers.%d.conv", li + 1), H, dim, c.last_kernel, true);
    e->layers.resize(c.n_layers);
    for (int l = 0; l < c.n_layers; ++l) {
        const std::string p = fm("encoder.encoder_transformer.layers.%d", l);
        MLayer& L = e->layers[l];
        L.q = m_conv(e, p + ".self_attn.q_proj", H, H, 1, false); L.k = m_conv(e, p + ".self_attn.k_proj", H, H, 1, false);
        L.v = m_conv(e, p + ".self_attn.v_proj", H, H, 1, false); L.o = m_conv(e, p + ".self_attn.o_proj", H, H, 1, false);
        L.f1 = m_conv(e, p + ".mlp.fc1", c.inter, H, 1, false); L.f2 = m_conv(e, p + ".mlp.fc2", H, c.inter, 1, false);
        L.ln1w = m_vec(e, p + ".input_layernorm.weight"); L.ln1b = m_vec(e, p + ".input_layernorm.bias");
        L.ln2w = m_vec(e, p + ".post_attention_layernorm.weight"); L.ln2b = m_vec(e, p + ".post_attention_layernorm.bias");
        L.sa = m_vec(e, p + ".self_attn_layer_scale.scale"); L.sm = m_vec(e, p + ".mlp_layer_scale.scale");
    }
    e->dsamp = m_conv(e, "encoder.downsample.conv", H, H * 2, 2, false);        // folded form (stride 2)
    for (int g = 0; g < 2; ++g) {
        const std::string p = std::string("encoder.quantizer.") + (g ? "acoustic" : "semantic") + "_residual_vector_quantizer";
        e->qproj[g] = m_conv(e, p + ".input_proj", c.cb_dim, H, 1, false);
        const int nl = g ? c.n_q - c.n_sem : c.n_sem;
        if (!e->books[g] && nl > 0) M_HIP(hipMalloc((void**)&e->books[g], (size_t)nl * c.cb_size * c.cb_dim * 4));
        for (int l = 0; l < nl; ++l)
            M_HIP(launch_mimi_codebook(m_vec(e, p + fm(".layers.%d.codebook.embed_sum", l)), m_vec(e, p + fm(".layers.%d.codebook.cluster_usage", l)),
                                       e->books[g] + (size_t)l * c.cb_size * c.cb_dim, c.cb_size, c.cb_dim, e->st));
    }
    // bf16x3 matrix-core images of every conv whose channel counts allow it (cout % 32 == 0, cin % 16 == 0)
    std::vector<MConv*> all = {&e->c0, &e->last, &e->dsamp, &e->qproj[0], &e->qproj[1]};
    for (int s = 0; s < 4; ++s) { all.push_back(&e->res1[s]); all.push_back(&e->res2[s]); all.push_back(&e->down[s]); }
    for (auto& L : e->layers) { all.push_back(&L.q); all.push_back(&L.k); all.push_back(&L.v); all.push_back(&L.o); all.push_back(&L.f1); all.push_back(&L.f2); }
    size_t total = 0;
    for (MConv* cv : all) if (cv->cout % 32 == 0 && cv->cin % 16 == 0) total += packed_conv_w_bytes(cv->cout, cv->cin, cv->k);
    if (total) {
        if (e->wpk_arena) { M_HIP(hipFree(e->wpk_arena)); e->wpk_arena = nullptr; }
        M_HIP(hipMalloc(&e->wpk_arena, total));
        char* cur = (char*)e->wpk_arena;
        for (MConv* cv : all) {
            cv->wpk = nullptr;
            if (cv->cout % 32 || cv->cin % 16) continue;
            M_HIP(launch_pack_conv_w(cv->w, cur, cv->cout, cv->cin, cv->k, e->st));
            cv->wpk = cur; cur += packed_conv_w_bytes(cv->cout, cv->cin, cv->k);
        }
    }
    M_HIP(hipGetLastError());
    M_HIP(hipStreamSynchronize(e->st));
    e->finalized = true;
    return Q3_OK;
}

static int m_ceil_div(int64_t a, int b) { return (int)((a + b - 1) / b); }
extern "C" int q3_mimi_frames(const q3_mimi_config* c, int64_t n_samples) {
    if (!c || n_samples < 1) return 0;
    for (int i = 0; i < 4; ++i) if (c->ratios[i] < 1 || c->ratios[i] > 16) return 0;      // (q3_mimi_create's range)
    if (n_samples > ((int64_t)1 << 48)) return -1;                                       // no count
    int64_t L = n_samples;
    for (int i = 0; i < 4; ++i) L = (L + c->ratios[i] - 1) / c->ratios[i];
    L = (L + 1) / 2;
    return L > 0x7fffffffLL ? -1 : (int)L;                                               // no count either: it does not fit
}

static hipError_t m_run_conv(q3_speech_encoder* e, const MConv& cv, const float* x, float* y, int L, int act = 0, const float* resid = nullptr,
                             const float* scale = nullptr) {
    ConvArgs a{}; a.x = x; a.w = cv.w; a.b = cv.b; a.y = y; a.cin = cv.cin; a.cout = cv.cout; a.L = L; a.k = cv.k; a.dil = 1;
    a.act = act; a.resid = resid; a.scale = scale; a.wpk = cv.wpk;
    return launch_conv1d(a, e->st);
}

// codes_host [T][n_q]; taps_host: NULL or 3 host pointers (NULL entries skipped): SEANet out [hidden][T25], transformer out [hidden][T25],
// downsampled [hidden][T]
static q3_status mimi_encode_from(q3_speech_encoder* e, const float* samples, hipMemcpyKind kind, int64_t n, uint32_t* codes_host,
                                  int cap_frames, int* n_frames, float** taps_host);

extern "C" q3_status q3_mimi_encode(q3_speech_encoder* e, const float* samples, int64_t n, uint32_t sample_rate, uint32_t* codes_host,
                                    int cap_frames, int* n_frames, float** taps_host) {
    if (!e || !samples || !n_frames) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_encode: null argument");
    if (!e->finalized) return q3i_set_err(Q3_INVALID_ARG, "speech encoder not finalized");
    if (sample_rate != 24000) return q3i_set_err(Q3_INVALID_ARG, "speech encoder expects 24000 Hz audio, got %u (resample first: q3_resample)", sample_rate);
    return mimi_encode_from(e, samples, hipMemcpyHostToDevice, n, codes_host, cap_frames, n_frames, taps_host);
}

// the same for samples that are on the encoder's device already (q3_intake.hip): the first conv's input buffer is reused further
// down, so they are copied into it, device to device, by the encoder's own stream
extern "C" q3_status q3_mimi_encode_ref(q3_speech_encoder* e, const q3_ref_audio* r, uint32_t* codes_host, int cap_frames, int* n_frames,
                                        float** taps_host) {
    if (!e || !r || !n_frames) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_encode_ref: null argument");
    int64_t n = 0; int dev = 0;
    const float* x_d = q3i_ref_audio_dev(r, &n, &dev);
    if (dev != e->device) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_encode_ref: reference audio is on device %d, the encoder on device %d", dev, e->device);
    if (!e->finalized) return q3i_set_err(Q3_INVALID_ARG, "speech encoder not finalized");
    return mimi_encode_from(e, x_d, hipMemcpyDeviceToDevice, n, codes_host, cap_frames, n_frames, taps_host);
}

// the workspace, the RoPE tables for T25 positions and the device-side codes of T frames, each grown when a call needs more
static q3_status mimi_reserve(q3_speech_encoder* e, size_t need, int T25, int T) {
    const q3_mimi_config& c = e->cfg;
    if (need > e->ws_floats) {
        M_HIP(hipStreamSynchronize(e->st));
        if (e->ws) M_HIP(hipFree(e->ws));
        e->ws = nullptr; e->ws_floats = 0;
        M_HIP(hipMalloc((void**)&e->ws, need * 4));
        e->ws_floats = need;
    }
    if (T25 > e->rope_T) {
        if (e->cs) { M_HIP(hipFree(e->cs)); M_HIP(hipFree(e->sn)); e->cs = e->sn = nullptr; }
        const int cap = T25 + 64;
        std::vector<float> cs((size_t)cap * 32), sn((size_t)cap * 32);
        for (int i = 0; i < 32; ++i) {         // MimiRotaryEmbedding: inv_freq = theta^(-2i/64), freqs = pos * inv_freq in f32 (host libm, as the oracle)
            const float inv = 1.0f / powf(c.rope_theta, (float)(2 * i) / 64.0f);
            for (int t = 0; t < cap; ++t) { const float f = (float)t * inv; cs[(size_t)t * 32 + i] = cosf(f); sn[(size_t)t * 32 + i] = sinf(f); }
        }
        M_HIP(hipMalloc((void**)&e->cs, cs.size() * 4)); M_HIP(hipMalloc((void**)&e->sn, sn.size() * 4));
        M_HIP(q3_hipMemcpy(e->cs, cs.data(), cs.size() * 4, hipMemcpyHostToDevice)); M_HIP(q3_hipMemcpy(e->sn, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
        e->rope_T = cap;
    }
    if (T > e->codes_cap) {
        if (e->codes_dev) M_HIP(hipFree(e->codes_dev));
        e->codes_dev = nullptr; e->codes_cap = 0;
        M_HIP(hipMalloc((void**)&e->codes_dev, (size_t)(T + 64) * c.n_q * 4));
        e->codes_cap = T + 64;
    }
    return Q3_OK;
}

// q3_mimi_encode behind its checks of handle and rate: `samples` on the host or on the encoder's device, as `kind` says
static q3_status mimi_encode_from(q3_speech_encoder* e, const float* samples, hipMemcpyKind kind, int64_t n, uint32_t* codes_host,
                                  int cap_frames, int* n_frames, float** taps_host) {
    if (n < 1 || n > (int64_t)24000 * 120) return q3i_set_err(Q3_INVALID_ARG, "reference audio of %lld samples unsupported (1 .. 120 s)", (long long)n);
    const q3_mimi_config& c = e->cfg;
    const int T = q3_mimi_frames(&c, n);
    *n_frames = T;
    if (!codes_host) return Q3_OK;
    if (cap_frames < T) return q3i_set_err(Q3_INVALID_ARG, "codes buffer too small (%d < %d frames)", cap_frames, T);
    M_HIP(hipSetDevice(e->device));
    const int F = c.n_filters, H = c.hidden;
    // workspace: three ping-pong buffers of the largest [C][L] activation (+ folding slack), the transformer's q|k|v|att, the MLP hidden
    int Ls[6]; Ls[0] = (int)n;
    for (int s = 0; s < 4; ++s) Ls[s + 1] = m_ceil_div(Ls[s], c.ratios[s]);
    const int T25 = Ls[4];
    size_t big = 0; { int dim = F; for (int s = 0; s < 4; ++s) { const size_t v = (size_t)dim * ((size_t)Ls[s] + 16 * c.ratios[s]); if (v > big) big = v; dim *= 2; }
                      const size_t v = (size_t)dim * (Ls[4] + 2); if (v > big) big = v; }
    const size_t tf = (size_t)T25 + 4;
    const size_t need = 3 * big + (size_t)(5 * H + c.inter) * tf + (size_t)2 * H * tf + (size_t)c.cb_dim * (T + 2) + 64;
    Q3I_CHECK(mimi_reserve(e, need, T25, T));
    float* A = e->ws; float* B = A + big; float* C = B + big; float* tr = C + big;
    hipStream_t st = e->st;
    auto TAP = [&](int id, const float* dev, size_t cnt) -> q3_status {
        if (taps_host && taps_host[id]) { M_HIP(hipStreamSynchronize(st)); M_HIP(q3_hipMemcpy(taps_host[id], dev, cnt * 4, hipMemcpyDeviceToHost)); }
        return Q3_OK;
    };
    // ---- SEANet ----
    M_HIP(hipMemcpyAsync(C, samples, (size_t)n * 4, kind, st));
    M_HIP(m_run_conv(e, e->c0, C, A, (int)n));                                          // x = A [F][n]
    float* x = A; float* o1 = B; float* o2 = C;
    int dim = F, L = (int)n;
    for (int s = 0; s < 4; ++s) {
        const int r = c.ratios[s], hid = dim / c.compress;
        // MimiResnetBlock: x + conv1(ELU(conv3(ELU(x))))
        M_HIP(launch_mimi_elu(x, o1, (size_t)dim * L, st));
        M_HIP(m_run_conv(e, e->res1[s], o1, o2, L, /*ELU*/ 6));                         // o2 [hid][L]
        M_HIP(m_run_conv(e, e->res2[s], o2, o1, L, 0, x));                              // o1 = x + conv1(.)  [dim][L]
        (void)hid;
        // ELU + strided conv as fold + 2-tap conv
        const int Lf = m_ceil_div(L, r);
        M_HIP(launch_mimi_fold(o1, o2, dim, L, r, Lf, 1, 0, st));                       // o2 [dim*r][Lf]
        M_HIP(m_run_conv(e, e->down[s], o2, x, Lf));                                    // x [2dim][Lf]
        dim *= 2; L = Lf;
    }
    M_HIP(launch_mimi_elu(x, o1, (size_t)dim * L, st));
    float* hs = o2;                                                                     // [H][T25]
    M_HIP(m_run_conv(e, e->last, o1, hs, L));
    Q3I_CHECK(TAP(0, hs, (size_t)H * T25));
    // ---- transformer ----
    float* nrm = tr; float* q = nrm + (size_t)H * tf; float* k = q + (size_t)H * tf; float* v = k + (size_t)H * tf; float* att = v + (size_t)H * tf;
    float* ff = att + (size_t)H * tf;
    const float scale = 1.0f / sqrtf(64.0f);
    for (auto& Lr : e->layers) {
        M_HIP(launch_layernorm_c(hs, Lr.ln1w, Lr.ln1b, nrm, H, T25, c.norm_eps, st));
        M_HIP(m_run_conv(e, Lr.q, nrm, q, T25)); M_HIP(m_run_conv(e, Lr.k, nrm, k, T25)); M_HIP(m_run_conv(e, Lr.v, nrm, v, T25));
        M_HIP(launch_rope_c(q, k, e->cs, e->sn, c.n_heads, 64, T25, st));
        M_HIP(launch_mimi_attn(q, k, v, att, c.n_heads, 64, T25, c.window, scale, st));
        M_HIP(m_run_conv(e, Lr.o, att, hs, T25, 0, hs, Lr.sa));                          // hs += scale_attn * o_proj(att)
        M_HIP(launch_layernorm_c(hs, Lr.ln2w, Lr.ln2b, nrm, H, T25, c.norm_eps, st));
        M_HIP(m_run_conv(e, Lr.f1, nrm, ff, T25, /*GELU*/ 1));
        M_HIP(m_run_conv(e, Lr.f2, ff, hs, T25, 0, hs, Lr.sm));                          // hs += scale_mlp * fc2(gelu(fc1))
    }
    Q3I_CHECK(TAP(1, hs, (size_t)H * T25));
    // ---- downsample: k = 4, stride 2, replicate padding -> fold with a leading replicate column, drop output column 0 ----
    float* fd = ff + (size_t)c.inter * tf;                                              // [2H][T + 1]
    float* dy = x;                                                                      // [H][T + 1] (x is free now)
    M_HIP(launch_mimi_fold(hs, fd, H, T25, 2, T, 0, 1, st));
    M_HIP(m_run_conv(e, e->dsamp, fd, dy, T + 1));
    float* xd = o1;                                                                     // [H][T]
    M_HIP(launch_copy_rows(dy + 1, T + 1, xd, T, H, T, st));
    Q3I_CHECK(TAP(2, xd, (size_t)H * T));
    // ---- split residual vector quantiser ----
    float* proj = fd + (size_t)2 * H * tf;
    for (int g = 0; g < 2; ++g) {
        const int nl = g ? c.n_q - c.n_sem : c.n_sem, q0 = g ? c.n_sem : 0;
        if (nl <= 0) continue;
        M_HIP(m_run_conv(e, e->qproj[g], xd, proj, T));
        M_HIP(launch_mimi_rvq(proj, T, e->books[g], nl, c.cb_size, c.cb_dim, e->codes_dev, c.n_q, q0, st));
    }
    M_HIP(hipGetLastError());
    M_HIP(hipStreamSynchronize(st));
    M_HIP(q3_hipMemcpy(codes_host, e->codes_dev, (size_t)T * c.n_q * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// ---- many clips in one packed pass of the encoder ----
// Pure host arithmetic, no HIP call: where each clip's slot lies. A slot is the clip's frames plus one guard frame, S = 2 * prod(ratios)
// samples per frame, so a slot starts on a whole column at every SEANet stage and on an even column at 25 Hz. Packable: one guard
// frame covers the left context of every conv (kernel - 1 samples at stage 0, res_kernel - 1 columns at each stage, last_kernel - 1
// at 25 Hz; a folded strided conv reaches one column back, and every stage has at least two columns per frame).
extern "C" q3_status q3_mimi_pack_plan(const q3_mimi_config* cfg, const int64_t* n_samples, int n, int64_t max_pass_samples, q3_mimi_pack_clip* clips,
                                       int64_t* frame_samples, int* packable, int* n_passes) {
    if (!cfg || !n_samples || !clips) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_pack_plan: null argument");
    if (n < 1 || n > 64) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_pack_plan: %d clips (1 .. 64)", n);
    if (max_pass_samples < 1) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_pack_plan: max_pass_samples %lld", (long long)max_pass_samples);
    int64_t S = 2;
    for (int s = 0; s < 4; ++s) {
        if (cfg->ratios[s] < 1 || cfg->ratios[s] > 16) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_pack_plan: bad ratio");
        S *= cfg->ratios[s];
    }
    bool ok = cfg->kernel >= 1 && cfg->res_kernel >= 1 && cfg->last_kernel >= 1 && cfg->kernel - 1 <= S && cfg->last_kernel - 1 <= 2;
    int64_t cpf = S;                                                   // columns per frame at stage s
    for (int s = 0; s < 4; ++s) { if (cfg->res_kernel - 1 > cpf) ok = false; cpf /= cfg->ratios[s]; }
    int pass = 0; int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        if (n_samples[i] < 1) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_pack_plan: clip %d: %lld samples", i, (long long)n_samples[i]);
        const int T = q3_mimi_frames(cfg, n_samples[i]);
        if (T < 0) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_pack_plan: clip %d: %lld samples are more frames than a count holds", i, (long long)n_samples[i]);
        const int64_t slot = ((int64_t)T + 1) * S;
        if (at > 0 && at + slot > max_pass_samples) { ++pass; at = 0; }      // (a clip whose own slot is larger gets a pass to itself)
        clips[i].frames = T; clips[i].pass = pass; clips[i].start = at;
        at += slot;
    }
    if (frame_samples) *frame_samples = S;
    if (packable) *packable = ok ? 1 : 0;
    if (n_passes) *n_passes = pass + 1;
    return Q3_OK;
}

// one pass: clips xs[i] (ns[i] samples, on the encoder's device) in the slots pc[i]; codes_host [sum of T][n_q], clip after clip;
// taps_host: NULL or 3 pointers per clip. mimi_encode_from with the packed width in place of the clip's length: the same convs in
// the same order over all slots at once, the elementwise steps as their packed instances.
static q3_status mimi_encode_packed(q3_speech_encoder* e, const float* const* xs, const int64_t* ns, const q3_mimi_pack_clip* pc, int n, int64_t S,
                                    uint32_t* codes_host, float** taps_host) {
    const q3_mimi_config& c = e->cfg;
    const int F = c.n_filters, H = c.hidden;
    hipStream_t st = e->st;
    int64_t W0 = 0; int Tsum = 0, maxT = 0, maxT25 = 0;
    for (int i = 0; i < n; ++i) { W0 += ((int64_t)pc[i].frames + 1) * S; Tsum += pc[i].frames; maxT = std::max(maxT, pc[i].frames); }
    if (W0 > 0x7fffffffLL - 4096) return q3i_set_err(Q3_INVALID_ARG, "packed pass of %lld samples unsupported", (long long)W0);
    int Ws[5]; Ws[0] = (int)W0;
    for (int s = 0; s < 4; ++s) Ws[s + 1] = Ws[s] / c.ratios[s];
    const int W25 = Ws[4], W12 = W25 / 2;
    // the tables: stage s = 0 .. 4 (the SEANet rates, 4 = 25 Hz), 5 = 12.5 Hz; first / pos per 25 Hz column
    std::vector<MimiClip> tab((size_t)6 * n);
    std::vector<int> colinfo((size_t)2 * W25, 0);
    int* first_h = colinfo.data(); int* pos_h = first_h + W25;
    for (int t = 0; t < W25; ++t) first_h[t] = -1;
    int out = 0;
    for (int i = 0; i < n; ++i) {
        int64_t div = 1, L = ns[i];
        for (int s = 0; s < 5; ++s) {
            tab[(size_t)s * n + i] = MimiClip{(int)(pc[i].start / div), (int)L, (int)(((int64_t)pc[i].frames + 1) * S / div), 0};
            if (s < 4) { div *= c.ratios[s]; L = (L + c.ratios[s] - 1) / c.ratios[s]; }
        }
        const MimiClip& c25 = tab[(size_t)4 * n + i];
        maxT25 = std::max(maxT25, c25.len);
        for (int t = 0; t < c25.len; ++t) { first_h[c25.start + t] = c25.start; pos_h[c25.start + t] = t; }
        tab[(size_t)5 * n + i] = MimiClip{c25.start / 2, pc[i].frames, pc[i].frames + 1, out};
        out += pc[i].frames;
    }
    size_t big = 0; { int dim = F; for (int s = 0; s < 4; ++s) { const size_t v = (size_t)dim * ((size_t)Ws[s] + 16 * c.ratios[s]); if (v > big) big = v; dim *= 2; }
                      const size_t v = (size_t)dim * (Ws[4] + 2); if (v > big) big = v; }
    const size_t tf = (size_t)W25 + 4;
    const size_t floats = 3 * big + (size_t)(5 * H + c.inter) * tf + (size_t)2 * H * tf + (size_t)c.cb_dim * (W12 + 2) + 64;
    const size_t ints = tab.size() * 4 + colinfo.size();
    Q3I_CHECK(mimi_reserve(e, floats + ints + 64, maxT25, Tsum));
    float* A = e->ws; float* B = A + big; float* C = B + big; float* tr = C + big;
    MimiClip* tab_d = (MimiClip*)(e->ws + ((floats + 3) & ~(size_t)3));
    int* first_d = (int*)(tab_d + tab.size()); int* pos_d = first_d + W25;
    M_HIP(hipMemcpyAsync(tab_d, tab.data(), tab.size() * sizeof(MimiClip), hipMemcpyHostToDevice, st));
    M_HIP(hipMemcpyAsync(first_d, colinfo.data(), colinfo.size() * 4, hipMemcpyHostToDevice, st));
    // tap `id` of every clip: its columns [start, start + len) of src [H][ld]
    auto TAP = [&](int id, const float* dev, int ld, int stage, bool dense) -> q3_status {
        if (!taps_host) return Q3_OK;
        bool any = false;
        for (int i = 0; i < n; ++i) {
            float* dst = taps_host[(size_t)3 * i + id];
            if (!dst) continue;
            const MimiClip& cl = tab[(size_t)stage * n + i];
            M_HIP(hipMemcpy2DAsync(dst, (size_t)cl.len * 4, dev + (dense ? cl.out : cl.start), (size_t)ld * 4, (size_t)cl.len * 4, H, hipMemcpyDeviceToHost, st));
            any = true;
        }
        if (any) M_HIP(hipStreamSynchronize(st));
        return Q3_OK;
    };
    // ---- SEANet ----
    M_HIP(hipMemsetAsync(C, 0, (size_t)W0 * 4, st));
    for (int i = 0; i < n; ++i) M_HIP(hipMemcpyAsync(C + pc[i].start, xs[i], (size_t)ns[i] * 4, hipMemcpyDeviceToDevice, st));
    M_HIP(m_run_conv(e, e->c0, C, A, Ws[0]));
    float* x = A; float* o1 = B; float* o2 = C;
    int dim = F; int64_t maxslot = ((int64_t)maxT + 1) * S;                             // the widest slot, in columns of the current stage
    for (int s = 0; s < 4; ++s) {
        const int r = c.ratios[s], W = Ws[s];
        if ((long long)dim * r > 65535) return q3i_set_err(Q3_INVALID_ARG, "speech encoder: %d folded channels unsupported", dim * r);
        const MimiClip* ts = tab_d + (size_t)s * n;
        hipLaunchKernelGGL(k_mimi_elu_p, dim3((unsigned)((maxslot + 255) / 256), dim, n), dim3(256), 0, st, ts, x, o1, W);
        M_HIP(hipGetLastError());
        M_HIP(m_run_conv(e, e->res1[s], o1, o2, W, /*ELU*/ 6));
        M_HIP(m_run_conv(e, e->res2[s], o2, o1, W, 0, x));
        hipLaunchKernelGGL(k_mimi_fold_p, dim3((unsigned)((maxslot / r + 255) / 256), dim * r, n), dim3(256), 0, st, ts, o1, o2, W, r, 1);
        M_HIP(hipGetLastError());
        M_HIP(m_run_conv(e, e->down[s], o2, x, W / r));
        dim *= 2; maxslot /= r;
    }
    hipLaunchKernelGGL(k_mimi_elu_p, dim3((unsigned)((maxslot + 255) / 256), dim, n), dim3(256), 0, st, tab_d + (size_t)4 * n, x, o1, W25);
    M_HIP(hipGetLastError());
    float* hs = o2;                                                                     // [H][W25]
    M_HIP(m_run_conv(e, e->last, o1, hs, W25));
    Q3I_CHECK(TAP(0, hs, W25, 4, false));
    // ---- transformer: per-column work over the packed width; RoPE by the position inside the clip, attention inside the clip ----
    float* nrm = tr; float* q = nrm + (size_t)H * tf; float* k = q + (size_t)H * tf; float* v = k + (size_t)H * tf; float* att = v + (size_t)H * tf;
    float* ff = att + (size_t)H * tf;
    const float scale = 1.0f / sqrtf(64.0f);
    for (auto& Lr : e->layers) {
        M_HIP(launch_layernorm_c(hs, Lr.ln1w, Lr.ln1b, nrm, H, W25, c.norm_eps, st));
        M_HIP(m_run_conv(e, Lr.q, nrm, q, W25)); M_HIP(m_run_conv(e, Lr.k, nrm, k, W25)); M_HIP(m_run_conv(e, Lr.v, nrm, v, W25));
        M_HIP(launch_rope_c_pos(q, k, e->cs, e->sn, pos_d, c.n_heads, 64, W25, st));
        hipLaunchKernelGGL(k_mimi_attn_p, dim3(W25, c.n_heads), dim3(64), 0, st, q, k, v, att, W25, first_d, c.window, scale);
        M_HIP(hipGetLastError());
        M_HIP(m_run_conv(e, Lr.o, att, hs, W25, 0, hs, Lr.sa));
        M_HIP(launch_layernorm_c(hs, Lr.ln2w, Lr.ln2b, nrm, H, W25, c.norm_eps, st));
        M_HIP(m_run_conv(e, Lr.f1, nrm, ff, W25, /*GELU*/ 1));
        M_HIP(m_run_conv(e, Lr.f2, ff, hs, W25, 0, hs, Lr.sm));
    }
    Q3I_CHECK(TAP(1, hs, W25, 4, false));
    // ---- downsample: every slot with its own replicate lead column; the lead outputs are dropped and the guards closed ----
    float* fd = ff + (size_t)c.inter * tf;                                              // [2H][W12]
    float* dy = x;                                                                      // [H][W12]
    hipLaunchKernelGGL(k_mimi_fold_rep_p, dim3((unsigned)((maxT + 1 + 255) / 256), 2 * H, n), dim3(256), 0, st, tab_d + (size_t)4 * n, hs, fd, W25);
    M_HIP(hipGetLastError());
    M_HIP(m_run_conv(e, e->dsamp, fd, dy, W12));
    float* xd = o1;                                                                     // [H][Tsum]
    hipLaunchKernelGGL(k_mimi_cols_p, dim3((unsigned)((maxT + 255) / 256), H, n), dim3(256), 0, st, tab_d + (size_t)5 * n, dy, W12, xd, Tsum);
    M_HIP(hipGetLastError());
    Q3I_CHECK(TAP(2, xd, Tsum, 5, true));
    // ---- split residual vector quantiser over every clip's frames at once ----
    float* proj = fd + (size_t)2 * H * tf;
    for (int g = 0; g < 2; ++g) {
        const int nl = g ? c.n_q - c.n_sem : c.n_sem, q0 = g ? c.n_sem : 0;
        if (nl <= 0) continue;
        M_HIP(m_run_conv(e, e->qproj[g], xd, proj, Tsum));
        M_HIP(launch_mimi_rvq(proj, Tsum, e->books[g], nl, c.cb_size, c.cb_dim, e->codes_dev, c.n_q, q0, st));
    }
    M_HIP(hipGetLastError());
    M_HIP(hipStreamSynchronize(st));
    M_HIP(q3_hipMemcpy(codes_host, e->codes_dev, (size_t)Tsum * c.n_q * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// Encoder12Hz::encode (encoder_12hz.rs:119-144) of n reference-audio objects: codes_host [sum of n_frames][n_q], clip after clip
extern "C" q3_status q3_mimi_encode_refs(q3_speech_encoder* e, const q3_ref_audio* const* refs, int n, uint32_t* codes_host, int cap_frames,
                                         int* n_frames, float** taps_host) {
    if (!e || !refs || !n_frames) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_encode_refs: null argument");
    if (n < 1 || n > 64) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_encode_refs: %d clips (1 .. 64)", n);
    for (int i = 0; i < n; ++i)
        if (!refs[i]) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_encode_refs: clip %d: null entry", i);
    const int64_t LIMIT = (int64_t)24000 * 120;
    std::vector<const float*> xs((size_t)n); std::vector<int64_t> ns((size_t)n);
    for (int i = 0; i < n; ++i) {
        int dev = 0;
        xs[i] = q3i_ref_audio_dev(refs[i], &ns[i], &dev);
        if (dev != e->device)
            return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_encode_refs: clip %d: reference audio is on device %d, the encoder on device %d", i, dev, e->device);
    }
    if (!e->finalized) return q3i_set_err(Q3_INVALID_ARG, "speech encoder not finalized");
    for (int i = 0; i < n; ++i)
        if (ns[i] < 1 || ns[i] > LIMIT)
            return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_encode_refs: clip %d: reference audio of %lld samples unsupported (1 .. 120 s)", i, (long long)ns[i]);
    std::vector<q3_mimi_pack_clip> pc((size_t)n);
    int64_t S = 0; int packable = 0, passes = 0;
    Q3I_CHECK(q3_mimi_pack_plan(&e->cfg, ns.data(), n, LIMIT, pc.data(), &S, &packable, &passes));
    long long total = 0;
    for (int i = 0; i < n; ++i) { n_frames[i] = pc[i].frames; total += pc[i].frames; }
    if (!codes_host) return Q3_OK;
    if (cap_frames < total) return q3i_set_err(Q3_INVALID_ARG, "q3_mimi_encode_refs: codes buffer too small (%d < %lld frames)", cap_frames, total);
    M_HIP(hipSetDevice(e->device));
    size_t frame0 = 0;
    for (int first = 0; first < n;) {
        int np = 1;
        while (first + np < n && pc[first + np].pass == pc[first].pass) ++np;
        uint32_t* codes = codes_host + frame0 * e->cfg.n_q;
        float** taps = taps_host ? taps_host + (size_t)3 * first : nullptr;
        // clip by clip where one guard frame does not cover the convs' context, and for a clip whose slot alone exceeds a pass
        if (!packable || (np == 1 && ((int64_t)pc[first].frames + 1) * S > LIMIT)) {
            for (int i = first; i < first + np; ++i) {
                int nf = 0;
                Q3I_CHECK(mimi_encode_from(e, xs[i], hipMemcpyDeviceToDevice, ns[i], codes, pc[i].frames, &nf, taps ? taps + (size_t)3 * (i - first) : nullptr));
                codes += (size_t)nf * e->cfg.n_q;
            }
        } else {
            Q3I_CHECK(mimi_encode_packed(e, xs.data() + first, ns.data() + first, pc.data() + first, np, S, codes, taps));
        }
        for (int i = first; i < first + np; ++i) frame0 += pc[i].frames;
        first += np;
    }
    return Q3_OK;
}
