// q3_intake.hip — the reference-audio intake: a clip as it lies on disk -> 24 kHz mono f32 on the device, in one launch
// (a unit of the engine: q3_engine.h says which holds what)
//
// The mirror of the output stage (q3_pcm_stage.hip) on the input side. What q3_wav_read and q3_resample do on the host for a
// reference clip — decode the samples, average the channels, resample to the encoders' 24 kHz — k_intake does on the device, and
// the result stays there for both encoders (q3_spk_encode_ref, q3_mimi_encode_ref).
//
// Decode: q3_wav_read's rule. An integer sample iv becomes (float)iv / 2^(bits-1) (8-bit PCM is unsigned on disk, 24-bit is
// sign-extended, 32-bit uses the positive scale), f32 is taken as it is, a G.711 byte is expanded to int16 first. Downmix: the
// channels summed in ascending order in f32, then one correctly rounded f32 division by (float)channels.
// Resample: q3_resample's filter as the table taps_of (q3_pcm_stage.hip) builds for L / M = 24000 / sr_in in lowest terms; output i
// is the dot product of row (i M) mod L with inputs c - 63 .. c + 64, c = floor(i M / L), zeros outside the clip, in k_pcm_stage's
// fixed order. Phases are 64-bit integers. At 24 kHz there is no filter: the decoded, downmixed samples as they are.
//
// One launch serves every clip of a call: grid (tile of 256 outputs, clip), a descriptor per clip. A block decodes and downmixes
// its tile's window of the mono stream into LDS as it stages it — consecutive lanes take consecutive frames — and computes one
// output per thread. Descriptors, tables and the clips' raw bytes go up in one transfer, each clip's frame 0 at a 16-byte
// boundary of it, so a sample of 2 or 4 bytes lies at a multiple of its size and is read with a load of that size; 24-bit samples
// are read byte by byte. The staging block goes back to the device-memory cache when the call returns; the objects keep their
// 24 kHz samples and nothing else.
#include "q3_engine.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

struct q3_ref_audio {
    float* dev = nullptr; int64_t n = 0; int device = 0;        // the 24 kHz samples
    uint32_t sr_in = 0; int format = 0, channels = 0;           // what the clip was
};

namespace {
constexpr int IN_TILE = 256;                       // outputs per block, one per thread
constexpr int IN_TAPS = 128, IN_HALF = 64;
constexpr uint32_t IN_RATE_OUT = 24000, IN_RATE_MIN = 4000, IN_RATE_MAX = 96000;
constexpr int IN_MAX_L = 320, IN_MAX_CH = 8, IN_MAX_CLIPS = 64;
constexpr long long IN_MAX_OUT = (long long)IN_RATE_OUT * 120;
// the window of a tile: floor(255 * M / L) + 1 + 128 inputs, M / L <= 4 (sr_in <= 96000)
constexpr int IN_WIN = (IN_TILE - 1) * (int)(IN_RATE_MAX / IN_RATE_OUT) + 1 + IN_TAPS;

// one clip of a launch (device-visible, 8-byte aligned)
struct InDesc {
    const uint8_t* raw; const float* taps; float* out;      // raw: frame 0 at a 16-byte boundary; taps: null at 24 kHz
    long long n, n_out;
    int fmt, ch, L, M;
};

// ITU-T G.711 expansion to int16 (q3_g711_to_pcm16's)
__device__ inline int ulaw_to_pcm16(int b) {
    const int u = ~b & 0xFF;
    const int t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4);
    return (u & 0x80) ? 0x84 - t : t - 0x84;
}
__device__ inline int alaw_to_pcm16(int b) {
    const int a = b ^ 0x55, seg = (a & 0x70) >> 4;
    int t = (a & 0x0F) << 4;
    t = seg == 0 ? t + 8 : seg == 1 ? t + 0x108 : (t + 0x108) << (seg - 1);
    return (a & 0x80) ? t : -t;
}

// sample k (frame * ch + channel) of a clip. The scales are powers of two, so the product is the quotient q3_wav_read takes.
__device__ inline float sample_at(const uint8_t* __restrict__ raw, int fmt, size_t k) {
    switch (fmt) {
        case Q3_SRC_U8: return (float)((int)raw[k] - 128) * 0x1p-7f;
        case Q3_SRC_S16: return (float)(int)(int16_t)((const uint16_t*)raw)[k] * 0x1p-15f;
        case Q3_SRC_S24: {
            const uint8_t* s = raw + 3 * k;
            const int iv = (int)((uint32_t)s[0] << 8 | (uint32_t)s[1] << 16 | (uint32_t)s[2] << 24) >> 8;
            return (float)iv * 0x1p-23f;
        }
        case Q3_SRC_S32: return (float)(int)((const uint32_t*)raw)[k] * 0x1p-31f;
        case Q3_SRC_F32: return __uint_as_float(((const uint32_t*)raw)[k]);
        case Q3_SRC_ULAW: return (float)ulaw_to_pcm16(raw[k]) * 0x1p-15f;
        default: return (float)alaw_to_pcm16(raw[k]) * 0x1p-15f;
    }
}
// frame g of the mono stream: the channels summed in ascending order, then a true division (q3_wav_read's)
__device__ inline float mono_at(const InDesc& d, long long g) {
    const size_t k0 = (size_t)g * (size_t)d.ch;
    float acc = 0.0f;
    for (int c = 0; c < d.ch; ++c) acc += sample_at(d.raw, d.fmt, k0 + (size_t)c);
    return d.ch > 1 ? __fdiv_rn(acc, (float)d.ch) : acc;
}

__global__ __launch_bounds__(IN_TILE) void k_intake(const InDesc* __restrict__ descs) {
    __shared__ float win[IN_WIN];
    const InDesc d = descs[blockIdx.y];
    const int tid = threadIdx.x;
    const long long o0 = (long long)blockIdx.x * IN_TILE;
    if (o0 >= d.n_out) return;                                   // (uniform over the block)
    const int cnt = (int)min((long long)IN_TILE, d.n_out - o0);
    float y;
    if (!d.taps) {                                               // 24 kHz: the samples as they are
        if (tid >= cnt) return;
        y = mono_at(d, o0 + tid);
    } else {
        // integer phase arithmetic: q = i * M, c = q / L, p = q % L; within the tile relative to its first output
        const long long q0 = o0 * (long long)d.M, c0 = q0 / d.L;
        const int p0 = (int)(q0 - c0 * d.L);
        const long long w0 = c0 - (IN_HALF - 1);                 // first input of the window
        const int wlen = (p0 + (cnt - 1) * d.M) / d.L + IN_TAPS; // <= IN_WIN: M <= 4 L
        for (int k = tid; k < wlen; k += IN_TILE) {
            const long long g = w0 + k;
            win[k] = (g >= 0 && g < d.n) ? mono_at(d, g) : 0.0f;
        }
        __syncthreads();
        if (tid >= cnt) return;
        const int q = p0 + tid * d.M, dc = q / d.L, p = q - dc * d.L;
        const float4* h = (const float4*)(d.taps + (size_t)p * IN_TAPS);
        const float* x = win + dc;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;        // k_pcm_stage's order: four interleaved sums, joined pairwise
#pragma unroll 8
        for (int j = 0; j < IN_TAPS / 4; ++j) {
            const float4 t = h[j];
            a0 = fmaf(t.x, x[4 * j], a0); a1 = fmaf(t.y, x[4 * j + 1], a1);
            a2 = fmaf(t.z, x[4 * j + 2], a2); a3 = fmaf(t.w, x[4 * j + 3], a3);
        }
        y = (a0 + a1) + (a2 + a3);
    }
    d.out[o0 + tid] = y;
}

// ---- the mark's detector: q3_mark_detect's definition on the clip where the intake left it ----
constexpr int MD_P = 4096, MD_H = 240;                           // the carrier's period; hop (10 ms)
constexpr int MD_THREADS = 256;
constexpr int MD_FOLD_WGS = MD_P / MD_THREADS;                   // 16: a tile of 256 positions of the period each
constexpr int MD_SHIFTS = 16, MD_CORR_WGS = MD_P / MD_SHIFTS;    // 16 shifts a workgroup, 256 workgroups: one per CU

// F[m] = sum over k of z[k P + m] / max(r_h, 1e-4), r_h the root mean square of the sample's own hop, in ascending k. Per k a
// workgroup's 256 samples lie in at most three hops: waves 0..2 take one each — lane q adds the squares of samples q, q + 64, ... of
// the hop in ascending order (a non-finite one as 0, zeros behind the clip), the fold is the wave reduction d = 32 .. 1 — and post the
// divisor; then every thread adds its sample's quotient. Every sum has one fixed order.
// Bounds: z is read at indices below n alone; rh at (k P + m) / 240 - (k P + m0) / 240 <= (m0 + 255) / 240 - m0 / 240 <= 2.
__global__ __launch_bounds__(MD_THREADS) void k_mark_fold(const float* __restrict__ z, long long n, float* __restrict__ F) {
    __shared__ float rh[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * MD_THREADS;
    float acc = 0.0f;
    for (long long base = m0; base < n; base += MD_P) {          // (uniform over the block)
        const long long h_lo = base / MD_H;
        const long long h = h_lo + wave;
        if (wave < 3 && h * MD_H < n) {
            float part = 0.0f;
            for (int j = lane; j < MD_H; j += 64) {
                const long long i = h * MD_H + j;
                float v = i < n ? z[i] : 0.0f;
                v = __builtin_isfinite(v) ? v : 0.0f;
                part = q3::add_rn(part, q3::mul_rn(v, v));
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) part = q3::add_rn(part, __shfl_down(part, o));
            if (lane == 0) rh[wave] = fmaxf(sqrtf(q3::mul_rn(part, (float)(1.0 / 240.0))), 1e-4f);
        }
        __syncthreads();
        const long long i = base + tid;
        if (i < n) {
            float v = z[i];
            v = __builtin_isfinite(v) ? v : 0.0f;
            acc = q3::add_rn(acc, __fdiv_rn(v, rh[(int)(i / MD_H - h_lo)]));
        }
        __syncthreads();                                         // (rh is written again)
    }
    F[m0 + tid] = acc;
}

// rho[d] = sum over m of F[m] c[(m + d) mod P]: a workgroup stages F and the carrier in LDS (32 KB) and takes 16 consecutive
// shifts; thread (s, t) = (tid >> 4, tid & 15) sums m = t, t + 16, ... of shift d0 + s in four interleaved sums, joined pairwise, and
// the 16 threads of a shift meet by four butterfly steps: one fixed order per shift. The 64 lanes of a wave read F at 16 consecutive
// words (each by four lanes: a broadcast) and the carrier at 19 consecutive words: no pass meets a bank twice.
__global__ __launch_bounds__(MD_THREADS) void k_mark_corr(const float* __restrict__ F, const float* __restrict__ c, float* __restrict__ rho) {
    __shared__ float Fs[MD_P], cs[MD_P];
    const int tid = threadIdx.x, t = tid & 15, d = blockIdx.x * MD_SHIFTS + (tid >> 4);
    for (int i = tid; i < MD_P; i += MD_THREADS) { Fs[i] = F[i]; cs[i] = c[i]; }
    __syncthreads();
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll 4
    for (int m = t; m < MD_P; m += 64) {
        a0 = fmaf(Fs[m], cs[(m + d) & (MD_P - 1)], a0); a1 = fmaf(Fs[m + 16], cs[(m + 16 + d) & (MD_P - 1)], a1);
        a2 = fmaf(Fs[m + 32], cs[(m + 32 + d) & (MD_P - 1)], a2); a3 = fmaf(Fs[m + 48], cs[(m + 48 + d) & (MD_P - 1)], a3);
    }
    float a = q3::add_rn(q3::add_rn(a0, a1), q3::add_rn(a2, a3));
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) a = q3::add_rn(a, __shfl_xor(a, o));
    if (t == 0) rho[d] = a;
}

struct InRate { int L = 1, M = 1; };
bool in_rate_of(uint32_t sr, InRate* r) {
    if (sr < IN_RATE_MIN || sr > IN_RATE_MAX) return false;
    uint32_t a = sr, b = IN_RATE_OUT;
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    if (IN_RATE_OUT / a > (uint32_t)IN_MAX_L) return false;
    r->L = (int)(IN_RATE_OUT / a); r->M = (int)(sr / a);
    return true;
}
q3_status in_rate_checked(const char* who, uint32_t sr, InRate* r) {
    if (in_rate_of(sr, r)) return Q3_OK;
    return set_err(Q3_UNSUPPORTED, "%s: sample rate %u not supported on the device (4000..96000 Hz with 24000 / gcd(sr, 24000) <= %d: 8000, 11025, "
                                   "12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000, ...); q3_resample takes any rate on the host", who, sr, IN_MAX_L);
}
// q3_resample's n_out
long long in_count(uint32_t sr, long long n) {
    return sr == IN_RATE_OUT ? n : (long long)llround((double)n * ((double)IN_RATE_OUT / (double)sr));
}
size_t in_sample_bytes(int fmt) { return fmt == Q3_SRC_S16 ? 2 : fmt == Q3_SRC_S24 ? 3 : (fmt == Q3_SRC_S32 || fmt == Q3_SRC_F32) ? 4 : 1; }
bool in_fmt_ok(int fmt) { return fmt >= Q3_SRC_U8 && fmt <= Q3_SRC_ALAW; }

// the tables, per rate: built once, kept on the host (at most eight rates; the oldest goes)
struct TapCache {
    std::mutex mu;
    std::vector<std::pair<uint32_t, std::shared_ptr<const std::vector<float>>>> rows;
    std::shared_ptr<const std::vector<float>> get(uint32_t sr, const InRate& r) {
        std::lock_guard<std::mutex> g(mu);
        for (auto& kv : rows) if (kv.first == sr) return kv.second;
        auto t = std::make_shared<std::vector<float>>();
        resampler_taps(r.L, r.M, *t);
        if (rows.size() >= 8) rows.erase(rows.begin());
        rows.emplace_back(sr, t);
        return t;
    }
};
TapCache& tap_cache() { static TapCache* c = new TapCache(); return *c; }

// the intake's own stream, one per device, created by the first call there
struct InStreams { std::mutex mu; std::unordered_map<int, hipStream_t> st; };
q3_status in_stream(int device, hipStream_t* out) {
    static InStreams* s = new InStreams();
    std::lock_guard<std::mutex> g(s->mu);
    auto it = s->st.find(device);
    if (it != s->st.end()) { *out = it->second; return Q3_OK; }
    q3_relax_capture_mode();
    hipStream_t st = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e != hipSuccess) return set_err(Q3_HIP_ERROR, "hipStreamCreateWithFlags: %s", hipGetErrorString(e));
    s->st.emplace(device, st);
    *out = st;
    return Q3_OK;
}

q3_status clip_checked(const char* who, int i, const q3_clip& c, InRate* r, long long* n_out) {
    if (!c.data) return set_err(Q3_INVALID_ARG, "%s: clip %d: null data", who, i);
    if (c.frames < 1) return set_err(Q3_INVALID_ARG, "%s: clip %d: %lld frames (at least 1)", who, i, (long long)c.frames);
    if (c.channels < 1 || c.channels > IN_MAX_CH) return set_err(Q3_INVALID_ARG, "%s: clip %d: %d channels (1 .. %d)", who, i, c.channels, IN_MAX_CH);
    if (!in_fmt_ok(c.format)) return set_err(Q3_INVALID_ARG, "%s: clip %d: format %d is none of Q3_SRC_U8 .. Q3_SRC_ALAW", who, i, c.format);
    Q3C(in_rate_checked(who, c.sample_rate, r));
    if (c.frames > IN_MAX_OUT * 4) return set_err(Q3_INVALID_ARG, "%s: clip %d: reference audio of %lld frames unsupported (1 .. 120 s)", who, i, (long long)c.frames);
    *n_out = in_count(c.sample_rate, c.frames);
    if (*n_out < 1 || *n_out > IN_MAX_OUT)
        return set_err(Q3_INVALID_ARG, "%s: clip %d: reference audio of %lld samples at 24 kHz unsupported (1 .. 120 s)", who, i, *n_out);
    return Q3_OK;
}
size_t up16z(size_t v) { return (v + 15) & ~(size_t)15; }

// descriptors | tables | raw bytes in one block and one transfer, the launch, a wait. objs[i] has its samples allocated.
q3_status intake_run(int device, int n, const q3_clip* clips, const std::vector<InRate>& rates, std::vector<q3_ref_audio*>& objs, char** stage_dev) {
    // layout of the staging block (every part at a multiple of 16 bytes)
    size_t bytes = up16z((size_t)n * sizeof(InDesc));
    std::vector<std::shared_ptr<const std::vector<float>>> tabs((size_t)n);
    std::vector<size_t> tab_off((size_t)n, 0), raw_off((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        if (clips[i].sample_rate == IN_RATE_OUT) continue;
        int same = -1;
        for (int j = 0; j < i && same < 0; ++j) if (clips[j].sample_rate == clips[i].sample_rate) same = j;
        if (same >= 0) { tabs[(size_t)i] = tabs[(size_t)same]; tab_off[(size_t)i] = tab_off[(size_t)same]; continue; }
        tabs[(size_t)i] = tap_cache().get(clips[i].sample_rate, rates[(size_t)i]);
        tab_off[(size_t)i] = bytes; bytes += up16z(tabs[(size_t)i]->size() * 4);
    }
    for (int i = 0; i < n; ++i) {
        raw_off[(size_t)i] = bytes;
        bytes += up16z((size_t)clips[i].frames * (size_t)clips[i].channels * in_sample_bytes(clips[i].format));
    }
    HIPC(dev_malloc((void**)stage_dev, bytes));
    char* dev = *stage_dev;
    std::vector<char> host(bytes);
    InDesc* desc = (InDesc*)host.data();
    long long max_out = 1;
    for (int i = 0; i < n; ++i) {
        const q3_clip& c = clips[i];
        InDesc& d = desc[i];
        d.raw = (const uint8_t*)(dev + raw_off[(size_t)i]);
        d.taps = tabs[(size_t)i] ? (const float*)(dev + tab_off[(size_t)i]) : nullptr;
        d.out = objs[(size_t)i]->dev;
        d.n = c.frames; d.n_out = objs[(size_t)i]->n;
        d.fmt = c.format; d.ch = c.channels; d.L = rates[(size_t)i].L; d.M = rates[(size_t)i].M;
        if (tabs[(size_t)i]) memcpy(host.data() + tab_off[(size_t)i], tabs[(size_t)i]->data(), tabs[(size_t)i]->size() * 4);
        memcpy(host.data() + raw_off[(size_t)i], c.data, (size_t)c.frames * (size_t)c.channels * in_sample_bytes(c.format));
        max_out = std::max(max_out, (long long)d.n_out);
    }
    hipStream_t st = nullptr;
    Q3C(in_stream(device, &st));
    HIPC(hipMemcpyAsync(dev, host.data(), bytes, hipMemcpyHostToDevice, st));
    const unsigned tiles = (unsigned)((max_out + IN_TILE - 1) / IN_TILE);
    hipLaunchKernelGGL(k_intake, dim3(tiles, (unsigned)n), dim3(IN_TILE), 0, st, (const InDesc*)dev);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(st));
    return Q3_OK;
}
}  // namespace

extern "C" const float* q3i_ref_audio_dev(const q3_ref_audio* r, int64_t* n, int* device) {
    *n = r->n; *device = r->device;
    return r->dev;
}

extern "C" q3_status q3_intake_taps(uint32_t sample_rate, float* taps_host, size_t cap_floats, int* L, int* M) {
    InRate r;
    Q3C(in_rate_checked("q3_intake_taps", sample_rate, &r));
    if (L) *L = r.L;
    if (M) *M = r.M;
    if (!taps_host) return Q3_OK;                              // L / M query
    if (cap_floats < (size_t)r.L * IN_TAPS) return set_err(Q3_INVALID_ARG, "q3_intake_taps: buffer too small (%zu floats needed)", (size_t)r.L * IN_TAPS);
    std::vector<float> t;
    resampler_taps(r.L, r.M, t);
    memcpy(taps_host, t.data(), t.size() * 4);
    return Q3_OK;
}

extern "C" q3_status q3_intake_count(uint32_t sample_rate, int64_t n_in, int64_t* n_out) {
    InRate r;
    Q3C(in_rate_checked("q3_intake_count", sample_rate, &r));
    if (!n_out || n_in < 0) return set_err(Q3_INVALID_ARG, "q3_intake_count: bad argument");
    *n_out = in_count(sample_rate, n_in);
    return Q3_OK;
}

extern "C" q3_status q3_ref_audio_create_many(int device, int n, const q3_clip* clips, q3_ref_audio** out) {
    const char* who = "q3_ref_audio_create_many";
    if (!clips || !out) return set_err(Q3_INVALID_ARG, "%s: null argument", who);
    if (n < 1 || n > IN_MAX_CLIPS) return set_err(Q3_INVALID_ARG, "%s: %d clips (1 .. %d)", who, n, IN_MAX_CLIPS);
    if (device < 0) return set_err(Q3_INVALID_ARG, "%s: device %d", who, device);
    std::vector<InRate> rates((size_t)n);
    std::vector<long long> n_out((size_t)n);
    for (int i = 0; i < n; ++i) Q3C(clip_checked(who, i, clips[i], &rates[(size_t)i], &n_out[(size_t)i]));
    HIPC(hipSetDevice(device));
    std::vector<q3_ref_audio*> objs;
    char* stage = nullptr;
    q3_status st = Q3_OK;
    for (int i = 0; i < n && st == Q3_OK; ++i) {
        q3_ref_audio* r = new q3_ref_audio();
        r->n = n_out[(size_t)i]; r->device = device; r->sr_in = clips[i].sample_rate; r->format = clips[i].format; r->channels = clips[i].channels;
        objs.push_back(r);
        q3_relax_capture_mode();
        const hipError_t e = dev_malloc((void**)&r->dev, (size_t)r->n * 4);
        if (e != hipSuccess) st = set_err(Q3_HIP_ERROR, "%s: %lld samples on the device: %s", who, (long long)r->n, hipGetErrorString(e));
    }
    if (st == Q3_OK) st = intake_run(device, n, clips, rates, objs, &stage);
    dev_free(stage);                                             // (the call has waited for the launch)
    if (st != Q3_OK) { for (q3_ref_audio* r : objs) q3_ref_audio_free(r); return st; }
    for (int i = 0; i < n; ++i) out[i] = objs[(size_t)i];
    return Q3_OK;
}

extern "C" q3_status q3_ref_audio_create(int device, const q3_clip* clip, q3_ref_audio** out) {
    if (!clip || !out) return set_err(Q3_INVALID_ARG, "q3_ref_audio_create: null argument");
    return q3_ref_audio_create_many(device, 1, clip, out);
}

extern "C" q3_status q3_ref_audio_from_wav(const char* path, int device, q3_ref_audio** out) {
    if (!path || !out) return set_err(Q3_INVALID_ARG, "q3_ref_audio_from_wav: null argument");
    q3_wav_desc w;
    Q3C(q3_wav_info(path, &w));
    if (w.frames < 1) return set_err(Q3_INVALID_ARG, "q3_ref_audio_from_wav: %s holds no samples", path);
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return set_err(Q3_IO, "Failed to open WAV file: %s", path);
    struct stat sb;
    if (fstat(fd, &sb) != 0 || (int64_t)sb.st_size < w.data_offset + w.data_bytes) { close(fd); return set_err(Q3_IO, "%s: changed while it was read", path); }
    void* m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return set_err(Q3_IO, "Failed to map WAV file: %s", path);
    q3_clip c;
    c.data = (const uint8_t*)m + w.data_offset; c.frames = w.frames; c.channels = w.channels; c.sample_rate = w.sample_rate; c.format = w.format;
    const q3_status st = q3_ref_audio_create_many(device, 1, &c, out);
    munmap(m, (size_t)sb.st_size);
    return st;
}

extern "C" q3_status q3_ref_audio_info(const q3_ref_audio* r, int64_t* n_samples, int* device, uint32_t* sr_in, int* format, int* channels) {
    if (!r) return set_err(Q3_INVALID_ARG, "q3_ref_audio_info: null handle");
    if (n_samples) *n_samples = r->n;
    if (device) *device = r->device;
    if (sr_in) *sr_in = r->sr_in;
    if (format) *format = r->format;
    if (channels) *channels = r->channels;
    return Q3_OK;
}

extern "C" q3_status q3_ref_audio_read(q3_ref_audio* r, float* host, int64_t cap, int64_t* n) {
    if (!r || !n) return set_err(Q3_INVALID_ARG, "q3_ref_audio_read: null argument");
    *n = r->n;
    if (!host) return Q3_OK;                                   // length query
    if (cap < r->n) return set_err(Q3_INVALID_ARG, "q3_ref_audio_read: buffer holds %lld samples, the object has %lld", (long long)cap, (long long)r->n);
    HIPC(hipSetDevice(r->device));
    hipStream_t st = nullptr;
    Q3C(in_stream(r->device, &st));
    HIPC(hipMemcpyAsync(host, r->dev, (size_t)r->n * 4, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return Q3_OK;
}

// The detector on the device: the carrier up, the fold, the 4096 x 4096 correlation, the 16 KB of rho back, a wait; the score and
// the offset from rho in f64 on the host (mark_score_f32). The scratch block goes back to the device-memory cache.
extern "C" q3_status q3_ref_audio_mark_score(q3_ref_audio* r, uint64_t key, double* score, int* offset) {
    const char* who = "q3_ref_audio_mark_score";
    if (!r || (!score && !offset)) return set_err(Q3_INVALID_ARG, "%s: null argument", who);
    if (key == 0) return set_err(Q3_INVALID_ARG, "%s: key 0 is off: there is no carrier", who);
    if (r->n < 2 * (int64_t)MD_P) return set_err(Q3_INVALID_ARG, "%s: clip of %lld samples (at least %d: two periods at 24 kHz)", who, (long long)r->n, 2 * MD_P);
    std::vector<float> host(2 * (size_t)MD_P);                   // the carrier up, rho back
    mark_carrier(key, host.data());
    HIPC(hipSetDevice(r->device));
    hipStream_t st = nullptr;
    Q3C(in_stream(r->device, &st));
    float* dev = nullptr;                                        // c | F | rho
    q3_relax_capture_mode();
    HIPC(dev_malloc((void**)&dev, 3 * (size_t)MD_P * 4));
    auto run = [&]() -> q3_status {
        HIPC(hipMemcpyAsync(dev, host.data(), (size_t)MD_P * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mark_fold, dim3(MD_FOLD_WGS), dim3(MD_THREADS), 0, st, (const float*)r->dev, (long long)r->n, dev + MD_P);
        HIPC(hipGetLastError());
        hipLaunchKernelGGL(k_mark_corr, dim3(MD_CORR_WGS), dim3(MD_THREADS), 0, st, (const float*)(dev + MD_P), (const float*)dev, dev + 2 * MD_P);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(host.data() + MD_P, dev + 2 * MD_P, (size_t)MD_P * 4, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        return Q3_OK;
    };
    const q3_status rs = run();
    dev_free(dev);
    Q3C(rs);
    return mark_score_f32(host.data() + MD_P, score, offset);
}

extern "C" void q3_ref_audio_free(q3_ref_audio* r) {
    if (!r) return;
    dev_free(r->dev);
    delete r;
}
