// q3_pcm_stage.hip — the output stage: 24 kHz f32 from the vocoder -> a requested sample rate, f32 or PCM16, per row
// (a unit of the engine: q3_engine.h says which holds what)
//
// The resampler is q3_resample's (q3_io.cpp): a 128-tap Blackman-Harris²-windowed sinc at 0.95 x the lower Nyquist, output i at
// input time i * M / L with L / M = sr_out / 24000 in lowest terms. What the host loop evaluates per output sample in f64 is a
// function of the phase p = (i * M) mod L alone, so it is tabulated once per rate: taps[L][128] (f64, rounded to f32), and output i
// is the dot product of row p with inputs c - 63 .. c + 64, c = floor(i * M / L): f32 products, accumulated in a fixed order.
//
// Streaming: a row emits output i once input c + 64 has arrived (and, with `last`, everything up to llround(n_in * sr_out / 24000)
// against zeros). The next output to emit then starts no earlier than 127 samples before the end of what has arrived, so a row
// keeps its last 128 input samples — two buffers, read one / write the other in the same launch, flipped when the push has
// succeeded: a push that fails or is refused leaves the row exactly where it was.
//
// One launch serves every row of a push: grid (output tile, row), a descriptor per row. A block stages its tile's input window
// (kept tail | new samples | zeros) in LDS and computes one output per thread; tile 0 of a row also writes the row's next tail.
#include "q3_engine.h"

namespace {
constexpr int PS_TILE = 256;                     // outputs per block, one per thread
constexpr int PS_TAPS = 128, PS_HALF = 64;
constexpr uint32_t PS_RATE_IN = 24000, PS_RATE_MIN = 4000, PS_RATE_MAX = 96000;
constexpr int PS_MAX_L = 320;
// the window of a tile: floor(255 * M / L) + 1 + 128 inputs, M / L <= 6 (sr_out >= 4000)
constexpr int PS_WIN = (PS_TILE - 1) * (int)(PS_RATE_IN / PS_RATE_MIN) + 1 + PS_TAPS;

// S16: q3_pcm16_from_f32's rule — clamp to [-1, 1], x 32767, truncate toward zero, NaN -> 0
__device__ inline int16_t pcm16_of(float x) {
    const float c = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
    const float s = c * 32767.0f;
    return s != s ? (int16_t)0 : (int16_t)(int)s;
}

__global__ __launch_bounds__(PS_TILE) void k_pcm_stage(const PsDesc* __restrict__ descs) {
    __shared__ float win[PS_WIN];
    const PsDesc d = descs[blockIdx.y];
    const int tid = threadIdx.x, o0 = blockIdx.x * PS_TILE;
    // sample g of the row's input stream: the kept tail below `base`, the new samples from there, zeros outside [0, end)
    auto in_at = [&](long long g) -> float {
        if (g >= d.base) { const long long k = g - d.base; return k < d.n_new ? d.src[k] : 0.0f; }
        const long long k = g - (d.base - PS_TAPS);
        return (k >= 0 && d.tail_in) ? d.tail_in[k] : 0.0f;
    };
    if (blockIdx.x == 0 && d.tail_out && tid < PS_TAPS) d.tail_out[tid] = in_at(d.base + d.n_new - PS_TAPS + tid);
    if (o0 >= d.n_out) return;                                   // (uniform over the block)
    const int cnt = min(PS_TILE, d.n_out - o0);
    float y;
    if (!d.taps) {                                               // 24 kHz: the samples as they are
        if (tid >= cnt) return;
        y = d.src[o0 + tid];
    } else {
        // integer phase arithmetic: q = i * M, c = q / L, p = q % L; within the tile relative to its first output
        const long long q0 = (d.i0 + o0) * (long long)d.M, c0 = q0 / d.L;
        const int p0 = (int)(q0 - c0 * d.L);
        const long long w0 = c0 - (PS_HALF - 1);                 // first input of the window
        const int wlen = (p0 + (cnt - 1) * d.M) / d.L + PS_TAPS;
        for (int k = tid; k < wlen; k += PS_TILE) win[k] = in_at(w0 + k);
        __syncthreads();
        if (tid >= cnt) return;
        const int q = p0 + tid * d.M, dc = q / d.L, p = q - dc * d.L;
        const float4* h = (const float4*)(d.taps + (size_t)p * PS_TAPS);
        const float* x = win + dc;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;        // four interleaved sums, joined pairwise: one fixed order per output
#pragma unroll 8
        for (int j = 0; j < PS_TAPS / 4; ++j) {
            const float4 t = h[j];
            a0 = fmaf(t.x, x[4 * j], a0); a1 = fmaf(t.y, x[4 * j + 1], a1);
            a2 = fmaf(t.z, x[4 * j + 2], a2); a3 = fmaf(t.w, x[4 * j + 3], a3);
        }
        y = (a0 + a1) + (a2 + a3);
    }
    if (d.fmt == Q3_PCM_S16) ((int16_t*)d.out)[o0 + tid] = pcm16_of(y);
    else ((float*)d.out)[o0 + tid] = y;
}

struct Rate { int L = 1, M = 1; };
bool rate_of(uint32_t sr, Rate* r) {
    if (sr < PS_RATE_MIN || sr > PS_RATE_MAX) return false;
    uint32_t a = sr, b = PS_RATE_IN;
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    if (sr / a > (uint32_t)PS_MAX_L) return false;
    r->L = (int)(sr / a); r->M = (int)(PS_RATE_IN / a);
    return true;
}
q3_status rate_checked(const char* who, uint32_t sr, Rate* r) {
    if (rate_of(sr, r)) return Q3_OK;
    return set_err(Q3_UNSUPPORTED, "%s: sample rate %u not supported (4000..96000 Hz with sr / gcd(sr, 24000) <= %d: 8000, 11025, 12000, 16000, 22050, "
                                   "24000, 32000, 44100, 48000, ...)", who, sr, PS_MAX_L);
}
// the table of q3_resample's filter: row p = the weights of inputs c - 63 .. c + 64 for an output at input time c + p / L
void taps_of(const Rate& r, std::vector<float>& out) {
    const double ratio = (double)r.L / (double)r.M;
    const double fc = 0.95 * (ratio < 1.0 ? ratio : 1.0);
    const double a0 = 0.35875, a1 = 0.48829, a2 = 0.14128, a3 = 0.01168, PI = 3.14159265358979323846;
    out.assign((size_t)r.L * PS_TAPS, 0.0f);
    for (int p = 0; p < r.L; ++p)
        for (int j = 0; j < PS_TAPS; ++j) {
            const double u = (double)p / (double)r.L - (double)(j - (PS_HALF - 1)), v = u / (double)PS_HALF;
            if (v <= -1.0 || v >= 1.0) continue;
            double w = a0 + a1 * cos(PI * v) + a2 * cos(2.0 * PI * v) + a3 * cos(3.0 * PI * v);
            w *= w;
            const double xs = PI * fc * u;
            const double sinc = fabs(xs) < 1e-12 ? 1.0 : sin(xs) / xs;
            out[(size_t)p * PS_TAPS + j] = (float)(fc * sinc * w);
        }
}
// outputs a row has emitted once n_in input samples have arrived (every i with floor(i * M / L) + 64 <= n_in - 1), and all of
// them once the input has ended (q3_resample's n_out)
long long emitted(uint32_t sr, const Rate& r, long long n_in, bool ended) {
    if (sr == PS_RATE_IN) return n_in;
    if (ended) return (long long)llround((double)n_in * ((double)sr / (double)PS_RATE_IN));
    return n_in > PS_HALF ? ((n_in - PS_HALF) * r.L + r.M - 1) / r.M : 0;
}
size_t fmt_bytes(int fmt) { return fmt == Q3_PCM_S16 ? 2 : 4; }
}  // namespace

struct PsRow {
    uint32_t sr = PS_RATE_IN; int fmt = Q3_PCM_F32; Rate r; const float* taps = nullptr;
    long long n_in = 0, n_out = 0;            // input samples consumed, output samples emitted
    int cur = 0; bool fresh = true;           // which of the two tail buffers holds the last 128 inputs; fresh: none yet (zeros)
    bool ended = false;                       // flushed by a push with `last`: restarted by set / reset only
};
struct q3_pcm_stage {
    int device = 0, R = 0; size_t max_push = 0;
    hipStream_t st = nullptr;
    std::vector<PsRow> rows;
    std::unordered_map<uint32_t, float*> taps;                 // per rate, on the device
    float* tails = nullptr;                                    // [R][2][128]
    char *out_dev = nullptr, *out_host = nullptr; size_t out_cap = 0;      // converted samples of a push: device, pinned host
    char *in_dev = nullptr, *in_host = nullptr; size_t in_cap = 0;         // q3_pcm_stage_push: descriptors | the rows' new samples
};

extern "C" q3_status q3_pcm_stage_taps(uint32_t sample_rate, float* taps_host, size_t cap_floats, int* L, int* M) {
    Rate r;
    Q3C(rate_checked("q3_pcm_stage_taps", sample_rate, &r));
    if (L) *L = r.L;
    if (M) *M = r.M;
    if (!taps_host) return Q3_OK;                              // L / M query
    if (cap_floats < (size_t)r.L * PS_TAPS) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_taps: buffer too small (%zu floats needed)", (size_t)r.L * PS_TAPS);
    std::vector<float> t;
    taps_of(r, t);
    memcpy(taps_host, t.data(), t.size() * 4);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_bound(uint32_t sample_rate, size_t n_in, size_t* n_out_max) {
    Rate r;
    Q3C(rate_checked("q3_pcm_stage_bound", sample_rate, &r));
    if (!n_out_max) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_bound: null argument");
    // the most one push can return: its own samples and, with `last`, the 64 held back: llround(N L / M) - ceil((N - n - 64) L / M)
    *n_out_max = sample_rate == PS_RATE_IN ? n_in : (size_t)(((long long)(n_in + PS_HALF) * r.L + r.M - 1) / r.M + 1);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_create(int device, int rows, size_t max_push_samples, q3_pcm_stage** out) {
    if (!out || rows < 1 || max_push_samples < 1) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_create: rows and max_push_samples must be positive");
    if (device < 0) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_create: no device (a manifest-only model has none): the stage runs on the GPU");
    if (max_push_samples > ((size_t)1 << 28)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_create: max_push_samples above 2^28");
    HIPC(hipSetDevice(device));
    std::unique_ptr<q3_pcm_stage> ps(new q3_pcm_stage());
    ps->device = device; ps->R = rows; ps->max_push = max_push_samples; ps->rows.resize((size_t)rows);
    auto fail = [&](q3_status s) { q3_pcm_stage_free(ps.release()); return s; };
    if (dev_malloc((void**)&ps->tails, (size_t)rows * 2 * PS_TAPS * 4) != hipSuccess) { (void)hipGetLastError(); return fail(set_err(Q3_OOM, "q3_pcm_stage_create: %d rows", rows)); }
    *out = ps.release();
    return Q3_OK;
}

extern "C" void q3_pcm_stage_free(q3_pcm_stage* ps) {
    if (!ps) return;
    (void)hipSetDevice(ps->device);
    if (ps->st) (void)hipStreamSynchronize(ps->st);
    for (auto& kv : ps->taps) dev_free(kv.second);
    dev_free(ps->tails); dev_free(ps->out_dev); dev_free(ps->in_dev);
    if (ps->out_host) (void)hipHostFree(ps->out_host);
    if (ps->in_host) (void)hipHostFree(ps->in_host);
    if (ps->st) (void)hipStreamDestroy(ps->st);
    delete ps;
}

int pcm_stage_rows(const q3_pcm_stage* ps) { return ps->R; }
size_t pcm_stage_sample_bytes(const q3_pcm_stage* ps, int row) { return fmt_bytes(ps->rows[(size_t)row].fmt); }
void pcm_stage_reset(q3_pcm_stage* ps, int row) {
    PsRow& r = ps->rows[(size_t)row];
    r.n_in = r.n_out = 0; r.cur = 0; r.fresh = true; r.ended = false;
}

extern "C" q3_status q3_pcm_stage_reset(q3_pcm_stage* ps, int row) {
    if (!ps || row < 0 || row >= ps->R) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_reset: bad row");
    pcm_stage_reset(ps, row);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_set(q3_pcm_stage* ps, int row, uint32_t sample_rate, int format) {
    if (!ps || row < 0 || row >= ps->R) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_set: bad row");
    if (format != Q3_PCM_F32 && format != Q3_PCM_S16) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_set: format must be Q3_PCM_F32 (0) or Q3_PCM_S16 (1)");
    Rate r;
    Q3C(rate_checked("q3_pcm_stage_set", sample_rate, &r));      // (before the device is touched)
    const float* taps = nullptr;
    if (sample_rate != PS_RATE_IN) {
        auto it = ps->taps.find(sample_rate);
        if (it == ps->taps.end()) {
            HIPC(hipSetDevice(ps->device));
            std::vector<float> t;
            taps_of(r, t);
            float* d = nullptr;
            if (dev_malloc((void**)&d, t.size() * 4) != hipSuccess) { (void)hipGetLastError(); return set_err(Q3_OOM, "q3_pcm_stage_set: tap table of %u Hz", sample_rate); }
            const hipError_t e = q3_hipMemcpy(d, t.data(), t.size() * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) { dev_free(d); return set_err(Q3_HIP_ERROR, "q3_pcm_stage_set: tap upload: %s", hipGetErrorString(e)); }
            it = ps->taps.emplace(sample_rate, d).first;
        }
        taps = it->second;
    }
    PsRow& pr = ps->rows[(size_t)row];
    pr.sr = sample_rate; pr.fmt = format; pr.r = r; pr.taps = taps;
    pcm_stage_reset(ps, row);
    return Q3_OK;
}

// Checks a push (every row at most once and in range — the entry points' business —, n within max_push_samples, no samples for a
// row that was flushed), lays the rows' outputs out in the staging buffer (16-byte aligned each) and writes the descriptors.
// Changes no row. The staging buffers may be reallocated: no push is in flight (each ends with a wait).
q3_status pcm_stage_plan(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, PsPlan& plan) {
    plan.desc.clear(); plan.off.assign(segs.size(), 0); plan.count.assign(segs.size(), 0); plan.bytes = 0; plan.max_tiles = 1;
    for (size_t i = 0; i < segs.size(); ++i) {
        const PsSeg& sg = segs[i]; const PsRow& r = ps->rows[(size_t)sg.row];
        if (sg.n > ps->max_push) return set_err(Q3_INVALID_ARG, "pcm stage: %zu samples for row %d, the stage takes %zu per push", sg.n, sg.row, ps->max_push);
        if (r.ended && sg.n > 0) return set_err(Q3_INVALID_ARG, "pcm stage: row %d was flushed (last): q3_pcm_stage_reset or _set restarts it", sg.row);
        if (r.ended || (sg.n == 0 && !sg.last)) continue;
        const long long total = emitted(r.sr, r.r, r.n_in + (long long)sg.n, sg.last != 0);
        plan.count[i] = (size_t)std::max<long long>(0, total - r.n_out);
        plan.off[i] = plan.bytes;
        plan.bytes = (plan.bytes + plan.count[i] * fmt_bytes(r.fmt) + 15) & ~(size_t)15;
    }
    if (plan.bytes > ps->out_cap) {
        HIPC(hipSetDevice(ps->device));
        dev_free(ps->out_dev); ps->out_dev = nullptr;
        if (ps->out_host) { (void)hipHostFree(ps->out_host); ps->out_host = nullptr; }
        ps->out_cap = 0;
        HIPC(dev_malloc((void**)&ps->out_dev, plan.bytes * 2));
        HIPC(hipHostMalloc((void**)&ps->out_host, plan.bytes * 2, hipHostMallocDefault));
        ps->out_cap = plan.bytes * 2;
    }
    for (size_t i = 0; i < segs.size(); ++i) {
        const PsSeg& sg = segs[i]; const PsRow& r = ps->rows[(size_t)sg.row];
        if (r.ended || (sg.n == 0 && !sg.last)) continue;
        float* tails = ps->tails + (size_t)sg.row * 2 * PS_TAPS;
        PsDesc d{};
        d.src = sg.dev; d.n_new = (int)sg.n; d.n_out = (int)plan.count[i]; d.out = ps->out_dev + plan.off[i];
        d.base = r.n_in; d.i0 = r.n_out; d.L = r.r.L; d.M = r.r.M; d.fmt = r.fmt; d.taps = r.taps;
        if (r.taps) { d.tail_in = r.fresh ? nullptr : tails + (size_t)r.cur * PS_TAPS; d.tail_out = tails + (size_t)(r.cur ^ 1) * PS_TAPS; }
        plan.max_tiles = std::max(plan.max_tiles, (d.n_out + PS_TILE - 1) / PS_TILE);
        plan.desc.push_back(d);
    }
    return Q3_OK;
}
// the one launch of a push: descriptors (plan.desc, uploaded by the caller) on the device
hipError_t pcm_stage_launch(const PsDesc* desc_dev, const PsPlan& plan, hipStream_t st) {
    if (plan.desc.empty()) return hipSuccess;
    hipLaunchKernelGGL(k_pcm_stage, dim3((unsigned)plan.max_tiles, (unsigned)plan.desc.size()), dim3(PS_TILE), 0, st, desc_dev);
    return hipGetLastError();
}
// the push has succeeded (the caller waited for its stream): the rows move on
void pcm_stage_commit(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, const PsPlan& plan) {
    for (size_t i = 0; i < segs.size(); ++i) {
        const PsSeg& sg = segs[i]; PsRow& r = ps->rows[(size_t)sg.row];
        if (r.ended || (sg.n == 0 && !sg.last)) continue;
        r.n_in += (long long)sg.n; r.n_out += (long long)plan.count[i];
        if (r.taps) { r.cur ^= 1; r.fresh = false; }
        if (sg.last) r.ended = true;
    }
}
const char* pcm_stage_out_dev(const q3_pcm_stage* ps) { return ps->out_dev; }
char* pcm_stage_out_host(const q3_pcm_stage* ps) { return ps->out_host; }

// the stage's own stream, for pushes that do not come with one (created on the first: a stage behind a codec stream never needs it)
static q3_status own_stream(q3_pcm_stage* ps) {
    if (ps->st) return Q3_OK;
    q3_relax_capture_mode();
    const hipError_t e = hipStreamCreateWithFlags(&ps->st, hipStreamNonBlocking);
    if (e != hipSuccess) { ps->st = nullptr; return set_err(Q3_HIP_ERROR, "hipStreamCreateWithFlags: %s", hipGetErrorString(e)); }
    return Q3_OK;
}
static q3_status in_reserve(q3_pcm_stage* ps, size_t bytes) {
    if (bytes <= ps->in_cap) return Q3_OK;
    dev_free(ps->in_dev); ps->in_dev = nullptr;
    if (ps->in_host) { (void)hipHostFree(ps->in_host); ps->in_host = nullptr; }
    ps->in_cap = 0;
    HIPC(dev_malloc((void**)&ps->in_dev, bytes * 2));
    HIPC(hipHostMalloc((void**)&ps->in_host, bytes * 2, hipHostMallocDefault));
    ps->in_cap = bytes * 2;
    return Q3_OK;
}

// Segments already on the device (readable by work on `st` — the caller's own stream, or nullptr for the stage's): one descriptor
// upload, the launch, the copy of the converted bytes to the host, a wait. out_host[i] (may be null) receives plan.count[i]
// samples of segment i. The rows move on only when all of it has succeeded.
q3_status pcm_stage_push_dev(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, hipStream_t st, void* const* out_host, size_t* n_samples) {
    PsPlan plan;
    Q3C(pcm_stage_plan(ps, segs, plan));
    for (size_t i = 0; i < segs.size(); ++i) if (n_samples) n_samples[i] = plan.count[i];
    if (plan.desc.empty()) return Q3_OK;
    HIPC(hipSetDevice(ps->device));
    if (!st) { Q3C(own_stream(ps)); st = ps->st; }
    const size_t db = plan.desc.size() * sizeof(PsDesc);
    // (the input staging's front holds the descriptors; q3_pcm_stage_push has put the samples behind them already)
    if (ps->in_cap < db) Q3C(in_reserve(ps, db));
    memcpy(ps->in_host, plan.desc.data(), db);
    HIPC(hipMemcpyAsync(ps->in_dev, ps->in_host, db, hipMemcpyHostToDevice, st));
    HIPC(pcm_stage_launch((const PsDesc*)ps->in_dev, plan, st));
    if (plan.bytes > 0) HIPC(hipMemcpyAsync(ps->out_host, ps->out_dev, plan.bytes, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    for (size_t i = 0; i < segs.size(); ++i)
        if (out_host && out_host[i] && plan.count[i] > 0) memcpy(out_host[i], ps->out_host + plan.off[i], plan.count[i] * fmt_bytes(ps->rows[(size_t)segs[i].row].fmt));
    pcm_stage_commit(ps, segs, plan);
    return Q3_OK;
}

// row list of a push: in range, none twice (the checks of q3_codec_stream_push)
q3_status pcm_stage_check_rows(const q3_pcm_stage* ps, const char* who, int n_rows, const int* rows) {
    std::vector<char> seen((size_t)ps->R, 0);
    for (int i = 0; i < n_rows; ++i) {
        const int r = rows[i];
        if (r < 0 || r >= ps->R) return set_err(Q3_INVALID_ARG, "%s: stage row %d out of range (%d rows)", who, r, ps->R);
        if (seen[(size_t)r]) return set_err(Q3_INVALID_ARG, "%s: stage row %d listed twice", who, r);
        seen[(size_t)r] = 1;
    }
    return Q3_OK;
}
// what a push of n samples to `row` would return (the caller's cap check, before anything changes)
size_t pcm_stage_count(const q3_pcm_stage* ps, int row, size_t n, int last) {
    const PsRow& r = ps->rows[(size_t)row];
    if (r.ended || (n == 0 && !last)) return 0;
    return (size_t)std::max<long long>(0, emitted(r.sr, r.r, r.n_in + (long long)n, last != 0) - r.n_out);
}

extern "C" q3_status q3_pcm_stage_push(q3_pcm_stage* ps, int n_rows, const int* rows, const float* const* in_host, const size_t* n_in,
                                       const int* last, void* const* out_host, const size_t* cap_samples, size_t* n_samples) {
    if (!ps) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_push: null stage");
    if (n_rows < 0 || (n_rows > 0 && (!rows || !in_host || !n_in || !out_host || !cap_samples || !n_samples)))
        return set_err(Q3_INVALID_ARG, "q3_pcm_stage_push: null argument");
    Q3C(pcm_stage_check_rows(ps, "q3_pcm_stage_push", n_rows, rows));
    const size_t db = ((size_t)n_rows * sizeof(PsDesc) + 15) & ~(size_t)15;
    size_t total = 0;
    for (int i = 0; i < n_rows; ++i) {
        const int lst = last ? last[i] : 0;
        if (n_in[i] > ps->max_push) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_push: %zu samples for row %d, the stage takes %zu per push", n_in[i], rows[i], ps->max_push);
        if (n_in[i] > 0 && !in_host[i]) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_push: null input pointer for row %d", rows[i]);
        if (n_in[i] > 0 && ps->rows[(size_t)rows[i]].ended) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_push: row %d was flushed (last): q3_pcm_stage_reset or _set restarts it", rows[i]);
        const size_t cnt = pcm_stage_count(ps, rows[i], n_in[i], lst);
        if (cnt > cap_samples[i]) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_push: output buffer of row %d too small (%zu < %zu samples)", rows[i], cap_samples[i], cnt);
        if (cnt > 0 && !out_host[i]) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_push: null output pointer for row %d", rows[i]);
        total += (n_in[i] + 3) & ~(size_t)3;
    }
    if (n_rows == 0) return Q3_OK;
    HIPC(hipSetDevice(ps->device));
    Q3C(own_stream(ps));
    Q3C(in_reserve(ps, db + total * 4));
    std::vector<PsSeg> segs((size_t)n_rows);
    size_t off = db;
    for (int i = 0; i < n_rows; ++i) {
        if (n_in[i] > 0) memcpy(ps->in_host + off, in_host[i], n_in[i] * 4);
        segs[(size_t)i] = {rows[i], (const float*)(ps->in_dev + off), n_in[i], last ? last[i] : 0};
        off += ((n_in[i] + 3) & ~(size_t)3) * 4;
    }
    if (total > 0) HIPC(hipMemcpyAsync(ps->in_dev + db, ps->in_host + db, total * 4, hipMemcpyHostToDevice, ps->st));
    return pcm_stage_push_dev(ps, segs, ps->st, out_host, n_samples);
}
