// q3_pcm_stage.hip — the output stage: 24 kHz f32 from the vocoder -> per row a requested sample rate and format, through the
// steps the row has asked for. (A unit of the engine: q3_engine.h says which holds what.)
//
// A row's stream passes a chain of seven steps, front to back: silence -> stretcher -> pitch -> loudness -> mark -> level ->
// resampler / format. The last one every row has; each of the others is on for the rows that ask for it, and a row whose step is off is not
// touched by any of it: no launch, no buffer, no descriptor, no allocation. Every step counts the samples that have entered and
// left it, keeps what the next push still needs on the device in two copies — a push reads one and writes the other, and they are
// flipped when the push has succeeded: a push that fails or is refused leaves the row exactly where it was — and writes a push's
// samples into the row's part of a buffer of its own (s, y, v, w, m, z), which the next step that is on takes as the row's input.
// One launch per step serves every row of a push that has the step, a descriptor per row. The host side further down writes the
// chain once (step_on, step_emitted, step_cap, chain_walk); the count, the plan and the commit of a push are three uses of it.
//
// 1. The silence step. k_trim takes the energy of every 10 ms hop of the row's 24 kHz stream, calls a hop active
// when a hop within 20 ms of it is above a threshold, and drops what a run of non-active hops has beyond an edge (at the stream's
// two ends) or beyond a cap (inside it, with one crossfaded hop at the seam). How many samples leave depends on the data, so a push
// with such a row runs in two passes: k_trim into s, the kept counts back to the host, then the plan and the launches of the
// steps behind. The row keeps the input whose fate is open (the last hops, and the front of the run in progress) and its counters.
// A push without such a row is a single pass.
//
// 2. The stretcher: a speaking rate. k_tempo stretches the stream by WSOLA — frames of 720 samples every 360 of the
// output, each taken from where the input continues the frame before it best within +-240 samples of its nominal place — into y.
// Which frames a push reaches follows from the sample counts alone (tempo_frames), so the host never reads a count back; the row
// keeps the input the next frame can still touch and the last frame's position. It runs at the effective tempo te, which is the
// row's tempo t moved by its pitch; a row at te = 1000 has no stretcher.
//
// 3. The pitch step: a pitch in cents. With te = llround(t / 2^(c / 1200)) in the place of t in the stretcher,
// k_pitch resamples the stretcher's output by te / t into v: q3_resample's filter, at a ratio whose table taps[te][128] would be
// too large to build per request, so the taps are evaluated per output from two tables that serve every ratio: the sinc at 512
// points per zero crossing and the squared window at 64 points per tap, both interpolated linearly at positions that integer
// arithmetic splits exactly into an index and a remainder. It holds 64 samples back like the resampler and keeps the row's last 128
// inputs. A row whose te equals its t (0 cents) has no pitch step.
//
// 4. The loudness step. k_loud K-weights the stream (ITU-R BS.1770-4: two biquads), keeps the energy of every 100 ms
// hop and the mean square of every 400 ms block, gates the blocks the row has seen so far (absolute and relative gate) into its
// integrated loudness, and — where the row normalises — multiplies the stream by a gain that ramps, hop by hop, toward the one that
// would bring that loudness to a target, into w. A hop's gain depends on the hops that ended before it alone, so the step holds
// nothing back: n samples leave for n that enter (a row that only meters hands its input on as it is). The row keeps its filter
// states, partial sums, last energies and gains in two copies, its block values append-only.
//
// 4f. The mark step. k_mark adds a keyed carrier — a period of 4096 samples with unit magnitude and key-derived
// phases in 500..3000 Hz — under a gain that follows the stream's own level: the root mean square of every 10 ms hop, ramped between
// the two hops that ended before the sample's hop began, times a strength. Like the loudness step it holds nothing back; the row
// keeps the partial sums of its open hop and two roots in two copies, and its carrier. It stands in front of the level step, so a
// ceiling holds behind it. q3_mark_embed is its host twin, q3_mark_detect (and q3_intake.hip's kernels) the detector.
//
// 5. The level step. k_level multiplies the stream by a gain and by the mean, over 128 samples, of the minima, over
// 128 samples, of the reduction each sample needs to stay under a ceiling: a look-ahead peak limiter whose output is a function of
// the sample index alone, into z. It holds 127 samples back and keeps the row's last 254 inputs.
//
// 6. The resampler and the format. The filter is q3_resample's (q3_io.cpp): a 128-tap Blackman-Harris²-windowed sinc
// at 0.95 x the lower Nyquist, output i at input time i * M / L with L / M = sr_out / 24000 in lowest terms. What the host loop
// evaluates per output sample in f64 is a function of the phase p = (i * M) mod L alone, so it is tabulated once per rate:
// taps[L][128] (f64, rounded to f32), and output i is the dot product of row p with inputs c - 63 .. c + 64, c = floor(i * M / L):
// f32 products, accumulated in a fixed order. A row emits output i once input c + 64 has arrived (and, with `last`, everything up
// to llround(n_in * sr_out / 24000) against zeros). The next output to emit then starts no earlier than 127 samples before the
// end of what has arrived, so a row keeps its last 128 input samples. k_pcm_stage's grid is (output tile, row): a block stages its
// tile's input window (kept tail | new samples | zeros) in LDS and computes one output per thread; tile 0 of a row also writes
// the row's next tail. Formats: f32, PCM16, and G.711 mu-law / A-law — the companding of the PCM16 value, one byte per sample.
#include "q3_engine.h"

// The steps' descriptors: one row of a pass of a step's kernel each (device-visible, 8-byte aligned). PsDesc, the resampler's, is
// in q3_engine.h: a codec stream carries it in its own descriptor block.
// k_trim, DESIGN 4.12e: the row's stream into the silence step is head_in (the
// undecided front of the run in progress, head hops from hop run + m on), tail_in (its last `tail` samples) below `base`, the n_new
// samples of src from there, zeros from n_total on. Hops c_old .. c_end - 1 get their energy in this pass, hops k_old .. k_new - 1
// are classified; st_in (null at the row's start) / st_out: the two copies of the row's TR_ST counters, res: st_out again, where the
// host reads it; y: the kept samples, ops: the kept hops (source hop, seam partner or -1), fl: loud and active flags of the pass
struct TrDesc {
    const float* src; const float* tail_in; float* tail_out; const float* head_in; float* head_out;
    const long long* st_in; long long* st_out; long long* res;
    float* y; int* ops; unsigned char* fl; const float* win;
    long long base, n_total, c_old, c_end, c_new, k_old, k_new;
    int n_new, last, E, P1, P2, tail, head, cap_ops; float theta; int fl_n;
    int tail_lead, tail_run;                // what tail_out takes: behind a leading run in progress, and otherwise (tail: what tail_in holds)
};
// k_tempo: the row's stream is hist_in (from sample hist_lo on) below
// `base`, the n_new samples of src from there, zeros from n_total on; frames k0 .. k1 - 1 run, n_y samples of y come out
struct TpDesc {
    const float* src; const float* hist_in; float* hist_out; const long long* p_in; long long* p_out; int* lags; float* y; const float* win;
    long long base, n_total, hist_lo, lo_next, k0, k1;
    int n_new, n_y, tempo, pad;
};
// k_pitch: the row's stream into the pitch step is tail_in (its last 128
// samples) below `base`, the n_new samples of src from there, zeros beyond; outputs j0 .. j0 + n_v - 1 go to v, output j at input
// time j t / te. sc / w2: the stage's sinc and window tables. den1 = 20 max(t, te); dq1, dr1: quotient and remainder of
// 19 S1 te by den1, what the sinc position advances by per tap; fc: (float)(0.95 min(1, te / t))
struct PtDesc {
    const float* src; const float* tail_in; float* tail_out; float* v; const float* sc; const float* w2;
    long long base, j0;
    int n_new, n_v, t, te, den1, dq1, dr1; float fc;
};
// k_loud: samples base .. base + n_new - 1 of the row's stream into the loudness
// step come from src; st_in (null at the row's start) / st_out are the two copies of its small state, hist its block values; w
// (null in meter mode) receives the n_new normalised samples. coef: b0 b1 b2 a1 a2 of the shelf, then of the high-pass
struct LoDesc {
    const float* src; float* w; const float* st_in; float* st_out; float* hist;
    long long base;
    int n_new, mode; float T, P, gate, a_lo, a_hi; int pad;
    float coef[10];
};
// k_mark: samples base .. base + n_new - 1 of the row's stream into the mark step
// come from src and leave into y; st_in (null at the row's start) / st_out are the two copies of its small state, c the row's
// carrier, s its strength
struct MkDesc {
    const float* src; float* y; const float* c; const float* st_in; float* st_out;
    long long base;
    int n_new; float s;
};
// k_level: the row's stream into the level step is tail_in (its last 254
// samples) below `base`, the n_new samples of src from there, nothing from n_total on; outputs o_base .. o_base + n_z - 1 go to z
struct LvDesc {
    const float* src; const float* tail_in; float* tail_out; float* z;
    long long base, n_total, o_base;
    int n_new, n_z; float g, c;
};

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

// G.711 of the int16 v that pcm16_of gives (ITU-T G.711; the segment is the place of the leading bit)
__device__ inline uint8_t ulaw_of(int v) {
    int p = v >> 2, mask = 0xFF;
    if (p < 0) { p = -p; mask = 0x7F; }
    p = min(p, 8159) + 33;                                       // 33 .. 8192
    const int seg = 26 - __clz(p);                               // leading bit 5 + seg (p >= 33: seg >= 0)
    return (uint8_t)((seg >= 8 ? 0x7F : ((seg << 4) | ((p >> (seg + 1)) & 0xF))) ^ mask);
}
__device__ inline uint8_t alaw_of(int v) {
    int p = v >> 3, mask = 0xD5;
    if (p < 0) { mask = 0x55; p = -p - 1; }
    const int seg = max(0, 27 - __clz(p));                       // leading bit 4 + seg (p = 0: segment 0)
    return (uint8_t)((seg >= 8 ? 0x7F : ((seg << 4) | ((seg < 2 ? p >> 1 : p >> seg) & 0xF))) ^ mask);
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
    if (d.fmt == Q3_PCM_F32) ((float*)d.out)[o0 + tid] = y;
    else if (d.fmt == Q3_PCM_S16) ((int16_t*)d.out)[o0 + tid] = pcm16_of(y);
    else if (d.fmt == Q3_PCM_ULAW) ((uint8_t*)d.out)[o0 + tid] = ulaw_of(pcm16_of(y));
    else ((uint8_t*)d.out)[o0 + tid] = alaw_of(pcm16_of(y));
}

// ---- the level step ----
constexpr int LV_W = 128, LV_D = LV_W - 1;                      // window, look-ahead
constexpr int LV_TAIL = 2 * LV_D, LV_TAIL_PITCH = 256;          // inputs a row keeps (in 256 floats a copy)
constexpr int LV_R = PS_TILE + 2 * LV_D;                        // 510 reductions a tile reads, 383 minima
constexpr int LV_GAIN_MIN = -6000, LV_GAIN_MAX = 2400, LV_CEIL_MIN = -2400;

// Grid (tile of 256 outputs, row). The tile's outputs are n = o0 .. o0 + 255 of the row's stream; it stages the reductions
// r[o0 - 127 .. o0 + 255 + 127], halves them seven times into the minima over 128 (a minimum is exact: its order is free), and
// each thread sums the 128 minima that end at its sample in four interleaved sums, in ascending order. Both arrays are read and
// written at consecutive words by consecutive lanes: the 32 lanes of a half-wave meet 32 different banks.
__global__ __launch_bounds__(PS_TILE) void k_level(const LvDesc* __restrict__ descs) {
    __shared__ float ra[LV_R + 2], rb[LV_R + 2];
    const LvDesc d = descs[blockIdx.y];
    const int tid = threadIdx.x;
    // sample q of the row's stream into the step: the kept tail below `base`, the new samples from there; 0 outside [0, n_total)
    auto x_at = [&](long long q) -> float {
        if (q < 0 || q >= d.n_total) return 0.0f;
        if (q >= d.base) return d.src[q - d.base];
        const long long k = q - (d.base - LV_TAIL);
        return (k >= 0 && d.tail_in) ? d.tail_in[k] : 0.0f;
    };
    if (blockIdx.x == 0 && d.tail_out && tid < LV_TAIL) d.tail_out[tid] = x_at(d.n_total - LV_TAIL + tid);
    const long long o0 = d.o_base + (long long)blockIdx.x * PS_TILE;
    if ((long long)blockIdx.x * PS_TILE >= d.n_z) return;        // (uniform over the block)
    for (int j = tid; j < LV_R; j += PS_TILE) {
        // outside the stream x_at gives 0 and the reduction is 1; a NaN compares false: 1 too
        const float au = fabsf(q3::mul_rn(d.g, x_at(o0 - LV_D + j)));
        ra[j] = au > d.c ? __fdiv_rn(d.c, au) : 1.0f;
    }
    __syncthreads();
    float *a = ra, *b = rb;
    int len = LV_R;
#pragma unroll
    for (int s = 1; s < LV_W; s <<= 1) {                         // a[j] = min r[j .. j + 2 s - 1] after the step
        len -= s;
        for (int j = tid; j < len; j += PS_TILE) b[j] = fminf(a[j], a[j + s]);
        __syncthreads();
        float* t = a; a = b; b = t;
    }
    if ((long long)blockIdx.x * PS_TILE + tid >= d.n_z) return;
    // a[tid + k] = m[n - 127 + k]
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll 8
    for (int k = 0; k < LV_W; k += 4) {
        s0 = q3::add_rn(s0, a[tid + k]); s1 = q3::add_rn(s1, a[tid + k + 1]);
        s2 = q3::add_rn(s2, a[tid + k + 2]); s3 = q3::add_rn(s3, a[tid + k + 3]);
    }
    const float av = q3::mul_rn(q3::add_rn(q3::add_rn(s0, s1), q3::add_rn(s2, s3)), 1.0f / (float)LV_W);
    const float y = q3::mul_rn(q3::mul_rn(d.g, x_at(o0 + tid)), av);
    d.z[(long long)blockIdx.x * PS_TILE + tid] = y < -d.c ? -d.c : (y > d.c ? d.c : y);      // (a NaN stays one)
}
// the streaming rule: the outputs final after n inputs
inline long long level_emitted(long long n, bool ended) { return ended ? n : std::max<long long>(0, n - LV_D); }

// ---- the loudness step ----
constexpr int LD_HOP = 2400, LD_HIST = 4096;                    // 100 ms; the block values a row keeps
constexpr int LD_THREADS = 256;
constexpr int LD_STATE = 80;                                    // floats a copy of the small state: [filter states 4 | partials 64 | e 3 | A1 A2 M cg est]
constexpr int LD_S_E = 68, LD_S_A1 = 71, LD_S_A2 = 72, LD_S_M = 73, LD_S_CG = 74, LD_S_EST = 75;
constexpr int LD_TARGET_MIN = -4000, LD_TARGET_MAX = -500, LD_PRIOR_MIN = -6000, LD_PRIOR_MAX = 2400;

// The root of the gain, rounded once: sqrtf is the correctly rounded root in this build (no fast-math flag), where __fsqrt_rn
// compiles to the hardware's approximation, one ulp wide.
__device__ inline float ld_sqrt_rn(float x) { return sqrtf(x); }

// two f32 operations in one instruction (v_pk_mul_f32 / v_pk_add_f32), each half rounded once; no contraction, as in q3_kernels.h
typedef float ld_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ ld_f2 ld_mul2(ld_f2 a, ld_f2 b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ ld_f2 ld_add2(ld_f2 a, ld_f2 b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ ld_f2 ld_sub2(ld_f2 a, ld_f2 b) {
#pragma clang fp contract(off)
    return a - b;
}

// One workgroup per row; the hops the push touches in order. Per hop: the block stages the new samples (a non-finite one as 0)
// and, where the row normalises, writes them times the ramp between the two gains that were known before the hop began; lane 0
// runs the two biquads over the staged samples in place; lanes 0..63 add the squares to the hop's 64 partial sums. A hop that
// completes is folded by wave 0, its block value joins the history (kept in LDS for the launch, appended in memory), and wave 0
// runs the gate over the history in f64, 64 interleaved partials folded by shuffles in the defined order.
// LDS: staging and squares are read and written at consecutive words by consecutive lanes (the squares rotated by the hop's
// offset: a permutation of 64 consecutive words), the history at word lane + 64 k: no pass meets a bank twice.
__global__ __launch_bounds__(LD_THREADS) void k_loud(const LoDesc* __restrict__ descs) {
    __shared__ float buf[LD_HOP];
    __shared__ float zh[LD_HIST];
    __shared__ float pub[4];                                     // wave 0 -> the block: A_h, M, cg, est
    const LoDesc d = descs[blockIdx.x];
    const int tid = threadIdx.x;
    long long h = d.base / LD_HOP;                               // the hop in progress
    int j0 = (int)(d.base - h * LD_HOP);
    // the row's small state: the gains and the reading in every thread, the hop energies in wave 0, the filter states in thread 0,
    // partial q in thread q
    float e3 = 0.0f, e2 = 0.0f, e1 = 0.0f, A1 = d.P, A2 = d.P, M = 0.0f, part = 0.0f;
    float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f, f3 = 0.0f;
    int cg = 0, est = 0;
    if (d.st_in) {
        e3 = d.st_in[LD_S_E]; e2 = d.st_in[LD_S_E + 1]; e1 = d.st_in[LD_S_E + 2];
        A1 = d.st_in[LD_S_A1]; A2 = d.st_in[LD_S_A2]; M = d.st_in[LD_S_M];
        cg = __float_as_int(d.st_in[LD_S_CG]); est = __float_as_int(d.st_in[LD_S_EST]);
        f0 = d.st_in[0]; f1 = d.st_in[1]; f2 = d.st_in[2]; f3 = d.st_in[3];
        if (tid < 64) part = d.st_in[4 + tid];
    }
    {
        const long long nb = h < 3 ? 0 : (h - 3 < LD_HIST ? h - 3 : LD_HIST);      // blocks of the hops that ended before this push
        for (int i = tid; i < (int)nb; i += LD_THREADS) zh[i] = d.hist[i];
    }
    const float b0 = d.coef[0], b1 = d.coef[1], b2 = d.coef[2], a1 = d.coef[3], a2 = d.coef[4];
    const float c0 = d.coef[5], c1 = d.coef[6], c2 = d.coef[7], a3 = d.coef[8], a4 = d.coef[9];
    long long done = 0;
    while (done < d.n_new) {
        const int cnt = (int)(d.n_new - done < (long long)(LD_HOP - j0) ? d.n_new - done : (long long)(LD_HOP - j0));
        const float* x = d.src + done;
        const float dg = q3::sub_rn(A1, A2);
        for (int i = tid; i < cnt; i += LD_THREADS) {
            const float v = x[i];
            buf[i] = __builtin_isfinite(v) ? v : 0.0f;
            if (d.w) d.w[done + i] = q3::mul_rn(v, q3::add_rn(A2, q3::mul_rn(dg, __fdiv_rn((float)(j0 + i), (float)LD_HOP))));
        }
        __syncthreads();
        if (tid == 0) {
            // The high-pass runs one sample behind the shelf, so that the two chains are the two halves of packed f32
            // operations (.x: the shelf at sample i, .y: the high-pass at sample i - 1): the same operations on the same
            // operands, each rounded once, at half the instructions a lone lane has to issue.
            const ld_f2 B0 = {b0, c0}, B1 = {b1, c1}, B2 = {b2, c2}, A1v = {a1, a3}, A2v = {a2, a4};
            ld_f2 S1 = {f0, f2}, S2 = {f1, f3};
            float o;
            {                                                    // the shelf alone at sample 0
                const float v = buf[0];
                o = q3::add_rn(q3::mul_rn(b0, v), S1.x);
                S1.x = q3::add_rn(q3::sub_rn(q3::mul_rn(b1, v), q3::mul_rn(a1, o)), S2.x);
                S2.x = q3::sub_rn(q3::mul_rn(b2, v), q3::mul_rn(a2, o));
            }
            int i = 1;
            for (; i + 8 <= cnt; i += 8) {                       // (the loads first: the stores below go to words already read)
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = buf[i + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const ld_f2 V = {v[u], o};
                    const ld_f2 O = ld_add2(ld_mul2(B0, V), S1);
                    S1 = ld_add2(ld_sub2(ld_mul2(B1, V), ld_mul2(A1v, O)), S2);
                    S2 = ld_sub2(ld_mul2(B2, V), ld_mul2(A2v, O));
                    o = O.x; buf[i + u - 1] = O.y;
                }
            }
            for (; i < cnt; ++i) {
                const ld_f2 V = {buf[i], o};
                const ld_f2 O = ld_add2(ld_mul2(B0, V), S1);
                S1 = ld_add2(ld_sub2(ld_mul2(B1, V), ld_mul2(A1v, O)), S2);
                S2 = ld_sub2(ld_mul2(B2, V), ld_mul2(A2v, O));
                o = O.x; buf[i - 1] = O.y;
            }
            {                                                    // the high-pass alone at the last sample
                const float k = q3::add_rn(q3::mul_rn(c0, o), S1.y);
                S1.y = q3::add_rn(q3::sub_rn(q3::mul_rn(c1, o), q3::mul_rn(a3, k)), S2.y);
                S2.y = q3::sub_rn(q3::mul_rn(c2, o), q3::mul_rn(a4, k));
                buf[cnt - 1] = k;
            }
            f0 = S1.x; f2 = S1.y; f1 = S2.x; f3 = S2.y;
        }
        __syncthreads();
        if (tid < 64)                                            // sample i of the staging is sample j0 + i of the hop
            for (int i = (tid - j0) & 63; i < cnt; i += 64) part = q3::add_rn(part, q3::mul_rn(buf[i], buf[i]));
        j0 += cnt; done += cnt;
        if (j0 < LD_HOP) break;                                  // (the push ends inside the hop)
        if (tid < 64) {                                          // wave 0: hop h is complete
            float s = part;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) s = q3::add_rn(s, __shfl_down(s, o));
            const float e0 = __shfl(s, 0);
            float An = h < 3 ? d.P : A1, Mn = M; int cgn = cg, en = est;
            const long long bi = h - 3;
            if (bi >= 0 && bi < LD_HIST) {
                const float z = q3::mul_rn(q3::add_rn(q3::add_rn(e3, e2), q3::add_rn(e1, e0)), (float)(1.0 / 9600.0));
                if (tid == 0) { zh[bi] = z; d.hist[bi] = z; }
                const int nb = (int)bi + 1;                      // (the newest block from the register: every lane has it)
                double Sa = 0.0; int ca = 0;
                for (int i = tid; i < nb; i += 64) { const float zi = i == (int)bi ? z : zh[i]; if (zi > d.gate) { Sa += (double)zi; ++ca; } }
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) { Sa += __shfl_down(Sa, o); ca += __shfl_down(ca, o); }
                Sa = __shfl(Sa, 0); ca = __shfl(ca, 0);
                if (ca > 0) {
                    const double Gr = (0.1 * Sa) / (double)ca;
                    double Sg = 0.0; int c2n = 0;
                    for (int i = tid; i < nb; i += 64) { const float zi = i == (int)bi ? z : zh[i]; if (zi > d.gate && (double)zi > Gr) { Sg += (double)zi; ++c2n; } }
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) { Sg += __shfl_down(Sg, o); c2n += __shfl_down(c2n, o); }
                    Sg = __shfl(Sg, 0); c2n = __shfl(c2n, 0);
                    Mn = (float)(Sg / (double)c2n); cgn = c2n; en = 1;
                }
                An = en ? fminf(fmaxf(ld_sqrt_rn(__fdiv_rn(d.T, Mn)), d.a_lo), d.a_hi) : A1;
            }
            if (tid == 0) { pub[0] = An; pub[1] = Mn; pub[2] = __int_as_float(cgn); pub[3] = __int_as_float(en); }
            e3 = e2; e2 = e1; e1 = e0; part = 0.0f;
        }
        __syncthreads();
        A2 = A1; A1 = pub[0]; M = pub[1]; cg = __float_as_int(pub[2]); est = __float_as_int(pub[3]);
        j0 = 0; ++h;
        __syncthreads();                                         // (pub and buf are written again)
    }
    if (tid == 0) {
        d.st_out[0] = f0; d.st_out[1] = f1; d.st_out[2] = f2; d.st_out[3] = f3;
        d.st_out[LD_S_E] = e3; d.st_out[LD_S_E + 1] = e2; d.st_out[LD_S_E + 2] = e1;
        d.st_out[LD_S_A1] = A1; d.st_out[LD_S_A2] = A2; d.st_out[LD_S_M] = M;
        d.st_out[LD_S_CG] = __int_as_float(cg); d.st_out[LD_S_EST] = __int_as_float(est);
    }
    if (tid < 64) d.st_out[4 + tid] = part;
}

// ---- the mark step ----
constexpr int MK_P = 4096, MK_H = 240;                          // the carrier's period; hop (10 ms)
constexpr int MK_THREADS = 256, MK_G = MK_THREADS / 64;         // hops of a round: one per wave
constexpr int MK_STATE = 68;                                    // floats a copy of the small state: [partials 64 | r(h-1) r(h-2) | - -]
constexpr int MK_S_R1 = 64, MK_S_R2 = 65;
constexpr int MK_STRENGTH_MIN = -4000, MK_STRENGTH_MAX = -1000;
constexpr int MK_BAND_LO = 500, MK_BAND_HI = 3000;              // Hz

// One workgroup per row; the hops the push touches in rounds of four, one hop per wave. Per round: lane q of a wave adds the squares
// of samples q, q + 64, ... of its hop that lie in the push (a non-finite one as 0; the hop the push opens in continues the row's
// partials), the fold is the wave reduction d = 32 .. 1, and lane 0 posts the root of the hop's mean square; then every thread
// writes samples of the round's hops: the sample plus the carrier under a gain that ramps between the roots of the two hops that
// ended before the sample's hop began. The hop energies do not depend on each other, so a round needs the two roots before it alone.
// Bounds: src and y hold n_new floats and i below is in [0, n_new); c holds MK_P floats; st_in / st_out MK_STATE.
__global__ __launch_bounds__(MK_THREADS) void k_mark(const MkDesc* __restrict__ descs) {
    __shared__ float rr[2 + MK_G];                               // r(h0 - 2), r(h0 - 1), then the round's own
    const MkDesc d = descs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long end = d.base + d.n_new;
    const long long h_first = d.base / MK_H, h_end = (end + MK_H - 1) / MK_H;
    float r1 = d.st_in ? d.st_in[MK_S_R1] : 0.0f, r2 = d.st_in ? d.st_in[MK_S_R2] : 0.0f;       // (thread 0's are the row's)
    if (tid == 0) { rr[0] = r2; rr[1] = r1; }
    for (long long h0 = h_first; h0 < h_end; h0 += MK_G) {
        const long long h = h0 + wave;
        if (h < h_end) {
            float part = (h == h_first && d.st_in) ? d.st_in[lane] : 0.0f;
            for (int j = lane; j < MK_H; j += 64) {
                const long long n = h * MK_H + j;
                if (n < d.base || n >= end) continue;
                float v = d.src[n - d.base];
                v = __builtin_isfinite(v) ? v : 0.0f;
                part = q3::add_rn(part, q3::mul_rn(v, v));
            }
            const bool complete = (h + 1) * MK_H <= end;
            if (h == h_end - 1) d.st_out[lane] = complete ? 0.0f : part;      // the partials of the hop still open
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) part = q3::add_rn(part, __shfl_down(part, o));
            if (lane == 0) rr[2 + wave] = complete ? ld_sqrt_rn(q3::mul_rn(part, (float)(1.0 / 240.0))) : 0.0f;
        }
        __syncthreads();
        for (int i = tid; i < MK_G * MK_H; i += MK_THREADS) {
            const int w = i / MK_H, j = i - w * MK_H;
            const long long n = (h0 + w) * MK_H + j;
            if (n < d.base || n >= end) continue;
            const float ra = rr[w], rb = rr[w + 1];              // r(h - 2), r(h - 1)
            const float g = q3::add_rn(ra, q3::mul_rn(q3::sub_rn(rb, ra), __fdiv_rn((float)j, (float)MK_H)));
            d.y[n - d.base] = q3::add_rn(d.src[n - d.base], q3::mul_rn(q3::mul_rn(d.s, g), d.c[n & (MK_P - 1)]));
        }
        const float n0 = rr[MK_G], n1 = rr[MK_G + 1];
        if (tid == 0)
            for (int w = 0; w < MK_G; ++w) if ((h0 + w + 1) * MK_H <= end) { r2 = r1; r1 = rr[2 + w]; }
        __syncthreads();
        if (tid == 0) { rr[0] = n0; rr[1] = n1; }                // (read again behind the next round's barrier)
    }
    if (tid == 0) { d.st_out[MK_S_R1] = r1; d.st_out[MK_S_R2] = r2; }
}

// ---- the time stretcher ----
constexpr int TP_W = 720, TP_HS = 360, TP_D = 240;             // frame, synthesis hop, search reach
constexpr int TP_MIN = 500, TP_MAX = 2000, TP_OFF = 1000;       // tempo in permille; 1000: no stretcher
constexpr int TP_LAGS = 2 * TP_D + 1;                           // 481 candidates
constexpr int TP_THREADS = 256;                                 // 64 groups of 8 consecutive lags (61 in use) x the 4 interleaved sums
constexpr int TP_SP = 1216;                                     // pitch of one copy of the search region: 8 * 60 + 4 * 180 + 8 <= 1216
constexpr int TP_S_FLOATS = 3 * TP_SP + 36 + TP_SP;
constexpr int TP_HIST = 2048;                                   // input a row keeps: < |a_k - a_{k-1} - Hs| + 2 * 240 + 720 <= 1561
constexpr int TP_NONE = 9999;                                   // no candidate yet

__device__ inline bool tp_better(float s1, int d1, float s2, int d2) {
    if (s1 > s2) return true;
    if (!(s1 == s2)) return false;
    const int a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2;
    return a1 < a2 || (a1 == a2 && d1 < d2);                    // ties: the smallest |lag|, then the negative one
}

// One workgroup per row; the row's frames k0 .. k1 - 1 in order (frame k's template is the continuation of frame k - 1).
// Thread (g, m) = (tid >> 2, tid & 3) owns lags 8g .. 8g + 7 and the partial sums over j = m (mod 4): per step of j one
// float4 of the search region (a sliding window of 8) and a quarter float4 of the template feed 16 FMAs. The four partial
// sums meet by two quad shuffles in the order (s0 + s1) + (s2 + s3): the order of the sums does not depend on how the
// input was cut into pushes. Copy m of the search region is shifted by m samples, so that every window is 16-byte aligned;
// the copies start at banks 0 / 4 / 32 / 36, so that the 16 lanes of one LDS pass read 64 different banks.
__global__ __launch_bounds__(TP_THREADS) void k_tempo(const TpDesc* __restrict__ descs) {
    __shared__ __attribute__((aligned(16))) float Tt[TP_W];           // template, transposed: Tt[m * 180 + i] = T[m + 4 i]
    __shared__ __attribute__((aligned(16))) float Sc[TP_S_FLOATS];    // copy m at sbase(m): Sc[sbase(m) + i] = x[a_k - 240 + i + m]
    __shared__ float red_s[TP_THREADS / 64]; __shared__ int red_d[TP_THREADS / 64];
    const TpDesc d = descs[blockIdx.x];
    const int tid = threadIdx.x, m = tid & 3, g = tid >> 2;
    auto sbase = [](int mm) { return mm * TP_SP + ((mm & 1) ? 4 : 0) + ((mm & 2) ? 32 : 0); };
    auto x_at = [&](long long q) -> float {
        if (q < 0 || q >= d.n_total) return 0.0f;
        if (q >= d.base) return d.src[q - d.base];
        const long long h = q - d.hist_lo;
        return (h >= 0 && h < TP_HIST && d.hist_in) ? d.hist_in[h] : 0.0f;
    };
    const long long y_base = d.k0 * TP_HS;
    long long p_prev = (d.k0 > 0 && d.p_in) ? d.p_in[0] : 0;
    for (long long k = d.k0; k < d.k1; ++k) {
        if (k == 0) {                                                // frame 0: its first half as it is
            for (int j = tid; j < TP_HS; j += TP_THREADS) if (j < d.n_y) d.y[j] = x_at(j);
            if (tid == 0) d.lags[0] = 0;
            p_prev = 0;
            continue;
        }
        const long long a = (k * TP_HS * (long long)d.tempo) / 1000;
        __syncthreads();                                             // (the frame before has read its LDS)
        for (int j = tid; j < TP_W; j += TP_THREADS) Tt[(j & 3) * (TP_W / 4) + (j >> 2)] = x_at(p_prev + TP_HS + j);
        for (int i = tid; i < TP_SP + 3; i += TP_THREADS) {
            const float v = i < TP_W + 2 * TP_D ? x_at(a - TP_D + i) : 0.0f;
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) if (i - mm >= 0 && i - mm < TP_SP) Sc[sbase(mm) + i - mm] = v;
        }
        __syncthreads();
        float bs = -INFINITY; int bd = TP_NONE;
        if (g * 8 < TP_LAGS) {
            float c[8], e[8], w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) c[u] = e[u] = 0.0f;
            const float4* S4 = (const float4*)(Sc + sbase(m)) + 2 * g;
            const float4* T4 = (const float4*)(Tt + m * (TP_W / 4));
            { const float4 lo = S4[0], hi = S4[1]; w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w; }
            for (int ib = 0; ib < TP_W / 16; ++ib) {
                const float4 t4 = T4[ib];
                const float tq[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 nx = S4[4 * ib + q + 2];            // (the last one is read and not used: inside the copy's pitch)
#pragma unroll
                    for (int u = 0; u < 8; ++u) { c[u] = fmaf(w[u], tq[q], c[u]); e[u] = fmaf(w[u], w[u], e[u]); }
                    w[0] = w[4]; w[1] = w[5]; w[2] = w[6]; w[3] = w[7]; w[4] = nx.x; w[5] = nx.y; w[6] = nx.z; w[7] = nx.w;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                c[u] = q3::add_rn(c[u], __shfl_xor(c[u], 1)); c[u] = q3::add_rn(c[u], __shfl_xor(c[u], 2));
                e[u] = q3::add_rn(e[u], __shfl_xor(e[u], 1)); e[u] = q3::add_rn(e[u], __shfl_xor(e[u], 2));
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if ((u >> 1) != m) continue;                         // each lane of the quad scores two of the eight
                const int lag = g * 8 + u - TP_D;
                if (lag > TP_D || (long long)lag < -a) continue;
                const float sc = e[u] > 0.0f ? __fdiv_rn(c[u], __fsqrt_rn(e[u])) : 0.0f;
                if (tp_better(sc, lag, bs, bd)) { bs = sc; bd = lag; }
            }
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float os = __shfl_xor(bs, o); const int od = __shfl_xor(bd, o);
            if (tp_better(os, od, bs, bd)) { bs = os; bd = od; }
        }
        if ((tid & 63) == 0) { red_s[tid >> 6] = bs; red_d[tid >> 6] = bd; }
        __syncthreads();
        bs = red_s[0]; bd = red_d[0];
#pragma unroll
        for (int v = 1; v < TP_THREADS / 64; ++v) if (tp_better(red_s[v], red_d[v], bs, bd)) { bs = red_s[v]; bd = red_d[v]; }
        if (bd == TP_NONE) bd = 0;                                   // (every score a NaN)
        // overlap-add: the second half of the frame before (the template's first half) under the window's second half, the
        // first half of this frame under its first: two products and one sum, each rounded once
        for (int j = tid; j < TP_HS; j += TP_THREADS) {
            const long long idx = k * TP_HS + j - y_base;
            if (idx < d.n_y)
                d.y[idx] = q3::add_rn(q3::mul_rn(d.win[TP_HS + j], Tt[(j & 3) * (TP_W / 4) + (j >> 2)]), q3::mul_rn(d.win[j], Sc[bd + TP_D + j]));
        }
        if (tid == 0) d.lags[k - d.k0] = bd;
        p_prev = a + bd;
    }
    if (tid == 0) d.p_out[0] = p_prev;
    // what the next frame can still touch, for the next push
    if (d.hist_out) {
        const long long n = d.n_total - d.lo_next;
        for (long long i = tid; i < n && i < TP_HIST; i += TP_THREADS) d.hist_out[i] = x_at(d.lo_next + i);
    }
}

// a_k = floor(k * Hs * t / 1000)
inline long long tp_a(long long k, int t) { return (long long)(((__int128)k * TP_HS * t) / 1000); }
inline long long tp_need(long long k, int t) { return k == 0 ? TP_W : std::max(tp_a(k, t), tp_a(k - 1, t) + TP_HS) + TP_D + TP_W; }
// the first input sample frame k can touch
inline long long tp_lo(long long k, int t) { return k == 0 ? 0 : std::max<long long>(0, std::min(tp_a(k, t), tp_a(k - 1, t) + TP_HS) - TP_D); }
// The streaming rule: after n input samples the frames with need_k <= n are computed and frames * Hs samples of y are final;
// once the input has ended, the frames up to ceil(N_out / Hs) are, and y is N_out = floor((n * 1000 + t / 2) / t) samples long.
void tempo_frames(int t, long long n, bool ended, long long* frames, long long* samples) {
    if (ended) {
        const long long n_out = (long long)(((__int128)n * 1000 + t / 2) / t);
        *frames = (n_out + TP_HS - 1) / TP_HS; *samples = n_out;
        return;
    }
    long long f = 0;
    if (n >= TP_W) {
        // need_k >= k * Hs * t / 1000 - 1 + 960 and <= k * Hs * t / 1000 + 1320: an estimate from below, then single steps
        f = std::max<long long>(1, (long long)(((__int128)(n - TP_W - TP_D - TP_HS) * 1000) / ((long long)TP_HS * t)));
        while (f > 1 && tp_need(f - 1, t) > n) --f;
        while (tp_need(f, t) <= n) ++f;
    }
    *frames = f; *samples = f * TP_HS;
}
// the most y samples one push of n new input samples adds, at any place of the stream and with `last`
size_t tempo_y_bound(int t, size_t n) { return (size_t)((((__int128)n + TP_W + TP_D + TP_HS) * 1000 + t - 1) / t) + 1; }

// ---- the pitch step ----
constexpr int PT_S1 = 512, PT_S2 = 64;                          // table points per zero crossing of the sinc, per tap of the window
constexpr int PT_SC_N = 61 * PT_S1 + 2, PT_W2_N = PS_HALF * PT_S2 + 2;
constexpr int PT_CENTS_MAX = 1200;
// the window of a tile: floor((r0 + 255 t) / te) + 128 inputs, r0 < te and t / te <= 2: at most 638
constexpr int PT_WIN = 641;

// One tap: the sinc and the window, each interpolated between two table points, their product, and the sum it joins; every
// operation rounded once. rem1 < den1 <= 40000: both exact in f32, the quotient correctly rounded.
__device__ __forceinline__ float pt_tap(const float* __restrict__ sc, const float* __restrict__ w2, int m1, int rem1, float fden1, int m2,
                                        float f2, float x, float acc) {
    const float s0 = sc[m1], w0 = w2[m2];
    const float s = fmaf(__fdiv_rn((float)rem1, fden1), q3::sub_rn(sc[m1 + 1], s0), s0);
    const float w = fmaf(f2, q3::sub_rn(w2[m2 + 1], w0), w0);
    return fmaf(q3::mul_rn(s, w), x, acc);
}

// Grid (tile of 256 outputs, row). Output j of the row sits at input time j t / te: cj = floor(j t / te), r = (j t) mod te, taps
// over inputs cj + k, k = -63 .. 64, at tau = r / te - k. With q = |r - k te| the sinc is read at 19 q S1 / (20 max(t, te)) and the
// window at q S2 / te, both as (index, remainder / denominator): k <= 0 walks q down from r + 63 te by te a tap, k >= 1 up from
// te - r, so the index and the remainder move by constants (the window's by S2 and 0) and one division per half places them.
// Bounds: the window holds wlen <= 638 < PT_WIN floats and thread tid reads win[dc .. dc + 127], dc <= wlen - 128;
// q <= 64 te, so the sinc index + 1 <= 19 * 64 * S1 / 20 + 1 = 31130 < PT_SC_N and the window index + 1 <= 64 S2 + 1 < PT_W2_N;
// in_at reads src[0 .. n_new) and tail_in[0 .. 128); v takes n_v floats.
__global__ __launch_bounds__(PS_TILE) void k_pitch(const PtDesc* __restrict__ descs) {
    __shared__ float win[PT_WIN];
    const PtDesc d = descs[blockIdx.y];
    const int tid = threadIdx.x, o0 = blockIdx.x * PS_TILE;
    // sample g of the row's stream into the step: the kept tail below `base`, the new samples from there, zeros outside
    auto in_at = [&](long long g) -> float {
        if (g >= d.base) { const long long k = g - d.base; return k < d.n_new ? d.src[k] : 0.0f; }
        const long long k = g - (d.base - PS_TAPS);
        return (k >= 0 && d.tail_in) ? d.tail_in[k] : 0.0f;
    };
    if (blockIdx.x == 0 && d.tail_out && tid < PS_TAPS) d.tail_out[tid] = in_at(d.base + d.n_new - PS_TAPS + tid);
    if (o0 >= d.n_v) return;                                     // (uniform over the block)
    const int cnt = min(PS_TILE, d.n_v - o0);
    const long long q0 = (d.j0 + o0) * (long long)d.t, c0 = q0 / d.te;
    const int r0 = (int)(q0 - c0 * d.te);
    const long long w0 = c0 - (PS_HALF - 1);                     // first input of the window
    const int wlen = (r0 + (cnt - 1) * d.t) / d.te + PS_TAPS;
    for (int k = tid; k < wlen; k += PS_TILE) win[k] = in_at(w0 + k);
    __syncthreads();
    if (tid >= cnt) return;
    const int qq = r0 + tid * d.t, dc = qq / d.te, r = qq - dc * d.te;
    const float* x = win + dc;                                   // x[i]: input cj + k, k = i - 63
    const float fden1 = (float)d.den1, fte = (float)d.te;
    const int n2 = r * PT_S2, m2r = n2 / d.te, rem2r = n2 - m2r * d.te;       // the window's position of q = r
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;            // a[k mod 4], each in ascending k
    {                                                            // k = -63 .. 0: q = r - k te
        const unsigned n1 = 19u * PT_S1 * (unsigned)(r + (PS_HALF - 1) * d.te);      // (< 2^31)
        int m1 = (int)(n1 / (unsigned)d.den1), rem1 = (int)(n1 - (unsigned)m1 * (unsigned)d.den1);
        int m2 = m2r + (PS_HALF - 1) * PT_S2;
        const float f2 = __fdiv_rn((float)rem2r, fte);
        auto step = [&]() { m1 -= d.dq1; rem1 -= d.dr1; if (rem1 < 0) { rem1 += d.den1; --m1; } m2 -= PT_S2; };
#pragma unroll 2
        for (int i = 0; i < PS_HALF; i += 4) {                   // (k = -63 is 1 mod 4)
            a1 = pt_tap(d.sc, d.w2, m1, rem1, fden1, m2, f2, x[i], a1); step();
            a2 = pt_tap(d.sc, d.w2, m1, rem1, fden1, m2, f2, x[i + 1], a2); step();
            a3 = pt_tap(d.sc, d.w2, m1, rem1, fden1, m2, f2, x[i + 2], a3); step();
            a0 = pt_tap(d.sc, d.w2, m1, rem1, fden1, m2, f2, x[i + 3], a0); step();      // (the step past k = 0 is not read)
        }
    }
    {                                                            // k = 1 .. 64: q = k te - r
        const unsigned n1 = 19u * PT_S1 * (unsigned)(d.te - r);
        int m1 = (int)(n1 / (unsigned)d.den1), rem1 = (int)(n1 - (unsigned)m1 * (unsigned)d.den1);
        int m2 = rem2r ? PT_S2 - m2r - 1 : PT_S2 - m2r;
        const float f2 = rem2r ? __fdiv_rn((float)(d.te - rem2r), fte) : 0.0f;
        auto step = [&]() { m1 += d.dq1; rem1 += d.dr1; if (rem1 >= d.den1) { rem1 -= d.den1; ++m1; } m2 += PT_S2; };
#pragma unroll 2
        for (int i = PS_HALF; i < PS_TAPS; i += 4) {
            a1 = pt_tap(d.sc, d.w2, m1, rem1, fden1, m2, f2, x[i], a1); step();
            a2 = pt_tap(d.sc, d.w2, m1, rem1, fden1, m2, f2, x[i + 1], a2); step();
            a3 = pt_tap(d.sc, d.w2, m1, rem1, fden1, m2, f2, x[i + 2], a3); step();
            a0 = pt_tap(d.sc, d.w2, m1, rem1, fden1, m2, f2, x[i + 3], a0); step();      // (the step past k = 64 is not read)
        }
    }
    d.v[o0 + tid] = q3::mul_rn(d.fc, q3::add_rn(q3::add_rn(a0, a1), q3::add_rn(a2, a3)));
}

// te = llround(t / 2^(c / 1200)): the tempo the stretcher runs at so that the step's t / te brings the duration back to t's
inline int pitch_te(int t, int c) { return c == 0 ? t : (int)llround((double)t / pow(2.0, (double)c / 1200.0)); }
// The streaming rule, the resampler's with L / M = te / t: after F final inputs every j with floor(j t / te) + 64 <= F - 1 is out,
// and after the flush floor((2 F te + t) / (2 t)) in total
inline long long pitch_emitted(int t, int te, long long F, bool ended) {
    if (ended) return (2 * F * te + t) / (2 * (long long)t);
    return F > PS_HALF ? ((F - PS_HALF) * te + t - 1) / t : 0;
}
// the most outputs one push of n new inputs adds, at any place of the stream and with `last`
inline size_t pitch_v_bound(int t, int te, size_t n) { return (size_t)((((long long)n + PS_HALF) * te + t - 1) / t + 1); }
// Sc[m] = sinc(m / S1), W2[m] = w^2(m / (64 S2)) with q3_resample's window (0 from |v| = 1 on, as there): f64, rounded once
void pitch_tables(std::vector<float>& sc, std::vector<float>& w2) {
    const double a0 = 0.35875, a1 = 0.48829, a2 = 0.14128, a3 = 0.01168, PI = 3.14159265358979323846;
    sc.assign((size_t)PT_SC_N, 0.0f); w2.assign((size_t)PT_W2_N, 0.0f);
    sc[0] = 1.0f;
    for (int m = 1; m < PT_SC_N; ++m) { const double xs = PI * (double)m / (double)PT_S1; sc[(size_t)m] = (float)(sin(xs) / xs); }
    for (int m = 0; m < PS_HALF * PT_S2; ++m) {
        const double v = (double)m / (double)(PS_HALF * PT_S2);
        const double w = a0 + a1 * cos(PI * v) + a2 * cos(2.0 * PI * v) + a3 * cos(3.0 * PI * v);
        w2[(size_t)m] = (float)(w * w);
    }
}

// ---- the silence step ----
constexpr int TR_H = 240, TR_G = 2;                             // hop (10 ms), guard in hops
constexpr int TR_THREADS = 256;
constexpr int TR_ST = 8;                                        // long longs a copy of the counters: [out | run | lead | pause | trail | bits | - | overflow]
constexpr int TR_S_OUT = 0, TR_S_RUN = 1, TR_S_LEAD = 2, TR_S_PAUSE = 3, TR_S_TRAIL = 4, TR_S_BITS = 5, TR_S_OVER = 7;
constexpr int TR_THR_MIN = -9000, TR_THR_MAX = -2000, TR_EDGE_MAX = 1000, TR_PAUSE_MIN = 20, TR_PAUSE_MAX = 2000;

// the run in progress (its first hop, -1: none) and the samples cut so far at the front, in pauses and at the end
struct TrRun { long long s, lead, pause, trail; };
// The rules per run over the classified hops k0 .. k1 - 1 (last: k1 = NH, the stream of N samples ends): emit(a, b) names the kept
// hops in order, b = -1 for a hop that leaves as it is and the seam's partner otherwise. m = min(E, P1 - 1): hop i of a later run
// leaves at once for i < m, whatever the run turns out to be.
template <typename Act, typename Emit>
__host__ __device__ __forceinline__ void tr_walk(TrRun& r, long long k0, long long k1, bool last, long long N, int E, int P1, int P2, Act act, Emit emit) {
    const int P = P1 + P2, m = E < P1 - 1 ? E : P1 - 1;
    for (long long h = k0; h < k1; ++h) {
        if (act(h)) {
            if (r.s >= 0) {
                const long long S = h - r.s;
                if (r.s == 0) {                                  // leading: its last min(S, E) hops
                    const long long k = S < E ? S : E;
                    for (long long i = h - k; i < h; ++i) emit(i, -1);
                    r.lead = (h - k) * TR_H;
                } else if (S <= P) {                             // a short pause: whole
                    for (long long i = r.s + (S < m ? S : m); i < h; ++i) emit(i, -1);
                } else {                                         // a long one: P1 hops, the last of them the seam, and the last P2
                    for (long long i = r.s + m; i < r.s + P1 - 1; ++i) emit(i, -1);
                    emit(r.s + P1 - 1, h - P2 - 1);
                    for (long long i = h - P2; i < h; ++i) emit(i, -1);
                    r.pause += (S - P) * TR_H;
                }
                r.s = -1;
            }
            emit(h, -1);
        } else {
            if (r.s < 0) r.s = h;
            if (r.s > 0 && h - r.s < m) emit(h, -1);
        }
    }
    if (last && r.s >= 0) {
        const long long S = k1 - r.s, k = S < E ? S : E;
        if (r.s == 0) {                                          // silent throughout
            for (long long i = k1 - k; i < k1; ++i) emit(i, -1);
            r.lead = (k1 - k) * TR_H < N ? (k1 - k) * TR_H : N;
        } else {                                                 // trailing: its first min(S, E) hops
            for (long long i = r.s + (S < m ? S : m); i < r.s + k; ++i) emit(i, -1);
            r.trail = N - ((r.s + k) * TR_H < N ? (r.s + k) * TR_H : N);
        }
        r.s = -1;
    }
}

// One workgroup per row, four phases with a barrier between them. (1) Energies: wave w takes hops c_old + w, + 4, ...; lane q adds
// the squares of samples q, q + 64, ... of the hop in ascending order (partial q), the fold is the wave reduction d = 32 .. 1, and
// lane 0 stores whether the hop is loud, behind the flags of the four hops before c_old, which the row's counters carry. Then every
// thread ORs five neighbours into the active flag of a hop k_old .. k_new - 1. (2) Thread 0 walks those hops from the row's run
// (tr_walk) and lists the kept hops. (3) Every thread gathers: output i is sample i % 240 of kept hop i / 240, the seam hop two
// products and a sum, each rounded once. (4) The row's next tail, the front of the run still open, the counters.
// Bounds: fl holds fl_n = c_end - c_old + 4 loud flags and, from fl_n on, k_new - k_old active ones; g - (c_old - 4) >= 0 since
// g >= k_old - 2 >= c_old - 4, and < fl_n since g < c_end. ops holds cap_ops pairs and the walk stops listing at cap_ops (reported
// in the counters: the host refuses the push). x_at reads src[0 .. n_new), tail_in[0 .. tail) and head_in[0 .. head * 240), each
// behind its own range check; y takes at most 240 * cap_ops floats; tail_out tail_lead or tail_run floats; head_out head * 240
// from float tail_run on: a copy holds max(tail_lead, tail_run + head * 240) floats, and a head exists only behind the shorter tail.
__global__ __launch_bounds__(TR_THREADS) void k_trim(const TrDesc* __restrict__ descs) {
    __shared__ long long sh[2];                                  // thread 0 -> the block: samples kept, the run at the end
    const TrDesc d = descs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    TrRun run = {-1, 0, 0, 0};
    long long out0 = 0, bits = 0;
    if (d.st_in) {
        out0 = d.st_in[TR_S_OUT]; run.s = d.st_in[TR_S_RUN]; run.lead = d.st_in[TR_S_LEAD]; run.pause = d.st_in[TR_S_PAUSE];
        run.trail = d.st_in[TR_S_TRAIL]; bits = d.st_in[TR_S_BITS];
    }
    const int m = min(d.E, d.P1 - 1), M = max(d.E, d.P1);
    const long long head_lo = run.s > 0 ? (run.s + m) * TR_H : -1;
    // sample q of the row's stream into the step: zeros outside [0, n_total), the new samples from `base`, the tail below, the head
    auto x_at = [&](long long q) -> float {
        if (q < 0 || q >= d.n_total) return 0.0f;
        if (q >= d.base) return d.src[q - d.base];
        const long long k = q - (d.base - d.tail);
        if (k >= 0) return d.tail_in ? d.tail_in[k] : 0.0f;
        const long long hq = q - head_lo;
        return (head_lo >= 0 && hq >= 0 && hq < (long long)d.head * TR_H && d.head_in) ? d.head_in[hq] : 0.0f;
    };
    const long long f0 = d.c_old - 4;                            // the hop of fl[0]
    if (tid < 4) d.fl[tid] = (unsigned char)((bits >> (3 - tid)) & 1);
    for (long long h = d.c_old + wave; h < d.c_end; h += TR_THREADS / 64) {
        float part = 0.0f;
        for (int j = lane; j < TR_H; j += 64) {
            float v = x_at(h * TR_H + j);
            v = __builtin_isfinite(v) ? v : 0.0f;
            part = q3::add_rn(part, q3::mul_rn(v, v));
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) part = q3::add_rn(part, __shfl_down(part, o));
        if (lane == 0) d.fl[h - f0] = part > d.theta ? 1 : 0;    // (a NaN compares false)
    }
    __syncthreads();
    unsigned char* ac = d.fl + d.fl_n;
    for (long long i = tid; i < d.k_new - d.k_old; i += TR_THREADS) {
        const long long h = d.k_old + i;
        int a = 0;
        for (long long g = h - TR_G; g <= h + TR_G; ++g) if (g >= 0 && g >= f0 && g < d.c_end) a |= d.fl[g - f0];
        ac[i] = (unsigned char)a;
    }
    __syncthreads();
    if (tid == 0) {
        long long nops = 0, over = 0, last_hop = -1;
        tr_walk(run, d.k_old, d.k_new, d.last != 0, d.n_total, d.E, d.P1, d.P2,
                [&](long long h) { return ac[h - d.k_old] != 0; },
                [&](long long a, long long b) {
                    if (nops >= d.cap_ops) { over = 1; return; }
                    d.ops[2 * nops] = (int)a; d.ops[2 * nops + 1] = (int)b; ++nops; last_hop = a;
                });
        long long kept = nops * TR_H;
        if (last_hop >= 0 && (last_hop + 1) * TR_H > d.n_total) kept -= (last_hop + 1) * TR_H - d.n_total;      // the stream's last, partial hop
        long long nb = 0;                                        // loud flags of the last four complete hops, the newest in bit 0
        for (int i = 0; i < 4; ++i) { const long long g = d.c_new - 1 - i; if (g >= 0 && g >= f0) nb |= (long long)d.fl[g - f0] << i; }
        auto put = [&](int i, long long v) { d.st_out[i] = v; d.res[i] = v; };
        put(TR_S_OUT, out0 + kept); put(TR_S_RUN, run.s); put(TR_S_LEAD, run.lead); put(TR_S_PAUSE, run.pause); put(TR_S_TRAIL, run.trail);
        put(TR_S_BITS, nb); put(6, 0); put(TR_S_OVER, over);
        sh[0] = kept; sh[1] = run.s;
    }
    __syncthreads();
    const long long kept = sh[0], s_end = sh[1];
    for (long long i = tid; i < kept; i += TR_THREADS) {
        const long long k = i / TR_H; const int j = (int)(i - k * TR_H);
        const long long a = d.ops[2 * k], b = d.ops[2 * k + 1];
        const float xa = x_at(a * TR_H + j);
        d.y[i] = b < 0 ? xa : q3::add_rn(q3::mul_rn(xa, d.win[TR_H + j]), q3::mul_rn(x_at(b * TR_H + j), d.win[j]));
    }
    // (a leading run still open needs its last E hops; anything else the last P2 + 1: the head lies behind the shorter tail)
    const int tl = s_end == 0 ? d.tail_lead : d.tail_run;
    for (int i = tid; i < tl; i += TR_THREADS) d.tail_out[i] = x_at(d.n_total - tl + i);
    if (s_end > 0) {                                             // hops m .. M - 1 of the run in progress, as far as they are classified
        const long long lo = (s_end + m) * TR_H, hi = (s_end + M < d.k_new ? s_end + M : d.k_new) * TR_H;
        for (long long q = lo + tid; q < hi; q += TR_THREADS) d.head_out[q - lo] = x_at(q);
    }
}

// hops: E, P1, P2 of a setting; what a row retains at most (the issue's hold) and what its state keeps beside the counters
struct TrSet { int E, P1, P2; };
inline TrSet tr_set(int edge_ms, int pause_ms) { const int P = pause_ms / 10; return {edge_ms / 10, P - P / 2, P / 2}; }
inline size_t tr_hold(const TrSet& t) { return (size_t)(std::max(t.E, t.P1) + t.P2 + TR_G + 2) * TR_H; }
inline int tr_head(const TrSet& t) { return std::max(t.E, t.P1) - std::min(t.E, t.P1 - 1); }   // hops
// samples of the tail: the last hops that can still leave (E of a leading run in progress, else P2 + 1), the guard, the partial hop
inline int tr_tail_lead(const TrSet& t) { return (t.E + TR_G + 1) * TR_H; }
inline int tr_tail_run(const TrSet& t) { return (t.P2 + 1 + TR_G + 1) * TR_H; }
// floats of a copy behind the counters: a leading run's tail, or the shorter tail and the head — never more than tr_hold
inline size_t tr_state_floats(const TrSet& t) { return std::max((size_t)tr_tail_lead(t), (size_t)tr_tail_run(t) + (size_t)tr_head(t) * TR_H); }
inline float tr_theta(int threshold_mB) { return (float)(240.0 * pow(10.0, (double)threshold_mB / 1000.0)); }
// w0[j] = (float)((j + 0.5) / 240), then w1[j] = (float)(1 - (j + 0.5) / 240): f64, rounded once
void tr_window(float* w) {
    for (int j = 0; j < TR_H; ++j) { const double t = ((double)j + 0.5) / (double)TR_H; w[j] = (float)t; w[TR_H + j] = (float)(1.0 - t); }
}
inline float h_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
inline float h_add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
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
size_t fmt_bytes(int fmt) { return fmt == Q3_PCM_F32 ? 4 : fmt == Q3_PCM_S16 ? 2 : 1; }
bool fmt_ok(int fmt) { return fmt >= Q3_PCM_F32 && fmt <= Q3_PCM_ALAW; }
}  // namespace

void resampler_taps(int L, int M, std::vector<float>& out) { Rate r; r.L = L; r.M = M; taps_of(r, out); }

// ---- buffers ----
// A device buffer of a push. It grows by free, then 2 x the request: no push is in flight (each ends with a wait).
struct DevBuf {
    char* dev = nullptr; size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = dev_malloc((void**)&dev, bytes * 2);
        if (e == hipSuccess) cap = bytes * 2;
        return e;
    }
    void release() { dev_free(dev); dev = nullptr; cap = 0; }
};
// ... with a pinned host twin: what a push sends up (descriptors, samples) or takes back (converted samples, counters)
struct PairBuf {
    char *dev = nullptr, *host = nullptr; size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        hipError_t e = dev_malloc((void**)&dev, bytes * 2);
        if (e == hipSuccess) e = hipHostMalloc((void**)&host, bytes * 2, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes * 2;
        return e;
    }
    hipError_t upload(const void* src, size_t bytes, hipStream_t st) {
        const hipError_t e = reserve(bytes);
        if (e != hipSuccess) return e;
        memcpy(host, src, bytes);
        return hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st);
    }
    void release() {
        dev_free(dev); dev = nullptr;
        if (host) { (void)hipHostFree(host); host = nullptr; }
        cap = 0;
    }
};

// ---- a row: its steps in chain order ----
// The row holds what it was asked for (OutSettings) as pcm_stage_apply got it; every step holds what that function derived from it
// for the chain and the kernels (a step's own test of being on among it: step_on), the running totals of the samples that have entered and left it since the row's (re)start, and its
// state on the device in two copies: a push reads copy `cur` and writes the other, the commit flips. Between two steps that are on,
// what has left the one in front is what has entered the one behind.
struct Totals { long long in = 0, out = 0; };
struct SilStep : Totals {                     // DESIGN 4.12e; thr == 0: off
    int thr = 0; TrSet set = {0, 0, 0}; float theta = 0.0f;
    long long read[TR_ST] = {0, -1, 0, 0, 0, 0, 0, 0};        // the counters after the last successful push (the host's copy)
    char* state = nullptr; size_t copy = 0, cap = 0; int cur = 0;      // two copies of `copy` bytes: [TR_ST counters | tail | head]
    void reset() { in = out = 0; for (int i = 0; i < TR_ST; ++i) read[i] = i == TR_S_RUN ? -1 : 0; }
};
struct TempoStep : Totals {                   // DESIGN 4.12a; te: the tempo the stretcher runs at (PitchStep), 1000: off
    int te = TP_OFF;
    long long frames = 0;                     // frames computed
    char* state = nullptr; int cur = 0;       // two copies: [last frame's position (16 bytes) | TP_HIST floats of input]
    DevBuf lags[2]; int lag_cur = 0; long long lag_k0 = 0, lag_n = 0;      // the lags of a push: lag_cur holds the last successful push's
    void reset() { in = out = 0; frames = 0; lag_k0 = lag_n = 0; }
};
struct PitchStep : Totals {                   // DESIGN 4.12d; the row's tempo t and pitch are one setting: the stretcher runs at
    int t = TP_OFF, te = TP_OFF;              // te = pitch_te(t, cents), this step brings the duration back to t; te == t: off
    float* tail = nullptr; int cur = 0;       // two copies of 128 floats: the last 128 inputs
    void reset() { in = out = 0; }
};
struct LoudStep : Totals {                    // DESIGN 4.12c; out == in: the step holds nothing back
    int mode = Q3_LOUD_OFF; float T = 0.0f, P = 1.0f, gate = 0.0f, lo = 0.0f, hi = 0.0f;
    float* state = nullptr; int cur = 0;      // two copies of LD_STATE floats, then the LD_HIST block values (one copy)
    void reset() { in = out = 0; }
};
struct MarkStep : Totals {                    // DESIGN 4.12f; key == 0: off; out == in: the step holds nothing back
    uint64_t key = 0; float s = 0.0f;
    float* tab = nullptr; uint64_t tab_key = 0;      // the row's carrier (MK_P floats, of key tab_key; 0: none), then two copies of MK_STATE floats
    int cur = 0;
    void reset() { in = out = 0; }
};
struct LevelStep : Totals {
    bool on = false; float g = 1.0f, c = 1.0f;
    float* tail = nullptr; int cur = 0;       // two copies of LV_TAIL_PITCH floats: the last 254 inputs
    void reset() { in = out = 0; }
};
struct ResStep : Totals {                     // the resampler and the format; every row has it
    uint32_t sr = PS_RATE_IN; int fmt = Q3_PCM_F32; Rate r; const float* taps = nullptr;
    int cur = 0; bool fresh = true;           // which of the row's two tails (q3_pcm_stage::tails) holds the last 128 inputs; fresh: none yet (zeros)
    void reset() { in = out = 0; cur = 0; fresh = true; }
};
struct PsRow {
    OutSettings asked;
    SilStep sil; TempoStep tp; PitchStep pt; LoudStep ld; MarkStep mk; LevelStep lv; ResStep rs;
    bool ended = false;                       // flushed by a push with `last`: restarted by pcm_stage_apply / reset only
    void reset() { sil.reset(); tp.reset(); pt.reset(); ld.reset(); mk.reset(); lv.reset(); rs.reset(); ended = false; }
};
constexpr size_t TP_STATE_BYTES = 16 + (size_t)TP_HIST * 4;

// ---- the chain, written once ----
enum { ST_SIL, ST_TEMPO, ST_PITCH, ST_LOUD, ST_MARK, ST_LEVEL, ST_RES, ST_N };
static bool step_on(const PsRow& r, int s) {
    switch (s) {
    case ST_SIL: return r.sil.thr != 0;
    case ST_TEMPO: return r.tp.te != TP_OFF;
    case ST_PITCH: return r.pt.te != r.pt.t;
    case ST_LOUD: return r.ld.mode != Q3_LOUD_OFF;
    case ST_MARK: return r.mk.key != 0;
    case ST_LEVEL: return r.lv.on;
    default: return true;
    }
}
static const Totals& step_totals(const PsRow& r, int s) {
    switch (s) {
    case ST_SIL: return r.sil;
    case ST_TEMPO: return r.tp;
    case ST_PITCH: return r.pt;
    case ST_LOUD: return r.ld;
    case ST_MARK: return r.mk;
    case ST_LEVEL: return r.lv;
    default: return r.rs;
    }
}
// The count rule of a step behind the silence step: the total that has left it once `in` samples have entered (with `last`: and the
// input has ended). The stretcher also says which frame it reaches. (What leaves the silence step depends on the data: its pre-pass
// says.)
static long long step_emitted(const PsRow& r, int s, long long in, bool last, long long* frames) {
    switch (s) {
    case ST_TEMPO: {
        long long f = 0, y = 0;
        tempo_frames(r.tp.te, in, last, &f, &y);
        *frames = std::max(f, r.tp.frames);
        return y;
    }
    case ST_PITCH: return pitch_emitted(r.pt.t, r.pt.te, in, last);
    case ST_LEVEL: return level_emitted(in, last);
    case ST_RES: return emitted(r.rs.sr, r.rs.r, in, last);
    default: return in;
    }
}
// The cap rule of a step in front of the resampler (whose own is q3_pcm_stage_bound): the most one push can hand on for n that enter
static size_t step_cap(const PsRow& r, int s, size_t n) {
    switch (s) {
    case ST_SIL: return n + tr_hold(r.sil.set);                    // its own samples and what the row had retained
    case ST_TEMPO: return tempo_y_bound(r.tp.te, n);
    case ST_PITCH: return pitch_v_bound(r.pt.t, r.pt.te, n);
    case ST_LEVEL: return n + LV_D;                                // with `last`, the 127 held back
    default: return n;
    }
}
static size_t chain_cap(const PsRow& r, size_t n) {
    for (int s = ST_SIL; s < ST_RES; ++s) if (step_on(r, s)) n = step_cap(r, s, n);
    return n;
}
// One segment's way through the chain in a push: per step that is on, the new samples that enter and leave it (zero where it is
// off); the frame its stretcher reaches; where its slice of each step's push buffer starts; and what stands at the front of the
// steps behind the silence step — the segment's own samples, or what the pre-pass kept.
struct SegWalk {
    long long n_in[ST_N], n_out[ST_N], frames;
    size_t off[ST_N];
    const float* front; long long n_front;
    bool sil, runs;                           // the pre-pass ran for it; it passes the steps behind
};
// new in = what the step in front hands on, new out = rule - step.out, from step `first` on, into which n new samples go
static void chain_walk(const PsRow& r, int first, long long n, bool last, SegWalk& w) {
    for (int s = first; s < ST_N; ++s) {
        if (!step_on(r, s)) continue;
        const Totals& t = step_totals(r, s);
        w.n_in[s] = n;
        n = w.n_out[s] = std::max<long long>(0, step_emitted(r, s, t.in + n, last, &w.frames) - t.out);
    }
}

// what the chain needs for the push in progress beside PsPlan: per segment its walk, per step the descriptors and the tiles of a row
struct StepPlan {
    std::vector<SegWalk> seg;
    std::vector<TrDesc> sdesc; std::vector<int> sseg; std::vector<long long> sres;      // the pre-pass: descriptors, their segments, the counters that came back
    std::vector<TpDesc> tdesc; std::vector<PtDesc> pdesc; std::vector<LoDesc> odesc; std::vector<MkDesc> mdesc; std::vector<LvDesc> ldesc;
    int tiles[ST_N];
};
struct q3_pcm_stage {
    int device = 0, R = 0; size_t max_push = 0;
    hipStream_t st = nullptr;
    std::vector<PsRow> rows;
    std::unordered_map<uint32_t, float*> taps;                 // the resampler's, per rate, on the device
    float* tails = nullptr;                                    // the resampler's, [R][2][128]
    // the steps' tables, each built by the first row that turns the step on
    float* s_win = nullptr;                                    // the seam's weights: w0, then w1, 240 floats each
    float* t_win = nullptr;                                    // the Hann window, 720 floats
    float* p_tab = nullptr;                                    // the sinc table, PT_SC_N floats, then the window's, PT_W2_N
    float o_coef[10] = {0}; bool o_coef_set = false;           // the K-weighting at 24 kHz, f32
    // per step, allocated by the first push of a row that has it: what it writes in a push, row after row (s: kept samples | kept
    // hops | flags; y, v, w, z: samples; the resampler's is `out`), and its descriptors (the silence step's: then the rows' counters
    // coming back; the resampler's: then the rows' new samples of q3_pcm_stage_push)
    DevBuf buf[ST_N]; PairBuf desc[ST_N];
    PairBuf out;                                               // the converted samples of a push
    StepPlan plan;
};
template <class B>
static q3_status buf_reserve(q3_pcm_stage* ps, B& b, size_t bytes) {
    if (bytes <= b.cap) return Q3_OK;
    HIPC(hipSetDevice(ps->device));
    HIPC(b.reserve(bytes));
    return Q3_OK;
}
// a small table built on the host -> the device (undone on error)
static q3_status table_upload(q3_pcm_stage* ps, float** dst, const float* host, size_t n, const char* who, const char* what, const char* up) {
    HIPC(hipSetDevice(ps->device));
    float* d = nullptr;
    if (dev_malloc((void**)&d, n * 4) != hipSuccess) { (void)hipGetLastError(); return set_err(Q3_OOM, "%s: %s", who, what); }
    const hipError_t e = q3_hipMemcpy(d, host, n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { dev_free(d); return set_err(Q3_HIP_ERROR, "%s: %s upload: %s", who, up, hipGetErrorString(e)); }
    *dst = d;
    return Q3_OK;
}
// a row's state of a step, if it has none
template <class T>
static q3_status row_state(q3_pcm_stage* ps, T** p, size_t bytes, const char* who, const char* what, int row) {
    if (*p) return Q3_OK;
    HIPC(hipSetDevice(ps->device));
    if (dev_malloc((void**)p, bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return set_err(Q3_OOM, "%s: %s of row %d", who, what, row); }
    return Q3_OK;
}

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

// the resampler's cap for n samples that reach it. n is at most what chain_cap makes of 2^48 + a silence hold (below 2^52: the
// stretcher and the pitch step at most double a count each); times L <= 320 that stays far inside 63 bits
static q3_status resampler_bound(uint32_t sample_rate, size_t n, size_t* n_out_max) {
    Rate r;
    Q3C(rate_checked("q3_pcm_stage_bound", sample_rate, &r));
    if (!n_out_max) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_bound: null argument");
    // the most one push can return: its own samples and, with `last`, the 64 held back: llround(N L / M) - ceil((N - n - 64) L / M)
    *n_out_max = sample_rate == PS_RATE_IN ? n : (size_t)(((long long)(n + PS_HALF) * r.L + r.M - 1) / r.M + 1);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_bound(uint32_t sample_rate, size_t n_in, size_t* n_out_max) {
    Rate r;
    Q3C(rate_checked("q3_pcm_stage_bound", sample_rate, &r));
    if (!n_out_max) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_bound: null argument");
    if (n_in > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_bound: n_in above 2^48");
    return resampler_bound(sample_rate, n_in, n_out_max);
}

// The _bound family: the caps of the steps a row with these settings has, in chain order (chain_cap), then the resampler's. hold: what
// the row's silence step can retain (0: none). Each caller checks its own ranges first; tempo, cents and n_in (at most 2^48) are in range.
static q3_status bound_through(uint32_t sample_rate, int tempo, int cents, int with_level, size_t hold, size_t n_in, size_t* n_out_max) {
    PsRow r;                                                       // (the settings alone; its silence step's cap is n_in + hold)
    r.pt.t = tempo; r.pt.te = r.tp.te = pitch_te(tempo, cents); r.lv.on = with_level != 0;
    return resampler_bound(sample_rate, chain_cap(r, n_in + hold), n_out_max);
}

static q3_status tempo_checked(const char* who, int tempo) {
    if (tempo >= TP_MIN && tempo <= TP_MAX) return Q3_OK;
    return set_err(Q3_INVALID_ARG, "%s: tempo %d permille out of range (%d..%d; %d = off)", who, tempo, TP_MIN, TP_MAX, TP_OFF);
}

extern "C" q3_status q3_pcm_stage_tempo_count(int tempo_permille, size_t n_in_total, int ended, size_t* frames, size_t* samples_24k) {
    Q3C(tempo_checked("q3_pcm_stage_tempo_count", tempo_permille));
    if (n_in_total > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_tempo_count: n_in_total above 2^48");
    long long f = 0, y = 0;
    tempo_frames(tempo_permille, (long long)n_in_total, ended != 0, &f, &y);
    if (frames) *frames = (size_t)f;
    if (samples_24k) *samples_24k = (size_t)y;
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_bound_tempo(uint32_t sample_rate, int tempo_permille, size_t n_in, size_t* n_out_max) {
    Q3C(tempo_checked("q3_pcm_stage_bound_tempo", tempo_permille));
    if (n_in > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_bound_tempo: n_in above 2^48");
    return bound_through(sample_rate, tempo_permille, 0, 0, 0, n_in, n_out_max);
}

static q3_status level_checked(const char* who, int gain_mB, int ceiling_mB) {
    if (gain_mB < LV_GAIN_MIN || gain_mB > LV_GAIN_MAX)
        return set_err(Q3_INVALID_ARG, "%s: gain %d mB out of range (%d..%d)", who, gain_mB, LV_GAIN_MIN, LV_GAIN_MAX);
    if (ceiling_mB < LV_CEIL_MIN || ceiling_mB > 0)
        return set_err(Q3_INVALID_ARG, "%s: ceiling %d mB out of range (%d..0)", who, ceiling_mB, LV_CEIL_MIN);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_level_coeffs(int gain_mB, int ceiling_mB, float* g, float* c) {
    Q3C(level_checked("q3_pcm_stage_level_coeffs", gain_mB, ceiling_mB));
    // in f64, rounded once
    if (g) *g = (float)pow(10.0, (double)gain_mB / 2000.0);
    if (c) *c = (float)pow(10.0, (double)ceiling_mB / 2000.0);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_level_count(size_t n_in_total, int ended, size_t* n_out) {
    if (!n_out) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_level_count: null argument");
    if (n_in_total > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_level_count: n_in_total above 2^48");
    *n_out = (size_t)level_emitted((long long)n_in_total, ended != 0);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_bound_level(uint32_t sample_rate, int tempo_permille, size_t n_in, size_t* n_out_max) {
    Q3C(tempo_checked("q3_pcm_stage_bound_level", tempo_permille));
    if (n_in > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_bound_level: n_in above 2^48");
    return bound_through(sample_rate, tempo_permille, 0, 1, 0, n_in, n_out_max);
}

extern "C" q3_status q3_loudness_kweight(uint32_t sample_rate, double* shelf_ba, double* highpass_ba) {
    if (sample_rate < 8000 || sample_rate > 192000) return set_err(Q3_INVALID_ARG, "q3_loudness_kweight: sample rate %u out of range (8000..192000)", sample_rate);
    if (!shelf_ba || !highpass_ba) return set_err(Q3_INVALID_ARG, "q3_loudness_kweight: null argument");
    // ITU-R BS.1770's analogue prototypes through the tangent pre-warped bilinear form
    const double PI = 3.14159265358979323846, fs = (double)sample_rate;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(PI * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
        shelf_ba[0] = (Vh + Vb * K / Q + K * K) / a0; shelf_ba[1] = 2.0 * (K * K - Vh) / a0; shelf_ba[2] = (Vh - Vb * K / Q + K * K) / a0;
        shelf_ba[3] = 1.0; shelf_ba[4] = 2.0 * (K * K - 1.0) / a0; shelf_ba[5] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(PI * f0 / fs), a0 = 1.0 + K / Q + K * K;
        highpass_ba[0] = 1.0; highpass_ba[1] = -2.0; highpass_ba[2] = 1.0;
        highpass_ba[3] = 1.0; highpass_ba[4] = 2.0 * (K * K - 1.0) / a0; highpass_ba[5] = (1.0 - K / Q + K * K) / a0;
    }
    return Q3_OK;
}

static q3_status loud_checked(const char* who, int mode, int target_mB, int prior_mB) {
    if (mode < Q3_LOUD_OFF || mode > Q3_LOUD_NORMALIZE)
        return set_err(Q3_INVALID_ARG, "%s: mode must be Q3_LOUD_OFF (0), Q3_LOUD_METER (1) or Q3_LOUD_NORMALIZE (2)", who);
    if (target_mB < LD_TARGET_MIN || target_mB > LD_TARGET_MAX)
        return set_err(Q3_INVALID_ARG, "%s: target %d mB out of range (%d..%d; -1900 = -19 LUFS)", who, target_mB, LD_TARGET_MIN, LD_TARGET_MAX);
    if (prior_mB < LD_PRIOR_MIN || prior_mB > LD_PRIOR_MAX)
        return set_err(Q3_INVALID_ARG, "%s: prior gain %d mB out of range (%d..%d)", who, prior_mB, LD_PRIOR_MIN, LD_PRIOR_MAX);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_loudness_consts(int target_mB, int prior_mB, float* T, float* P, float* gate_abs, float* a_lo, float* a_hi) {
    Q3C(loud_checked("q3_pcm_stage_loudness_consts", Q3_LOUD_OFF, target_mB, prior_mB));
    // in f64, rounded once
    if (T) *T = (float)pow(10.0, ((double)target_mB / 100.0 + 0.691) / 10.0);
    if (P) *P = (float)pow(10.0, (double)prior_mB / 2000.0);
    if (gate_abs) *gate_abs = (float)pow(10.0, (-70.0 + 0.691) / 10.0);
    if (a_lo) *a_lo = (float)pow(10.0, -2400.0 / 2000.0);
    if (a_hi) *a_hi = (float)pow(10.0, 2400.0 / 2000.0);
    return Q3_OK;
}
void out_loudness_at_rest(const OutSettings& o, float* mean_square, float* gain, int* blocks, int* gated) {
    if (gain) (void)q3_pcm_stage_loudness_consts(o.target_mB, o.prior_mB, nullptr, gain, nullptr, nullptr, nullptr);
    if (mean_square) *mean_square = 0.0f;
    if (blocks) *blocks = 0;
    if (gated) *gated = 0;
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
    dev_free(ps->tails); dev_free(ps->s_win); dev_free(ps->t_win); dev_free(ps->p_tab);
    for (PsRow& r : ps->rows) {
        dev_free(r.sil.state); dev_free(r.tp.state); dev_free(r.pt.tail); dev_free(r.ld.state); dev_free(r.mk.tab); dev_free(r.lv.tail);
        r.tp.lags[0].release(); r.tp.lags[1].release();
    }
    for (int s = 0; s < ST_N; ++s) { ps->buf[s].release(); ps->desc[s].release(); }
    ps->out.release();
    if (ps->st) (void)hipStreamDestroy(ps->st);
    delete ps;
}

int pcm_stage_rows(const q3_pcm_stage* ps) { return ps->R; }
const OutSettings& pcm_stage_settings(const q3_pcm_stage* ps, int row) { return ps->rows[(size_t)row].asked; }
void pcm_stage_reset(q3_pcm_stage* ps, int row) { ps->rows[(size_t)row].reset(); }

extern "C" q3_status q3_pcm_stage_reset(q3_pcm_stage* ps, int row) {
    if (!ps || row < 0 || row >= ps->R) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_reset: bad row");
    pcm_stage_reset(ps, row);
    return Q3_OK;
}

static q3_status pitch_checked(const char* who, int tempo, int cents) {
    Q3C(tempo_checked(who, tempo));
    if (cents < -PT_CENTS_MAX || cents > PT_CENTS_MAX)
        return set_err(Q3_INVALID_ARG, "%s: pitch %d cents out of range (%d..%d; 0 = off)", who, cents, -PT_CENTS_MAX, PT_CENTS_MAX);
    const int te = pitch_te(tempo, cents);
    if (te < TP_MIN || te > TP_MAX)
        return set_err(Q3_INVALID_ARG, "%s: tempo %d permille with a pitch of %d cents needs the stretcher at %d permille (%d..%d)", who, tempo, cents, te,
                       TP_MIN, TP_MAX);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_pitch_plan(int tempo_permille, int cents, int* tempo_eff, double* cents_realized) {
    Q3C(pitch_checked("q3_pcm_stage_pitch_plan", tempo_permille, cents));
    const int te = pitch_te(tempo_permille, cents);
    if (tempo_eff) *tempo_eff = te;
    if (cents_realized) *cents_realized = te == tempo_permille ? 0.0 : 1200.0 * log2((double)tempo_permille / (double)te);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_pitch_tables(float* sinc, size_t cap1, float* win, size_t cap2, int* S1, int* S2) {
    if (S1) *S1 = PT_S1;
    if (S2) *S2 = PT_S2;
    if (!sinc && !win) return Q3_OK;                               // S1 / S2 query
    if ((sinc && cap1 < (size_t)PT_SC_N) || (win && cap2 < (size_t)PT_W2_N))
        return set_err(Q3_INVALID_ARG, "q3_pcm_stage_pitch_tables: buffer too small (%d and %d floats needed)", PT_SC_N, PT_W2_N);
    std::vector<float> sc, w2;
    pitch_tables(sc, w2);
    if (sinc) memcpy(sinc, sc.data(), sc.size() * 4);
    if (win) memcpy(win, w2.data(), w2.size() * 4);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_pitch_count(int tempo_permille, int cents, size_t n_in_total, int ended, size_t* samples_24k) {
    Q3C(pitch_checked("q3_pcm_stage_pitch_count", tempo_permille, cents));
    if (!samples_24k) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_pitch_count: null argument");
    if (n_in_total > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_pitch_count: n_in_total above 2^48");
    const int te = pitch_te(tempo_permille, cents);
    long long f = 0, y = (long long)n_in_total;
    if (te != TP_OFF) tempo_frames(te, (long long)n_in_total, ended != 0, &f, &y);
    *samples_24k = (size_t)(te == tempo_permille ? y : pitch_emitted(tempo_permille, te, y, ended != 0));
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_bound_pitch(uint32_t sample_rate, int tempo_permille, int cents, int with_level, size_t n_in, size_t* n_out_max) {
    Q3C(pitch_checked("q3_pcm_stage_bound_pitch", tempo_permille, cents));
    if (n_in > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_bound_pitch: n_in above 2^48");
    return bound_through(sample_rate, tempo_permille, cents, with_level, 0, n_in, n_out_max);
}

// the blocks a row has stored once n samples have passed its loudness step
static long long loud_blocks(long long n) { return std::min<long long>(LD_HIST, std::max<long long>(0, n / LD_HOP - 3)); }

extern "C" q3_status q3_pcm_stage_loudness(q3_pcm_stage* ps, int row, float* mean_square, float* gain, int* blocks, int* gated) {
    if (!ps || row < 0 || row >= ps->R) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_loudness: bad row");
    const LoudStep& ld = ps->rows[(size_t)row].ld;
    if (ld.mode == Q3_LOUD_OFF) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_loudness: row %d has no loudness step (q3_pcm_stage_set_loudness)", row);
    if (ld.in == 0) { out_loudness_at_rest(ps->rows[(size_t)row].asked, mean_square, gain, blocks, gated); return Q3_OK; }
    float v[4];                                                    // A1 A2 M cg
    HIPC(hipSetDevice(ps->device));
    HIPC(q3_hipMemcpy(v, ld.state + (size_t)ld.cur * LD_STATE + LD_S_A1, sizeof(v), hipMemcpyDeviceToHost));
    int cg = 0; memcpy(&cg, &v[3], 4);
    if (mean_square) *mean_square = v[2];
    if (gain) *gain = v[0];
    if (blocks) *blocks = (int)loud_blocks(ld.in);
    if (gated) *gated = cg;
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_loudness_blocks(q3_pcm_stage* ps, int row, float* z, size_t cap, size_t* n) {
    if (!ps || row < 0 || row >= ps->R) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_loudness_blocks: bad row");
    if (!n) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_loudness_blocks: null argument");
    const LoudStep& ld = ps->rows[(size_t)row].ld;
    const long long nb = ld.mode == Q3_LOUD_OFF ? 0 : loud_blocks(ld.in);
    *n = (size_t)nb;
    if (nb == 0 || (!z && cap == 0)) return Q3_OK;                 // (no buffer: the count alone)
    if (!z || cap < (size_t)nb) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_loudness_blocks: %lld blocks, the buffer takes %zu", nb, cap);
    HIPC(hipSetDevice(ps->device));
    HIPC(q3_hipMemcpy(z, ld.state + 2 * (size_t)LD_STATE, (size_t)nb * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_tempo_lags(q3_pcm_stage* ps, int row, int64_t* k0, int* lags, size_t cap, size_t* n) {
    if (!ps || row < 0 || row >= ps->R) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_tempo_lags: bad row");
    if (!n) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_tempo_lags: null argument");
    const TempoStep& tp = ps->rows[(size_t)row].tp;
    *n = (size_t)tp.lag_n;
    if (k0) *k0 = (int64_t)tp.lag_k0;
    if (tp.lag_n == 0 || (!lags && cap == 0)) return Q3_OK;       // (no buffer: the count alone)
    if (!lags || cap < (size_t)tp.lag_n) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_tempo_lags: %lld lags, the buffer takes %zu", tp.lag_n, cap);
    HIPC(hipSetDevice(ps->device));
    HIPC(q3_hipMemcpy(lags, tp.lags[tp.lag_cur].dev, (size_t)tp.lag_n * sizeof(int), hipMemcpyDeviceToHost));
    return Q3_OK;
}

static q3_status silence_checked(const char* who, int threshold_mB, int edge_ms, int pause_ms) {
    if (threshold_mB != 0 && (threshold_mB < TR_THR_MIN || threshold_mB > TR_THR_MAX))
        return set_err(Q3_INVALID_ARG, "%s: threshold %d mB out of range (%d..%d; 0 = off)", who, threshold_mB, TR_THR_MIN, TR_THR_MAX);
    if (edge_ms < 0 || edge_ms > TR_EDGE_MAX || edge_ms % 10 != 0)
        return set_err(Q3_INVALID_ARG, "%s: edge of %d ms (0..%d, a multiple of 10)", who, edge_ms, TR_EDGE_MAX);
    if (pause_ms < TR_PAUSE_MIN || pause_ms > TR_PAUSE_MAX || pause_ms % 10 != 0)
        return set_err(Q3_INVALID_ARG, "%s: pause cap of %d ms (%d..%d, a multiple of 10)", who, pause_ms, TR_PAUSE_MIN, TR_PAUSE_MAX);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_silence_hold(int edge_ms, int pause_ms, size_t* samples) {
    Q3C(silence_checked("q3_pcm_stage_silence_hold", 0, edge_ms, pause_ms));
    if (!samples) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_silence_hold: null argument");
    *samples = tr_hold(tr_set(edge_ms, pause_ms));
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_bound_silence(uint32_t sample_rate, int tempo_permille, int cents, int with_level, int edge_ms, int pause_ms, size_t n_in,
                                                size_t* n_out_max) {
    Q3C(silence_checked("q3_pcm_stage_bound_silence", 0, edge_ms, pause_ms));
    if (n_in > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_bound_silence: n_in above 2^48");
    // a push hands on at most its own samples and what the row had retained: q3_pcm_stage_bound_pitch's refusals, for n_in + hold
    const size_t hold = tr_hold(tr_set(edge_ms, pause_ms));
    Q3C(pitch_checked("q3_pcm_stage_bound_pitch", tempo_permille, cents));
    if (n_in + hold > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_bound_pitch: n_in above 2^48");
    return bound_through(sample_rate, tempo_permille, cents, with_level, hold, n_in, n_out_max);
}

// the whole definition for one clip on the CPU: the same f32 operations in the same order as k_trim
extern "C" q3_status q3_silence_trim(const float* x, size_t n, int threshold_mB, int edge_ms, int pause_ms, float* y, size_t cap, size_t* n_y, int64_t* counts) {
    Q3C(silence_checked("q3_silence_trim", threshold_mB, edge_ms, pause_ms));
    if (threshold_mB == 0) return set_err(Q3_INVALID_ARG, "q3_silence_trim: threshold 0 is off: nothing to do");
    if ((n > 0 && !x) || !n_y) return set_err(Q3_INVALID_ARG, "q3_silence_trim: null argument");
    if (n > ((size_t)1 << 40)) return set_err(Q3_INVALID_ARG, "q3_silence_trim: n above 2^40");
    const TrSet t = tr_set(edge_ms, pause_ms);
    const float theta = tr_theta(threshold_mB);
    const long long N = (long long)n, NH = (N + TR_H - 1) / TR_H;
    std::vector<char> loud((size_t)NH, 0), act((size_t)NH, 0);
    for (long long h = 0; h < NH; ++h) {
        float p[64];
        for (int q = 0; q < 64; ++q) p[q] = 0.0f;
        for (int j = 0; j < TR_H; ++j) {
            const long long i = h * TR_H + j;
            float v = i < N ? x[i] : 0.0f;
            if (!std::isfinite(v)) v = 0.0f;
            p[j & 63] = h_add_rn(p[j & 63], h_mul_rn(v, v));
        }
        for (int d = 32; d >= 1; d >>= 1) for (int q = 0; q < d; ++q) p[q] = h_add_rn(p[q], p[q + d]);
        loud[(size_t)h] = p[0] > theta ? 1 : 0;
    }
    for (long long h = 0; h < NH; ++h)
        for (long long g = std::max<long long>(0, h - TR_G); g <= std::min(NH - 1, h + TR_G); ++g) act[(size_t)h] |= loud[(size_t)g];
    std::vector<std::pair<long long, long long>> ops;
    TrRun run = {-1, 0, 0, 0};
    tr_walk(run, 0, NH, true, N, t.E, t.P1, t.P2, [&](long long h) { return act[(size_t)h] != 0; },
            [&](long long a, long long b) { ops.push_back({a, b}); });
    long long kept = (long long)ops.size() * TR_H;
    if (!ops.empty() && (ops.back().first + 1) * TR_H > N) kept -= (ops.back().first + 1) * TR_H - N;
    *n_y = (size_t)kept;
    if (counts) { counts[0] = N; counts[1] = kept; counts[2] = run.lead; counts[3] = run.pause; counts[4] = run.trail; }
    if (!y && cap == 0) return Q3_OK;                              // (no buffer: the counts alone)
    if (!y || cap < (size_t)kept) return set_err(Q3_INVALID_ARG, "q3_silence_trim: %lld samples, the buffer takes %zu", kept, cap);
    float w[2 * TR_H];
    tr_window(w);
    for (long long i = 0; i < kept; ++i) {
        const long long k = i / TR_H, j = i - k * TR_H, a = ops[(size_t)k].first, b = ops[(size_t)k].second;
        y[i] = b < 0 ? x[a * TR_H + j] : h_add_rn(h_mul_rn(x[a * TR_H + j], w[TR_H + j]), h_mul_rn(x[b * TR_H + j], w[j]));
    }
    return Q3_OK;
}

// ---- the mark: carrier, host twin of k_mark, detector ----
static inline float h_sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
static q3_status mark_checked(const char* who, int strength_mB) {
    if (strength_mB < MK_STRENGTH_MIN || strength_mB > MK_STRENGTH_MAX)
        return set_err(Q3_INVALID_ARG, "%s: strength %d mB out of range (%d..%d)", who, strength_mB, MK_STRENGTH_MIN, MK_STRENGTH_MAX);
    return Q3_OK;
}
static inline float mark_strength(int strength_mB) { return (float)pow(10.0, (double)strength_mB / 2000.0); }

// Unit magnitude and a key-derived phase in every bin of the period whose frequency lies in the band, zero elsewhere; the inverse
// real DFT in f64 (the angle of bin k at sample n is 2 pi ((k n) mod P) / P, reduced in integers), scaled to unit RMS, rounded once
void mark_carrier(uint64_t key, float* c) {
    const double PI = 3.14159265358979323846;
    const uint64_t kk = synth_hash(key ^ synth_name_hash("q3.mark.carrier"));
    const int k_lo = (MK_BAND_LO * MK_P + (int)PS_RATE_IN - 1) / (int)PS_RATE_IN, k_hi = (MK_BAND_HI * MK_P) / (int)PS_RATE_IN;      // 86 .. 512
    std::vector<double> ct((size_t)MK_P), sn((size_t)MK_P), acc((size_t)MK_P, 0.0);
    for (int m = 0; m < MK_P; ++m) { const double a = 2.0 * PI * (double)m / (double)MK_P; ct[(size_t)m] = cos(a); sn[(size_t)m] = sin(a); }
    for (int k = k_lo; k <= k_hi; ++k) {
        const uint64_t z = synth_hash(kk + (uint64_t)k * 0x9E3779B97F4A7C15ULL);
        const double phi = 2.0 * PI * (double)(z >> 11) * (1.0 / 9007199254740992.0);
        const double cp = cos(phi), sp = sin(phi);
        for (int n = 0; n < MK_P; ++n) { const size_t m = (size_t)((k * n) & (MK_P - 1)); acc[(size_t)n] += ct[m] * cp - sn[m] * sp; }
    }
    double ss = 0.0;
    for (int n = 0; n < MK_P; ++n) ss += acc[(size_t)n] * acc[(size_t)n];
    const double inv = 1.0 / sqrt(ss / (double)MK_P);
    for (int n = 0; n < MK_P; ++n) c[n] = (float)(acc[(size_t)n] * inv);
}

extern "C" q3_status q3_mark_carrier(uint64_t key, float* c) {
    if (key == 0) return set_err(Q3_INVALID_ARG, "q3_mark_carrier: key 0 is off: there is no carrier");
    if (!c) return set_err(Q3_INVALID_ARG, "q3_mark_carrier: null argument");
    mark_carrier(key, c);
    return Q3_OK;
}

// the whole definition for one clip on the CPU: the same f32 operations in the same order as k_mark
extern "C" q3_status q3_mark_embed(const float* x, size_t n, uint64_t key, int strength_mB, float* y) {
    if (key == 0) return set_err(Q3_INVALID_ARG, "q3_mark_embed: key 0 is off: nothing to do");
    Q3C(mark_checked("q3_mark_embed", strength_mB));
    if (n > 0 && (!x || !y)) return set_err(Q3_INVALID_ARG, "q3_mark_embed: null argument");
    if (n > ((size_t)1 << 40)) return set_err(Q3_INVALID_ARG, "q3_mark_embed: n above 2^40");
    std::vector<float> c((size_t)MK_P);
    mark_carrier(key, c.data());
    const float s = mark_strength(strength_mB);
    float ramp[MK_H];
    for (int j = 0; j < MK_H; ++j) ramp[j] = (float)((double)j / 240.0);
    float r1 = 0.0f, r2 = 0.0f;
    for (size_t h0 = 0; h0 < n; h0 += MK_H) {
        const size_t cnt = std::min((size_t)MK_H, n - h0);
        float p[64];
        for (int q = 0; q < 64; ++q) p[q] = 0.0f;
        const float dg = h_sub_rn(r1, r2);
        for (size_t j = 0; j < cnt; ++j) {
            const float xv = x[h0 + j];
            const float v = std::isfinite(xv) ? xv : 0.0f;
            p[j & 63] = h_add_rn(p[j & 63], h_mul_rn(v, v));
            const float g = h_add_rn(r2, h_mul_rn(dg, ramp[j]));
            y[h0 + j] = h_add_rn(xv, h_mul_rn(h_mul_rn(s, g), c[(h0 + j) & (size_t)(MK_P - 1)]));
        }
        if (cnt < (size_t)MK_H) break;
        for (int d = 32; d >= 1; d >>= 1) for (int q = 0; q < d; ++q) p[q] = h_add_rn(p[q], p[q + d]);
        r2 = r1; r1 = sqrtf(h_mul_rn(p[0], (float)(1.0 / 240.0)));
    }
    return Q3_OK;
}

// rho[d] = sum_m F[m] c[(m + d) mod P] -> (max - mean) / std over the shifts and the shift of the maximum (the first of equals)
static void mark_score_of(const double* rho, double* score, int* offset) {
    double mean = 0.0, var = 0.0; int arg = 0;
    for (int d = 0; d < MK_P; ++d) { mean += rho[d]; if (rho[d] > rho[arg]) arg = d; }
    mean /= (double)MK_P;
    for (int d = 0; d < MK_P; ++d) var += (rho[d] - mean) * (rho[d] - mean);
    const double sd = sqrt(var / (double)MK_P);
    if (score) *score = sd > 0.0 ? (rho[arg] - mean) / sd : 0.0;
    if (offset) *offset = arg;
}
q3_status mark_score_f32(const float* rho, double* score, int* offset) {
    std::vector<double> r((size_t)MK_P);
    for (int d = 0; d < MK_P; ++d) r[(size_t)d] = (double)rho[d];
    mark_score_of(r.data(), score, offset);
    return Q3_OK;
}

extern "C" double q3_mark_score_detect(void) { return Q3_MARK_SCORE_DETECT; }

extern "C" q3_status q3_mark_detect(const float* z, size_t n, uint64_t key, double* score, int* offset) {
    if (key == 0) return set_err(Q3_INVALID_ARG, "q3_mark_detect: key 0 is off: there is no carrier");
    if (!z || (!score && !offset)) return set_err(Q3_INVALID_ARG, "q3_mark_detect: null argument");
    if (n < 2 * (size_t)MK_P) return set_err(Q3_INVALID_ARG, "q3_mark_detect: clip of %zu samples (at least %d: two periods at 24 kHz)", n, 2 * MK_P);
    if (n > ((size_t)1 << 40)) return set_err(Q3_INVALID_ARG, "q3_mark_detect: n above 2^40");
    std::vector<float> c((size_t)MK_P);
    mark_carrier(key, c.data());
    std::vector<double> F((size_t)MK_P, 0.0), c2(2 * (size_t)MK_P), rho((size_t)MK_P);
    for (size_t h0 = 0; h0 < n; h0 += MK_H) {                      // (the clip's last, partial hop against zeros)
        const size_t cnt = std::min((size_t)MK_H, n - h0);
        double e = 0.0;
        for (size_t j = 0; j < cnt; ++j) { const double v = std::isfinite(z[h0 + j]) ? (double)z[h0 + j] : 0.0; e += v * v; }
        const double r = std::max(sqrt(e / 240.0), 1e-4);
        for (size_t j = 0; j < cnt; ++j) { const double v = std::isfinite(z[h0 + j]) ? (double)z[h0 + j] : 0.0; F[(h0 + j) & (size_t)(MK_P - 1)] += v / r; }
    }
    for (int m = 0; m < 2 * MK_P; ++m) c2[(size_t)m] = (double)c[(size_t)(m & (MK_P - 1))];
    for (int d = 0; d < MK_P; ++d) {
        double a = 0.0;
        const double* cd = c2.data() + d;
        for (int m = 0; m < MK_P; ++m) a += F[(size_t)m] * cd[m];
        rho[(size_t)d] = a;
    }
    mark_score_of(rho.data(), score, offset);
    return Q3_OK;
}

// ---- settings (Settings) ----
// The checked edits: every range of an output setting, and the rule that ties a tempo to a pitch, is in the *_checked functions
// above and reaches every layer through these.
q3_status out_set_output(const char* who, OutSettings& o, uint32_t sample_rate, int format) {
    if (!fmt_ok(format)) return set_err(Q3_INVALID_ARG, "%s: format must be Q3_PCM_F32 (0), Q3_PCM_S16 (1), Q3_PCM_ULAW (2) or Q3_PCM_ALAW (3)", who);
    Rate r;
    Q3C(rate_checked(who, sample_rate, &r));
    o.rate = sample_rate; o.fmt = format;
    return Q3_OK;
}
q3_status out_set_tempo(const char* who, OutSettings& o, int tempo_permille) {
    Q3C(pitch_checked(who, tempo_permille, o.cents));
    o.tempo = tempo_permille;
    return Q3_OK;
}
q3_status out_set_pitch(const char* who, OutSettings& o, int cents) {
    Q3C(pitch_checked(who, o.tempo, cents));
    o.cents = cents;
    return Q3_OK;
}
q3_status out_set_level(const char* who, OutSettings& o, int gain_mB, int ceiling_mB) {
    Q3C(level_checked(who, gain_mB, ceiling_mB));
    o.gain_mB = gain_mB; o.ceil_mB = ceiling_mB;
    return Q3_OK;
}
q3_status out_set_loudness(const char* who, OutSettings& o, int mode, int target_mB, int prior_mB) {
    Q3C(loud_checked(who, mode, target_mB, prior_mB));
    o.loud = mode; o.target_mB = target_mB; o.prior_mB = prior_mB;
    return Q3_OK;
}
q3_status out_set_silence(const char* who, OutSettings& o, int threshold_mB, int edge_ms, int pause_ms) {
    Q3C(silence_checked(who, threshold_mB, edge_ms, pause_ms));
    o.sil_mB = threshold_mB; o.edge_ms = edge_ms; o.pause_ms = pause_ms;
    return Q3_OK;
}
q3_status out_set_mark(const char* who, OutSettings& o, uint64_t key, int strength_mB) {
    Q3C(mark_checked(who, strength_mB));
    o.mark_key = key; o.mark_mB = strength_mB;
    return Q3_OK;
}

// `o` (which came through the checked edits) onto a row. First everything that can fail — the tables and the row's states of the
// steps that `o` turns on, each made by the first call that needs it and kept from then on —, then the step fields, then the
// restart: a call that fails leaves the row as it was and where it was. The one exception is a silence step whose state has to
// grow: the old state is freed first (grow-only, and the row restarts anyway), so when the new one cannot be had the row is left
// with its silence step off (asked.sil_mB == 0) and otherwise untouched. That allocation comes last, so nothing fails behind it.
q3_status pcm_stage_apply(q3_pcm_stage* ps, int row, const char* who, const OutSettings& o) {
    PsRow& r = ps->rows[(size_t)row];
    Rate rate;
    Q3C(rate_checked(who, o.rate, &rate));                      // (before the device is touched)
    const float* taps = nullptr;
    if (o.rate != PS_RATE_IN) {
        auto it = ps->taps.find(o.rate);
        if (it == ps->taps.end()) {
            std::vector<float> t;
            taps_of(rate, t);
            char what[48];
            snprintf(what, sizeof(what), "tap table of %u Hz", o.rate);
            float* d = nullptr;
            Q3C(table_upload(ps, &d, t.data(), t.size(), who, what, "tap"));
            it = ps->taps.emplace(o.rate, d).first;
        }
        taps = it->second;
    }
    const int te = pitch_te(o.tempo, o.cents);
    if (te != TP_OFF) {
        if (!ps->t_win) {
            // periodic Hann, built in f64
            std::vector<float> w((size_t)TP_W);
            for (int j = 0; j < TP_W; ++j) w[(size_t)j] = (float)(0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * (double)j / (double)TP_W));
            Q3C(table_upload(ps, &ps->t_win, w.data(), w.size(), who, "window", "window"));
        }
        Q3C(row_state(ps, &r.tp.state, 2 * TP_STATE_BYTES, who, "state", row));
    }
    if (te != o.tempo) {
        if (!ps->p_tab) {
            std::vector<float> sc, w2;
            pitch_tables(sc, w2);
            sc.insert(sc.end(), w2.begin(), w2.end());
            Q3C(table_upload(ps, &ps->p_tab, sc.data(), sc.size(), who, "tables", "table"));
        }
        Q3C(row_state(ps, &r.pt.tail, 2 * (size_t)PS_TAPS * 4, who, "tail", row));
    }
    if (o.loud != Q3_LOUD_OFF) {
        if (!ps->o_coef_set) {
            // the K-weighting at 24 kHz: in f64, rounded once
            double sh[6], hp[6];
            Q3C(q3_loudness_kweight(PS_RATE_IN, sh, hp));
            const double c[10] = {sh[0], sh[1], sh[2], sh[4], sh[5], hp[0], hp[1], hp[2], hp[4], hp[5]};
            for (int i = 0; i < 10; ++i) ps->o_coef[i] = (float)c[i];
            ps->o_coef_set = true;
        }
        Q3C(row_state(ps, &r.ld.state, (2 * (size_t)LD_STATE + LD_HIST) * 4, who, "state", row));
    }
    if (o.mark_key != 0) {
        // the row's table and state, then its carrier where the key is new to the table (no push is in flight: each ends with a wait).
        // An upload that fails leaves the table without a carrier and the row with its mark step off, and otherwise untouched.
        Q3C(mark_checked(who, o.mark_mB));
        Q3C(row_state(ps, &r.mk.tab, ((size_t)MK_P + 2 * (size_t)MK_STATE) * 4, who, "carrier", row));
        if (r.mk.tab_key != o.mark_key) {
            std::vector<float> c((size_t)MK_P);
            mark_carrier(o.mark_key, c.data());
            r.mk.tab_key = 0;
            const hipError_t e = q3_hipMemcpy(r.mk.tab, c.data(), (size_t)MK_P * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) { r.mk.key = 0; r.asked.mark_key = 0; return set_err(Q3_HIP_ERROR, "%s: carrier upload: %s", who, hipGetErrorString(e)); }
            r.mk.tab_key = o.mark_key;
        }
    }
    const bool level = o.gain_mB != 0 || o.ceil_mB != 0;
    if (level) Q3C(row_state(ps, &r.lv.tail, 2 * (size_t)LV_TAIL_PITCH * 4, who, "state", row));
    const TrSet ts = tr_set(o.edge_ms, o.pause_ms);
    const size_t sil_copy = ((size_t)TR_ST * 8 + tr_state_floats(ts) * 4 + 15) & ~(size_t)15;
    if (o.sil_mB != 0) {
        if (!ps->s_win) {
            float w[2 * TR_H];
            tr_window(w);
            Q3C(table_upload(ps, &ps->s_win, w, 2 * TR_H, who, "seam weights", "weight"));
        }
        if (2 * sil_copy > r.sil.cap) {
            dev_free(r.sil.state); r.sil.state = nullptr; r.sil.cap = 0;
            const q3_status st = row_state(ps, &r.sil.state, 2 * sil_copy, who, "state", row);
            if (st != Q3_OK) { r.sil.thr = 0; r.asked.sil_mB = 0; return st; }
            r.sil.cap = 2 * sil_copy;
        }
    }
    r.asked = o;
    r.rs.sr = o.rate; r.rs.fmt = o.fmt; r.rs.r = rate; r.rs.taps = taps;
    r.pt.t = o.tempo; r.pt.te = r.tp.te = te;
    r.lv.on = level;
    (void)q3_pcm_stage_level_coeffs(o.gain_mB, o.ceil_mB, &r.lv.g, &r.lv.c);
    r.ld.mode = o.loud;
    (void)q3_pcm_stage_loudness_consts(o.target_mB, o.prior_mB, &r.ld.T, &r.ld.P, &r.ld.gate, &r.ld.lo, &r.ld.hi);
    r.mk.key = o.mark_key; r.mk.s = mark_strength(o.mark_mB);
    r.sil.thr = o.sil_mB; r.sil.set = ts; r.sil.theta = tr_theta(o.sil_mB);
    if (o.sil_mB != 0) r.sil.copy = sil_copy;
    pcm_stage_reset(ps, row);
    return Q3_OK;
}

// a public setter: the row's settings with one checked edit, applied
template <class Edit>
static q3_status stage_set(q3_pcm_stage* ps, int row, const char* who, Edit edit) {
    if (!ps || row < 0 || row >= ps->R) return set_err(Q3_INVALID_ARG, "%s: bad row", who);
    OutSettings o = ps->rows[(size_t)row].asked;
    Q3C(edit(who, o));
    return pcm_stage_apply(ps, row, who, o);
}
extern "C" q3_status q3_pcm_stage_set(q3_pcm_stage* ps, int row, uint32_t sample_rate, int format) {
    return stage_set(ps, row, "q3_pcm_stage_set", [&](const char* who, OutSettings& o) { return out_set_output(who, o, sample_rate, format); });
}
extern "C" q3_status q3_pcm_stage_set_tempo(q3_pcm_stage* ps, int row, int tempo_permille) {
    return stage_set(ps, row, "q3_pcm_stage_set_tempo", [&](const char* who, OutSettings& o) { return out_set_tempo(who, o, tempo_permille); });
}
extern "C" q3_status q3_pcm_stage_set_pitch(q3_pcm_stage* ps, int row, int cents) {
    return stage_set(ps, row, "q3_pcm_stage_set_pitch", [&](const char* who, OutSettings& o) { return out_set_pitch(who, o, cents); });
}
extern "C" q3_status q3_pcm_stage_set_level(q3_pcm_stage* ps, int row, int gain_mB, int ceiling_mB) {
    return stage_set(ps, row, "q3_pcm_stage_set_level", [&](const char* who, OutSettings& o) { return out_set_level(who, o, gain_mB, ceiling_mB); });
}
extern "C" q3_status q3_pcm_stage_set_loudness(q3_pcm_stage* ps, int row, int mode, int target_mB, int prior_mB) {
    return stage_set(ps, row, "q3_pcm_stage_set_loudness", [&](const char* who, OutSettings& o) { return out_set_loudness(who, o, mode, target_mB, prior_mB); });
}
extern "C" q3_status q3_pcm_stage_set_mark(q3_pcm_stage* ps, int row, uint64_t key, int strength_mB) {
    return stage_set(ps, row, "q3_pcm_stage_set_mark", [&](const char* who, OutSettings& o) { return out_set_mark(who, o, key, strength_mB); });
}
extern "C" q3_status q3_pcm_stage_set_silence(q3_pcm_stage* ps, int row, int threshold_mB, int edge_ms, int pause_ms) {
    return stage_set(ps, row, "q3_pcm_stage_set_silence", [&](const char* who, OutSettings& o) { return out_set_silence(who, o, threshold_mB, edge_ms, pause_ms); });
}

void out_silence_at_rest(int64_t* n_in, int64_t* n_out, int64_t* lead_cut, int64_t* pause_cut, int64_t* trail_cut) {
    for (int64_t* p : {n_in, n_out, lead_cut, pause_cut, trail_cut}) if (p) *p = 0;
}

extern "C" q3_status q3_pcm_stage_silence(q3_pcm_stage* ps, int row, int64_t* n_in, int64_t* n_out, int64_t* lead_cut, int64_t* pause_cut, int64_t* trail_cut) {
    if (!ps || row < 0 || row >= ps->R) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_silence: bad row");
    const SilStep& sil = ps->rows[(size_t)row].sil;
    if (sil.thr == 0) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_silence: row %d has no silence step (q3_pcm_stage_set_silence)", row);
    if (sil.in == 0) { out_silence_at_rest(n_in, n_out, lead_cut, pause_cut, trail_cut); return Q3_OK; }
    if (n_in) *n_in = sil.in;
    if (n_out) *n_out = sil.out;
    if (lead_cut) *lead_cut = sil.read[TR_S_LEAD];
    if (pause_cut) *pause_cut = sil.read[TR_S_PAUSE];
    if (trail_cut) *trail_cut = sil.read[TR_S_TRAIL];
    return Q3_OK;
}

// one step's descriptors of a push up from its pinned buffer, and its launch
template <class D, void (*K)(const D*)>
static hipError_t step_launch(PairBuf& b, const std::vector<D>& descs, dim3 grid, dim3 block, hipStream_t st) {
    if (descs.empty()) return hipSuccess;
    const hipError_t e = b.upload(descs.data(), descs.size() * sizeof(D), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(K, grid, block, 0, st, (const D*)b.dev);
    return hipGetLastError();
}

// The chain's first step, in a pass of its own: what leaves it depends on the data. The samples are on the device,
// readable by work on `st`. One descriptor upload, one k_trim launch (a workgroup per such row), the rows' counters back in one
// copy, a wait. Then those segments' walks say what the step kept and where it stands, in the stage's s buffer. Changes no row:
// k_trim writes the copy of the row's state that is not the current one.
static q3_status chain_prepass(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, hipStream_t st) {
    StepPlan& p = ps->plan;
    std::vector<TrDesc>& descs = p.sdesc;
    descs.clear(); p.sseg.clear();
    size_t bytes = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        const PsSeg& sg = segs[i]; const PsRow& r = ps->rows[(size_t)sg.row]; const SilStep& sil = r.sil;
        if (!step_on(r, ST_SIL) || r.ended) continue;
        p.seg[i].n_front = 0;                                      // (until the step hands something on)
        if (sg.n == 0 && !sg.last) continue;
        if (!sil.state || !ps->s_win) return set_err(Q3_INVALID_ARG, "pcm stage: row %d has a silence step and no state", sg.row);
        TrDesc d{};
        const TrSet& t = sil.set;
        d.base = sil.in; d.n_new = (int)sg.n; d.n_total = sil.in + (long long)sg.n; d.last = sg.last ? 1 : 0;
        d.c_old = d.base / TR_H; d.c_new = d.n_total / TR_H; d.c_end = sg.last ? (d.n_total + TR_H - 1) / TR_H : d.c_new;
        d.k_old = std::max<long long>(0, d.c_old - TR_G); d.k_new = sg.last ? d.c_end : std::max<long long>(0, d.c_new - TR_G);
        d.E = t.E; d.P1 = t.P1; d.P2 = t.P2; d.head = tr_head(t); d.theta = sil.theta;
        d.tail_lead = tr_tail_lead(t); d.tail_run = tr_tail_run(t);
        d.tail = sil.read[TR_S_RUN] == 0 ? d.tail_lead : d.tail_run;      // (what the last successful push left: the host's copy of the counters says which)
        // the hops a push can hand on: the ones it classifies and the ones the row had retained
        d.cap_ops = (int)(d.k_new - d.k_old) + (int)(tr_hold(t) / TR_H) + 2;
        d.fl_n = (int)(d.c_end - d.c_old) + 4;
        // its slice of s: kept samples | kept hops | flags
        p.seg[i].off[ST_SIL] = bytes;
        bytes += (((size_t)d.cap_ops * TR_H * 4 + 15) & ~(size_t)15) + (((size_t)d.cap_ops * 2 * sizeof(int) + 15) & ~(size_t)15) +
                 (((size_t)d.fl_n + (size_t)(d.k_new - d.k_old) + 15) & ~(size_t)15);
        d.src = sg.dev; d.win = ps->s_win;
        char* in = sil.state + (size_t)sil.cur * sil.copy; char* out = sil.state + (size_t)(sil.cur ^ 1) * sil.copy;
        d.st_in = sil.in > 0 ? (const long long*)in : nullptr; d.st_out = (long long*)out;
        d.tail_in = sil.in > 0 ? (const float*)(in + TR_ST * 8) : nullptr; d.tail_out = (float*)(out + TR_ST * 8);
        d.head_in = sil.in > 0 ? (const float*)(in + TR_ST * 8) + d.tail_run : nullptr; d.head_out = (float*)(out + TR_ST * 8) + d.tail_run;
        descs.push_back(d); p.sseg.push_back((int)i);
    }
    if (descs.empty()) return Q3_OK;
    HIPC(hipSetDevice(ps->device));
    DevBuf& s = ps->buf[ST_SIL]; PairBuf& sd = ps->desc[ST_SIL];
    Q3C(buf_reserve(ps, s, bytes));
    const size_t nd = descs.size(), db = (nd * sizeof(TrDesc) + 15) & ~(size_t)15, rb = nd * TR_ST * 8;
    Q3C(buf_reserve(ps, sd, db + rb));
    for (size_t k = 0; k < nd; ++k) {
        TrDesc& d = descs[k];
        char* at = s.dev + p.seg[(size_t)p.sseg[k]].off[ST_SIL];
        d.y = (float*)at; at += ((size_t)d.cap_ops * TR_H * 4 + 15) & ~(size_t)15;
        d.ops = (int*)at; at += ((size_t)d.cap_ops * 2 * sizeof(int) + 15) & ~(size_t)15;
        d.fl = (unsigned char*)at;
        d.res = (long long*)(sd.dev + db) + k * TR_ST;
    }
    HIPC((step_launch<TrDesc, k_trim>(sd, descs, dim3((unsigned)nd), dim3(TR_THREADS), st)));
    HIPC(hipMemcpyAsync(sd.host + db, sd.dev + db, rb, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    p.sres.assign((const long long*)(sd.host + db), (const long long*)(sd.host + db) + nd * TR_ST);
    for (size_t k = 0; k < nd; ++k) {
        const size_t i = (size_t)p.sseg[k];
        const PsSeg& sg = segs[i]; const SilStep& sil = ps->rows[(size_t)sg.row].sil; SegWalk& w = p.seg[i];
        const long long* res = &p.sres[k * TR_ST];
        const long long kept = res[TR_S_OUT] - sil.out;
        if (res[TR_S_OVER] || kept < 0 || kept > (long long)descs[k].cap_ops * TR_H)
            return set_err(Q3_HIP_ERROR, "pcm stage: the silence step of row %d kept %lld samples, its buffer takes %d hops", sg.row, kept, descs[k].cap_ops);
        w.sil = true; w.n_in[ST_SIL] = (long long)sg.n; w.n_out[ST_SIL] = kept;
        w.front = descs[k].y; w.n_front = kept;
    }
    return Q3_OK;
}

// whether a step that is on has what its _set_* allocates
static q3_status step_ready(const q3_pcm_stage* ps, const PsRow& r, int row, int s) {
    switch (s) {
    case ST_TEMPO: if (!r.tp.state) return set_err(Q3_INVALID_ARG, "pcm stage: row %d has a tempo and no state", row); break;
    case ST_PITCH: if (!r.pt.tail || !ps->p_tab) return set_err(Q3_INVALID_ARG, "pcm stage: row %d has a pitch and no state", row); break;
    case ST_LOUD: if (!r.ld.state) return set_err(Q3_INVALID_ARG, "pcm stage: row %d has a loudness step and no state", row); break;
    case ST_MARK: if (!r.mk.tab || r.mk.tab_key != r.mk.key) return set_err(Q3_INVALID_ARG, "pcm stage: row %d has a mark and no carrier", row); break;
    case ST_LEVEL: if (!r.lv.tail) return set_err(Q3_INVALID_ARG, "pcm stage: row %d has a level and no state", row); break;
    default: break;
    }
    return Q3_OK;
}
// One step's descriptor for one segment: w.n_in[s] new samples at src enter, w.n_out[s] leave into dst, the segment's slice of the
// step's push buffer (the resampler's: of the staging buffer). Moves src on to what the next step reads.
static q3_status step_fill(q3_pcm_stage* ps, PsPlan& plan, const PsSeg& sg, const SegWalk& w, int s, char* dst, const float*& src) {
    StepPlan& p = ps->plan; const PsRow& r = ps->rows[(size_t)sg.row];
    const int n_in = (int)w.n_in[s], n_out = (int)w.n_out[s];
    switch (s) {
    case ST_TEMPO: {
        const TempoStep& tp = r.tp;
        char* in = tp.state + (size_t)tp.cur * TP_STATE_BYTES; char* out = tp.state + (size_t)(tp.cur ^ 1) * TP_STATE_BYTES;
        TpDesc t{};
        t.src = src; t.hist_in = tp.in > 0 ? (const float*)(in + 16) : nullptr; t.hist_out = sg.last ? nullptr : (float*)(out + 16);
        // (the lag buffer that is written is the one the last successful push did not write: its lags stay readable)
        t.p_in = (const long long*)in; t.p_out = (long long*)out; t.lags = (int*)tp.lags[tp.lag_cur ^ 1].dev;
        t.y = (float*)dst; t.win = ps->t_win;
        t.base = tp.in; t.n_total = tp.in + n_in; t.hist_lo = tp_lo(tp.frames, tp.te); t.lo_next = tp_lo(w.frames, tp.te);
        t.k0 = tp.frames; t.k1 = w.frames; t.n_new = n_in; t.n_y = n_out; t.tempo = tp.te;
        if (!sg.last && t.n_total - t.lo_next > TP_HIST) return set_err(Q3_INVALID_ARG, "pcm stage: row %d would keep %lld samples", sg.row, t.n_total - t.lo_next);
        p.tdesc.push_back(t);
        break;
    }
    case ST_PITCH: {
        const PitchStep& pt = r.pt;
        PtDesc q{};
        q.src = src; q.n_new = n_in; q.base = pt.in; q.j0 = pt.out;
        q.tail_in = pt.in > 0 ? pt.tail + (size_t)pt.cur * PS_TAPS : nullptr;
        q.tail_out = sg.last ? nullptr : pt.tail + (size_t)(pt.cur ^ 1) * PS_TAPS;
        q.v = (float*)dst; q.n_v = n_out; q.sc = ps->p_tab; q.w2 = ps->p_tab + PT_SC_N;
        q.t = pt.t; q.te = pt.te; q.den1 = 20 * std::max(pt.t, pt.te);
        q.dq1 = (19 * PT_S1 * pt.te) / q.den1; q.dr1 = (19 * PT_S1 * pt.te) % q.den1;
        q.fc = (float)(0.95 * (pt.te < pt.t ? (double)pt.te / (double)pt.t : 1.0));
        p.pdesc.push_back(q);
        break;
    }
    case ST_LOUD: {
        if (n_in == 0) return Q3_OK;                               // (nothing passes: no descriptor, no flip)
        const LoudStep& ld = r.ld;
        LoDesc o{};
        o.src = src; o.w = (float*)dst;                            // (null where the row only meters: the samples pass as they are)
        o.st_in = ld.in > 0 ? ld.state + (size_t)ld.cur * LD_STATE : nullptr; o.st_out = ld.state + (size_t)(ld.cur ^ 1) * LD_STATE;
        o.hist = ld.state + 2 * (size_t)LD_STATE;
        o.base = ld.in; o.n_new = n_in; o.mode = ld.mode;
        o.T = ld.T; o.P = ld.P; o.gate = ld.gate; o.a_lo = ld.lo; o.a_hi = ld.hi;
        memcpy(o.coef, ps->o_coef, sizeof(o.coef));
        p.odesc.push_back(o);
        if (!dst) return Q3_OK;
        break;
    }
    case ST_MARK: {
        if (n_in > 0) {                                            // (nothing passes: no descriptor, no flip)
            const MarkStep& mk = r.mk;
            float* st = mk.tab + MK_P;
            MkDesc k{};
            k.src = src; k.y = (float*)dst; k.c = mk.tab;
            k.st_in = mk.in > 0 ? st + (size_t)mk.cur * MK_STATE : nullptr; k.st_out = st + (size_t)(mk.cur ^ 1) * MK_STATE;
            k.base = mk.in; k.n_new = n_in; k.s = mk.s;
            p.mdesc.push_back(k);
        }
        break;
    }
    case ST_LEVEL: {
        const LevelStep& lv = r.lv;
        LvDesc l{};
        l.src = src; l.n_new = n_in; l.base = lv.in; l.n_total = lv.in + n_in;
        l.tail_in = lv.in > 0 ? lv.tail + (size_t)lv.cur * LV_TAIL_PITCH : nullptr;
        l.tail_out = sg.last ? nullptr : lv.tail + (size_t)(lv.cur ^ 1) * LV_TAIL_PITCH;
        l.z = (float*)dst; l.o_base = lv.out; l.n_z = n_out; l.g = lv.g; l.c = lv.c;
        p.ldesc.push_back(l);
        break;
    }
    default: {
        const ResStep& rs = r.rs;
        float* tails = ps->tails + (size_t)sg.row * 2 * PS_TAPS;
        PsDesc d{};
        d.src = src; d.n_new = n_in; d.n_out = n_out; d.out = dst;
        d.base = rs.in; d.i0 = rs.out; d.L = rs.r.L; d.M = rs.r.M; d.fmt = rs.fmt; d.taps = rs.taps;
        if (rs.taps) { d.tail_in = rs.fresh ? nullptr : tails + (size_t)rs.cur * PS_TAPS; d.tail_out = tails + (size_t)(rs.cur ^ 1) * PS_TAPS; }
        plan.desc.push_back(d);
        break;
    }
    }
    p.tiles[s] = std::max(p.tiles[s], (n_out + PS_TILE - 1) / PS_TILE);
    src = (const float*)dst;
    return Q3_OK;
}
// The plan of a push, behind the silence step's pre-pass where a row has that step: walks every segment through the chain, lays its
// slices out in the steps' push buffers (4 floats aligned) and its output in the staging buffer (16 bytes aligned), and writes
// the descriptors. Changes no row. The buffers (and a row's lag buffer that is not the current one) may be reallocated: no push is
// in flight (each ends with a wait).
static q3_status chain_plan(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, PsPlan& plan) {
    StepPlan& p = ps->plan;
    plan.desc.clear(); plan.off.assign(segs.size(), 0); plan.count.assign(segs.size(), 0); plan.bytes = 0;
    p.tdesc.clear(); p.pdesc.clear(); p.odesc.clear(); p.mdesc.clear(); p.ldesc.clear();
    size_t floats[ST_N] = {0};
    for (int s = 0; s < ST_N; ++s) p.tiles[s] = 1;
    for (size_t i = 0; i < segs.size(); ++i) {
        const PsSeg& sg = segs[i]; const PsRow& r = ps->rows[(size_t)sg.row]; SegWalk& w = p.seg[i];
        w.runs = !r.ended && (w.n_front > 0 || sg.last);
        if (!w.runs) continue;
        chain_walk(r, ST_TEMPO, w.n_front, sg.last != 0, w);
        for (int s = ST_TEMPO; s < ST_RES; ++s) {
            if (!step_on(r, s)) continue;
            Q3C(step_ready(ps, r, sg.row, s));
            if (s == ST_LOUD && r.ld.mode != Q3_LOUD_NORMALIZE) continue;      // (a row that only meters writes no samples)
            w.off[s] = floats[s]; floats[s] += ((size_t)w.n_out[s] + 3) & ~(size_t)3;
        }
        plan.count[i] = (size_t)w.n_out[ST_RES];
        plan.off[i] = w.off[ST_RES] = plan.bytes;
        plan.bytes = (plan.bytes + plan.count[i] * fmt_bytes(r.rs.fmt) + 15) & ~(size_t)15;
    }
    Q3C(buf_reserve(ps, ps->out, plan.bytes));
    for (int s = ST_TEMPO; s < ST_RES; ++s) if (floats[s] > 0) Q3C(buf_reserve(ps, ps->buf[s], floats[s] * 4));
    for (size_t i = 0; i < segs.size(); ++i) {
        const PsSeg& sg = segs[i]; PsRow& r = ps->rows[(size_t)sg.row]; const SegWalk& w = p.seg[i];
        if (!w.runs) continue;
        if (step_on(r, ST_TEMPO) && w.frames > r.tp.frames) Q3C(buf_reserve(ps, r.tp.lags[r.tp.lag_cur ^ 1], (size_t)(w.frames - r.tp.frames) * sizeof(int)));
        const float* src = w.front;
        for (int s = ST_TEMPO; s < ST_N; ++s) {
            if (!step_on(r, s)) continue;
            char* dst = s == ST_RES ? ps->out.dev + w.off[s] : s == ST_LOUD && r.ld.mode != Q3_LOUD_NORMALIZE ? nullptr : ps->buf[s].dev + w.off[s] * 4;
            Q3C(step_fill(ps, plan, sg, w, s, dst, src));
        }
    }
    return Q3_OK;
}
// The launches of a push behind the pre-pass, in chain order: each step's descriptors go up from the stage's own pinned buffer (no
// push is in flight: each ends with a wait). The stretcher and the loudness step run a workgroup per row, the others one per tile
// of 256 outputs and row. The resampler's descriptors (plan.desc) are on the device already, at desc_dev.
static hipError_t chain_launch(q3_pcm_stage* ps, const PsPlan& plan, const PsDesc* desc_dev, hipStream_t st) {
    const StepPlan& p = ps->plan;
    hipError_t e = step_launch<TpDesc, k_tempo>(ps->desc[ST_TEMPO], p.tdesc, dim3((unsigned)p.tdesc.size()), dim3(TP_THREADS), st);
    if (e == hipSuccess) e = step_launch<PtDesc, k_pitch>(ps->desc[ST_PITCH], p.pdesc, dim3((unsigned)p.tiles[ST_PITCH], (unsigned)p.pdesc.size()), dim3(PS_TILE), st);
    if (e == hipSuccess) e = step_launch<LoDesc, k_loud>(ps->desc[ST_LOUD], p.odesc, dim3((unsigned)p.odesc.size()), dim3(LD_THREADS), st);
    if (e == hipSuccess) e = step_launch<MkDesc, k_mark>(ps->desc[ST_MARK], p.mdesc, dim3((unsigned)p.mdesc.size()), dim3(MK_THREADS), st);
    if (e == hipSuccess) e = step_launch<LvDesc, k_level>(ps->desc[ST_LEVEL], p.ldesc, dim3((unsigned)p.tiles[ST_LEVEL], (unsigned)p.ldesc.size()), dim3(PS_TILE), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pcm_stage, dim3((unsigned)p.tiles[ST_RES], (unsigned)plan.desc.size()), dim3(PS_TILE), 0, st, desc_dev);
    return hipGetLastError();
}
// the push has succeeded (the caller waited for its stream): every step that ran adds what the plan recorded, and flips
static void chain_commit(q3_pcm_stage* ps, const std::vector<PsSeg>& segs) {
    const StepPlan& p = ps->plan;
    for (size_t k = 0; k < p.sseg.size(); ++k) memcpy(ps->rows[(size_t)segs[(size_t)p.sseg[k]].row].sil.read, &p.sres[k * TR_ST], sizeof(SilStep::read));
    for (size_t i = 0; i < segs.size(); ++i) {
        const PsSeg& sg = segs[i]; PsRow& r = ps->rows[(size_t)sg.row]; const SegWalk& w = p.seg[i];
        auto add = [&](Totals& t, int s) { t.in += w.n_in[s]; t.out += w.n_out[s]; };
        if (w.sil) { add(r.sil, ST_SIL); r.sil.cur ^= 1; }
        if (!w.runs) continue;
        if (step_on(r, ST_TEMPO)) {
            TempoStep& tp = r.tp;
            tp.lag_cur ^= 1; tp.lag_k0 = tp.frames; tp.lag_n = w.frames - tp.frames;
            add(tp, ST_TEMPO); tp.frames = w.frames; tp.cur ^= 1;
        }
        if (step_on(r, ST_PITCH)) { add(r.pt, ST_PITCH); if (!sg.last) r.pt.cur ^= 1; }
        if (step_on(r, ST_LOUD) && w.n_in[ST_LOUD] > 0) { add(r.ld, ST_LOUD); r.ld.cur ^= 1; }
        if (step_on(r, ST_MARK) && w.n_in[ST_MARK] > 0) { add(r.mk, ST_MARK); r.mk.cur ^= 1; }
        if (step_on(r, ST_LEVEL)) { add(r.lv, ST_LEVEL); if (!sg.last) r.lv.cur ^= 1; }
        add(r.rs, ST_RES);
        if (r.rs.taps) { r.rs.cur ^= 1; r.rs.fresh = false; }
        if (sg.last) r.ended = true;
    }
}

// the stage's own stream, for pushes that do not come with one (created on the first: a stage behind a codec stream never needs it)
static q3_status own_stream(q3_pcm_stage* ps) {
    if (ps->st) return Q3_OK;
    q3_relax_capture_mode();
    const hipError_t e = hipStreamCreateWithFlags(&ps->st, hipStreamNonBlocking);
    if (e != hipSuccess) { ps->st = nullptr; return set_err(Q3_HIP_ERROR, "hipStreamCreateWithFlags: %s", hipGetErrorString(e)); }
    return Q3_OK;
}

// The push sequence (q3_engine.h says what each call is for). Every row at most once and in range is the entry points' business
// (pcm_stage_check_rows); here: n within max_push_samples — which applies to what enters the chain — and no samples for a row that
// was flushed.
q3_status pcm_stage_begin(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, PsPlan& plan) {
    StepPlan& p = ps->plan;
    p.seg.assign(segs.size(), SegWalk{}); p.sdesc.clear(); p.sseg.clear();
    plan.desc.clear(); plan.off.assign(segs.size(), 0); plan.count.assign(segs.size(), 0); plan.bytes = 0; plan.late = false;
    for (size_t i = 0; i < segs.size(); ++i) {
        const PsSeg& sg = segs[i]; const PsRow& r = ps->rows[(size_t)sg.row];
        if (sg.n > ps->max_push) return set_err(Q3_INVALID_ARG, "pcm stage: %zu samples for row %d, the stage takes %zu per push", sg.n, sg.row, ps->max_push);
        if (r.ended && sg.n > 0) return set_err(Q3_INVALID_ARG, "pcm stage: row %d was flushed (last): q3_pcm_stage_reset or _set restarts it", sg.row);
        p.seg[i].front = sg.dev; p.seg[i].n_front = (long long)sg.n;
        if (step_on(r, ST_SIL)) plan.late = true;
    }
    return plan.late ? Q3_OK : chain_plan(ps, segs, plan);
}
q3_status pcm_stage_run(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, PsPlan& plan, const PsDesc* desc_dev, hipStream_t st) {
    if (plan.late) {
        Q3C(chain_prepass(ps, segs, st));
        Q3C(chain_plan(ps, segs, plan));
        desc_dev = nullptr;                                        // (planned too late for the caller's descriptor block)
    }
    if (plan.desc.empty()) return Q3_OK;                           // (a silence step may have taken samples and kept none yet)
    if (!desc_dev) {
        // (the front of the resampler's staging holds the descriptors; q3_pcm_stage_push has put the samples behind them already)
        PairBuf& in = ps->desc[ST_RES];
        HIPC(in.upload(plan.desc.data(), plan.desc.size() * sizeof(PsDesc), st));
        desc_dev = (const PsDesc*)in.dev;
    }
    HIPC(chain_launch(ps, plan, desc_dev, st));
    if (plan.bytes > 0) HIPC(hipMemcpyAsync(ps->out.host, ps->out.dev, plan.bytes, hipMemcpyDeviceToHost, st));
    return Q3_OK;
}
void pcm_stage_finish(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, const PsPlan& plan, void* const* out_host, size_t* n_samples) {
    for (size_t i = 0; i < segs.size(); ++i) {
        if (n_samples) n_samples[i] = plan.count[i];
        if (out_host && out_host[i] && plan.count[i] > 0) memcpy(out_host[i], ps->out.host + plan.off[i], plan.count[i] * fmt_bytes(ps->rows[(size_t)segs[i].row].rs.fmt));
    }
    chain_commit(ps, segs);
}
q3_status pcm_stage_push_dev(q3_pcm_stage* ps, const std::vector<PsSeg>& segs, hipStream_t st, void* const* out_host, size_t* n_samples) {
    PsPlan plan;
    Q3C(pcm_stage_begin(ps, segs, plan));
    if (plan.late || !plan.desc.empty()) {
        HIPC(hipSetDevice(ps->device));
        if (!st) { Q3C(own_stream(ps)); st = ps->st; }
        Q3C(pcm_stage_run(ps, segs, plan, nullptr, st));
        if (!plan.desc.empty()) HIPC(hipStreamSynchronize(st));
    }
    pcm_stage_finish(ps, segs, plan, out_host, n_samples);
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
    if (step_on(r, ST_SIL)) {
        // what comes is known after the pre-pass alone; the cap covers the a-priori bound: the caps of the row's steps, in a row
        size_t b = 0;
        (void)resampler_bound(r.rs.sr, chain_cap(r, n), &b);
        return b;
    }
    SegWalk w{};
    chain_walk(r, ST_TEMPO, (long long)n, last != 0, w);
    return (size_t)w.n_out[ST_RES];
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
    PairBuf& in = ps->desc[ST_RES];                                // the resampler's descriptors | the rows' new samples
    HIPC(in.reserve(db + total * 4));
    std::vector<PsSeg> segs((size_t)n_rows);
    size_t off = db;
    for (int i = 0; i < n_rows; ++i) {
        if (n_in[i] > 0) memcpy(in.host + off, in_host[i], n_in[i] * 4);
        segs[(size_t)i] = {rows[i], (const float*)(in.dev + off), n_in[i], last ? last[i] : 0};
        off += ((n_in[i] + 3) & ~(size_t)3) * 4;
    }
    if (total > 0) HIPC(hipMemcpyAsync(in.dev + db, in.host + db, total * 4, hipMemcpyHostToDevice, ps->st));
    return pcm_stage_push_dev(ps, segs, ps->st, out_host, n_samples);
}
