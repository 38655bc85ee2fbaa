// q3_tone.hip — the output stage's tone step: a cascade of up to 8 biquad sections per row at 24 kHz
// (part of the q3_pcm_stage unit, included at its end: q3_pcm_stage.hip owns the row, the chain and the commit)
//
// The step stands behind the formant step and in front of the loudness step; it hands on as many samples as it takes, at once.
// A section is y = b0 x + s1; s1' = b1 x - a1 y + s2; s2' = b2 x - a2 y (transposed direct form II, a0 = 1): a recursion, and a
// lone lane that walks it pays the latency of two dependent f64 operations per sample and section. k_tone cuts the recursion open
// instead. With x = 0 the state moves by s' = A s, A = [[-a1, 1], [-a2, 0]], and the section is linear, so over a segment of len
// samples
//     state out = A^len (state in) + (state out from zero state),    y = (y from zero state) + (free response of the state in).
// One workgroup of one wave per (row, push). The push passes through LDS in chunks of 4096 samples, lane l owning samples
// 64 l .. 64 l + 63 of the chunk (segments at a pitch of 65 floats: the 64 lanes walk 64 different banks). Per section, in place:
//   1. every lane runs its segment from zero state, leaves that output in LDS and keeps the end state z;
//   2. the segments' maps s -> M s + z (M = A^64, A^len for the ragged last one, the identity behind it) are composed by an
//      inclusive scan across the wave — four DPP row shifts, then the two row broadcasts, a lane without a source composing with
//      the identity — after which lane l holds the map from the chunk's entry state to its own exit state;
//   3. the row's carried state enters: every lane forms its exit state, takes its neighbour's as its entry state (lane 0: the
//      carried one), and lane 63's is the chunk's, carried on;
//   4. every lane adds the free response of its entry state to its 64 outputs: two f64 recurrences that read no sample.
// The sections of a chunk follow each other in LDS; a lane touches its own segment alone, so the barriers are the two around
// the chunk's load and store. Samples are f32 between sections, states, coefficients and products f64 (poles of a 20 Hz section sit
// at radius 0.996: A^64 in f32 would be the error). The powers of A come from the host, in f64 per setting. The row's 16 doubles of
// state go back with ordinary vector stores. No scratch, no atomics, one launch for every row of a push that has the step.
#include "q3_engine.h"

namespace {
constexpr int TN_THREADS = 64, TN_PITCH = TN_SEG + 1, TN_LD = 16;
constexpr int TN_ROW_SHR = 0x110, TN_BCAST15 = 0x142, TN_BCAST31 = 0x143;      // DPP controls: row_shr:n is TN_ROW_SHR + n

// lane i takes v of the lane the control names, `id` where there is none (or where its row is not in `rows`)
template <int CTRL, int ROWS>
__device__ __forceinline__ double tn_dpp(double id, double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(id), __double2loint(v), CTRL, ROWS, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(id), __double2hiint(v), CTRL, ROWS, 0xf, false);
    return __hiloint2double(hi, lo);
}

struct TnMap { double m00, m01, m10, m11, z0, z1; };           // s -> M s + z

// c = c after p, p the map of the lane the control names: M = Mc Mp, z = Mc zp + zc
template <int CTRL, int ROWS>
__device__ __forceinline__ void tn_compose(TnMap& c) {
    TnMap p;
    p.m00 = tn_dpp<CTRL, ROWS>(1.0, c.m00); p.m01 = tn_dpp<CTRL, ROWS>(0.0, c.m01);
    p.m10 = tn_dpp<CTRL, ROWS>(0.0, c.m10); p.m11 = tn_dpp<CTRL, ROWS>(1.0, c.m11);
    p.z0 = tn_dpp<CTRL, ROWS>(0.0, c.z0); p.z1 = tn_dpp<CTRL, ROWS>(0.0, c.z1);
    TnMap r;
    r.m00 = fma(c.m00, p.m00, c.m01 * p.m10); r.m01 = fma(c.m00, p.m01, c.m01 * p.m11);
    r.m10 = fma(c.m10, p.m00, c.m11 * p.m10); r.m11 = fma(c.m10, p.m01, c.m11 * p.m11);
    r.z0 = fma(c.m00, p.z0, fma(c.m01, p.z1, c.z0));
    r.z1 = fma(c.m10, p.z0, fma(c.m11, p.z1, c.z1));
    c = r;
}

// Bounds: src and y hold n_new floats and c0 + j below is in [0, n_new); st_in / st_out hold 2 * TN_MAX doubles; a lane's segment is
// buf[65 lane .. 65 lane + 63], the last one ending at 4158 < 64 * 65.
__global__ __launch_bounds__(TN_THREADS) void k_tone(const TnDesc* __restrict__ descs) {
    __shared__ float buf[TN_SEG * TN_PITCH];
    __shared__ double carry[2 * TN_MAX];                         // the sections' states at the chunk's entry
    const TnDesc& d = descs[blockIdx.x];
    const float* __restrict__ src = d.src; float* __restrict__ y = d.y;
    const int n = d.n_new, ns = d.n_sec, lane = threadIdx.x;
    if (lane < 2 * TN_MAX) carry[lane] = d.st_in ? d.st_in[lane] : 0.0;
    float* seg = buf + lane * TN_PITCH;
    for (int c0 = 0; c0 < n; c0 += TN_CHUNK) {
        const int m = n - c0 < TN_CHUNK ? n - c0 : TN_CHUNK;
        for (int s0 = 0; s0 < m; s0 += TN_LD * TN_SEG) {            // TN_LD segments a round: the requests first, then the stores
            float v[TN_LD];
#pragma unroll
            for (int u = 0; u < TN_LD; ++u) { const int j = s0 + u * TN_SEG + lane; v[u] = j < m ? src[c0 + j] : 0.0f; }
#pragma unroll
            for (int u = 0; u < TN_LD; ++u) buf[((s0 >> 6) + u) * TN_PITCH + lane] = __builtin_isfinite(v[u]) ? v[u] : 0.0f;
        }
        __syncthreads();
        const int left = m - lane * TN_SEG, len = left < 0 ? 0 : (left < TN_SEG ? left : TN_SEG);
        for (int k = 0; k < ns; ++k) {
            const TnSec& sc = d.sec[k];
            const double b0 = sc.b0, b1 = sc.b1, b2 = sc.b2, na1 = -sc.a1, na2 = -sc.a2;
            double s1 = 0.0, s2 = 0.0;
            int i = 0;                                           // 1. the segment from zero state: eight samples a round, read first
            for (; i + 8 <= len; i += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = seg[i + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double x = (double)v[u];
                    const double o = fma(b0, x, s1);
                    s1 = fma(na1, o, fma(b1, x, s2));
                    s2 = fma(na2, o, b2 * x);
                    v[u] = (float)o;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) seg[i + u] = v[u];
            }
            for (; i < len; ++i) {
                const double x = (double)seg[i];
                const double o = fma(b0, x, s1);
                s1 = fma(na1, o, fma(b1, x, s2));
                s2 = fma(na2, o, b2 * x);
                seg[i] = (float)o;
            }
            TnMap mp = {1.0, 0.0, 0.0, 1.0, s1, s2};             // (an empty segment: the identity)
            if (len > 0) {
                const double* A = len == TN_SEG ? sc.A64 : sc.Ar;
                mp.m00 = A[0]; mp.m01 = A[1]; mp.m10 = A[2]; mp.m11 = A[3];
            }
            // 2. the inclusive scan, every lane of the wave in it
            tn_compose<TN_ROW_SHR + 1, 0xf>(mp); tn_compose<TN_ROW_SHR + 2, 0xf>(mp);
            tn_compose<TN_ROW_SHR + 4, 0xf>(mp); tn_compose<TN_ROW_SHR + 8, 0xf>(mp);
            tn_compose<TN_BCAST15, 0xa>(mp);                     // rows 1 and 3 behind rows 0 and 2
            tn_compose<TN_BCAST31, 0xc>(mp);                     // rows 2 and 3 behind rows 0 and 1
            // 3. the carried state in, the exit states one lane on
            const double c1 = carry[2 * k], c2 = carry[2 * k + 1];
            const double e1 = fma(mp.m00, c1, fma(mp.m01, c2, mp.z0)), e2 = fma(mp.m10, c1, fma(mp.m11, c2, mp.z1));
            double h1 = __shfl_up(e1, 1), h2 = __shfl_up(e2, 1);
            if (lane == 0) { h1 = c1; h2 = c2; }
            if (lane == TN_THREADS - 1) { carry[2 * k] = e1; carry[2 * k + 1] = e2; }
            for (i = 0; i + 8 <= len; i += 8) {                  // 4. the free response of the entry state
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = seg[i + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    v[u] = (float)((double)v[u] + h1);
                    const double t = h1;
                    h1 = fma(na1, t, h2);
                    h2 = na2 * t;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) seg[i + u] = v[u];
            }
            for (; i < len; ++i) {
                seg[i] = (float)((double)seg[i] + h1);
                const double t = h1;
                h1 = fma(na1, t, h2);
                h2 = na2 * t;
            }
        }
        __syncthreads();
        for (int s0 = 0; s0 < m; s0 += TN_LD * TN_SEG) {
            float v[TN_LD];
#pragma unroll
            for (int u = 0; u < TN_LD; ++u) v[u] = buf[((s0 >> 6) + u) * TN_PITCH + lane];
#pragma unroll
            for (int u = 0; u < TN_LD; ++u) { const int j = s0 + u * TN_SEG + lane; if (j < m) y[c0 + j] = v[u]; }
        }
        __syncthreads();
    }
    if (lane < 2 * TN_MAX) d.st_out[lane] = carry[lane];
}
}  // namespace

static const char* const TN_KINDS = "Q3_TONE_PEAK (0), _LOWSHELF (1), _HIGHSHELF (2), _HIGHPASS (3) or _LOWPASS (4)";

static q3_status tone_band_checked(const char* who, int i, const q3_tone_band& b) {
    if (b.kind < Q3_TONE_PEAK || b.kind > Q3_TONE_LOWPASS) return set_err(Q3_INVALID_ARG, "%s: band %d: kind must be %s, not %d", who, i, TN_KINDS, b.kind);
    if (b.freq_hz < TN_FREQ_MIN || b.freq_hz > TN_FREQ_MAX)
        return set_err(Q3_INVALID_ARG, "%s: band %d: freq_hz %d out of range (%d..%d)", who, i, b.freq_hz, TN_FREQ_MIN, TN_FREQ_MAX);
    const bool pass = b.kind == Q3_TONE_HIGHPASS || b.kind == Q3_TONE_LOWPASS;
    if (!pass && (b.gain_mB < -TN_GAIN_MAX || b.gain_mB > TN_GAIN_MAX))
        return set_err(Q3_INVALID_ARG, "%s: band %d: gain_mB %d out of range (%d..%d)", who, i, b.gain_mB, -TN_GAIN_MAX, TN_GAIN_MAX);
    if (b.q_milli < TN_Q_MIN || b.q_milli > TN_Q_MAX)
        return set_err(Q3_INVALID_ARG, "%s: band %d: q_milli %d out of range (%d..%d)", who, i, b.q_milli, TN_Q_MIN, TN_Q_MAX);
    return Q3_OK;
}

q3_status tone_checked(const char* who, int n_bands, const q3_tone_band* bands) {
    if (n_bands < 0 || n_bands > TN_MAX) return set_err(Q3_INVALID_ARG, "%s: n_bands %d out of range (0..%d; 0 = off)", who, n_bands, TN_MAX);
    if (n_bands > 0 && !bands) return set_err(Q3_INVALID_ARG, "%s: null bands", who);
    for (int i = 0; i < n_bands; ++i) Q3C(tone_band_checked(who, i, bands[i]));
    return Q3_OK;
}

// Audio EQ Cookbook (R. Bristow-Johnson): A = 10^(dB / 40), w0 = 2 pi f / rate, alpha = sin w0 / (2 Q)
extern "C" q3_status q3_tone_design(uint32_t rate, const q3_tone_band* band, double* ba) {
    if (!band || !ba) return set_err(Q3_INVALID_ARG, "q3_tone_design: null argument");
    if (rate < 8000 || rate > 192000) return set_err(Q3_INVALID_ARG, "q3_tone_design: sample rate %u out of range (8000..192000)", rate);
    Q3C(tone_band_checked("q3_tone_design", 0, *band));
    if (2 * (int64_t)band->freq_hz >= (int64_t)rate) return set_err(Q3_INVALID_ARG, "q3_tone_design: freq_hz %d is not below half the rate %u", band->freq_hz, rate);
    const double A = pow(10.0, (double)band->gain_mB / 4000.0), w0 = 2.0 * 3.14159265358979323846 * (double)band->freq_hz / (double)rate;
    const double cw = cos(w0), alpha = sin(w0) / (2.0 * ((double)band->q_milli / 1000.0)), sq = 2.0 * sqrt(A) * alpha;
    switch (band->kind) {
    case Q3_TONE_PEAK:
        ba[0] = 1.0 + alpha * A; ba[1] = -2.0 * cw; ba[2] = 1.0 - alpha * A;
        ba[3] = 1.0 + alpha / A; ba[4] = -2.0 * cw; ba[5] = 1.0 - alpha / A;
        break;
    case Q3_TONE_LOWSHELF:
        ba[0] = A * ((A + 1.0) - (A - 1.0) * cw + sq); ba[1] = 2.0 * A * ((A - 1.0) - (A + 1.0) * cw); ba[2] = A * ((A + 1.0) - (A - 1.0) * cw - sq);
        ba[3] = (A + 1.0) + (A - 1.0) * cw + sq; ba[4] = -2.0 * ((A - 1.0) + (A + 1.0) * cw); ba[5] = (A + 1.0) + (A - 1.0) * cw - sq;
        break;
    case Q3_TONE_HIGHSHELF:
        ba[0] = A * ((A + 1.0) + (A - 1.0) * cw + sq); ba[1] = -2.0 * A * ((A - 1.0) + (A + 1.0) * cw); ba[2] = A * ((A + 1.0) + (A - 1.0) * cw - sq);
        ba[3] = (A + 1.0) - (A - 1.0) * cw + sq; ba[4] = 2.0 * ((A - 1.0) - (A + 1.0) * cw); ba[5] = (A + 1.0) - (A - 1.0) * cw - sq;
        break;
    case Q3_TONE_HIGHPASS:
        ba[0] = (1.0 + cw) / 2.0; ba[1] = -(1.0 + cw); ba[2] = (1.0 + cw) / 2.0;
        ba[3] = 1.0 + alpha; ba[4] = -2.0 * cw; ba[5] = 1.0 - alpha;
        break;
    default:
        ba[0] = (1.0 - cw) / 2.0; ba[1] = 1.0 - cw; ba[2] = (1.0 - cw) / 2.0;
        ba[3] = 1.0 + alpha; ba[4] = -2.0 * cw; ba[5] = 1.0 - alpha;
        break;
    }
    return Q3_OK;
}

// What a row holds on the host for its bands (they came through tone_checked): per section TN_TAB doubles — b0 b1 b2 a1 a2 over a0,
// then A^1 .. A^64 row-major, multiplied up in long double and rounded once
void tone_plan(int n_bands, const q3_tone_band* bands, std::vector<double>& tab) {
    tab.assign((size_t)n_bands * TN_TAB, 0.0);
    for (int k = 0; k < n_bands; ++k) {
        double ba[6];
        (void)q3_tone_design(24000, &bands[k], ba);
        double* t = &tab[(size_t)k * TN_TAB];
        t[0] = ba[0] / ba[3]; t[1] = ba[1] / ba[3]; t[2] = ba[2] / ba[3]; t[3] = ba[4] / ba[3]; t[4] = ba[5] / ba[3];
        const long double a[4] = {-(long double)t[3], 1.0L, -(long double)t[4], 0.0L};
        long double p[4] = {a[0], a[1], a[2], a[3]};
        for (int j = 0; j < TN_SEG; ++j) {
            for (int i = 0; i < 4; ++i) t[5 + 4 * j + i] = (double)p[i];
            const long double q[4] = {a[0] * p[0] + a[1] * p[2], a[0] * p[1] + a[1] * p[3], a[2] * p[0] + a[3] * p[2], a[2] * p[1] + a[3] * p[3]};
            for (int i = 0; i < 4; ++i) p[i] = q[i];
        }
    }
}

// the sections of a push of n_new samples into a descriptor: the ragged segment, if there is one, has n_new % 64 samples
void tone_fill(const std::vector<double>& tab, int n_new, TnDesc& d) {
    d.n_new = n_new; d.n_sec = (int)(tab.size() / TN_TAB);
    const int rag = n_new % TN_SEG;
    for (int k = 0; k < d.n_sec; ++k) {
        const double* t = &tab[(size_t)k * TN_TAB]; TnSec& s = d.sec[k];
        s.b0 = t[0]; s.b1 = t[1]; s.b2 = t[2]; s.a1 = t[3]; s.a2 = t[4];
        memcpy(s.A64, t + 5 + 4 * (TN_SEG - 1), sizeof(s.A64));
        memcpy(s.Ar, t + 5 + 4 * (rag > 0 ? rag - 1 : TN_SEG - 1), sizeof(s.Ar));
    }
}

hipError_t tone_launch(const TnDesc* descs_dev, int n_rows, hipStream_t st) {
    hipLaunchKernelGGL(k_tone, dim3((unsigned)n_rows), dim3(TN_THREADS), 0, st, descs_dev);
    return hipGetLastError();
}
