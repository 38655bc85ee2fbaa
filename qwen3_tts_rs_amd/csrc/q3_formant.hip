// q3_formant.hip — the output stage's formant step: the spectral envelope of a row's stream warped by a factor
// (part of the q3_pcm_stage unit, included at its end: q3_pcm_stage.hip owns the row, the chain and the commit)
//
// The step stands directly behind the pitch step. Per frame of N = 1024 samples at hop H = 256 under a root-Hann window it takes
// the log-magnitude spectrum, keeps the cepstrum's quefrencies |n| <= 40 (the envelope E, harmonics left out), reads E at bin
// k * omega, and multiplies the spectrum by exp(clamp(E(k omega) - E(k), +-18 dB)): with omega = t / te the envelope that the pitch
// step moved by te / t is moved back, with omega = 1 / s it is moved by s on its own. The definition is include/q3tts.h's
// (q3_pcm_stage_set_formant); FM_N, FM_H, FM_LIFT and FM_CLAMP below are its N, H, 40 and ln 10^(18/20).
//
// Two kernels, a descriptor per row (FmDesc), the row the last grid dimension:
//   k_fm_frame   one workgroup of 128 threads per frame. A real sequence of 1024 is taken as 512 complex points z[j] = a[2j] + i a[2j+1].
//                The 512-point transform is one radix-2 decimation-in-frequency step — each lane forms its own four points of the
//                even half (wave 0: z[j] + z[j + 256]) or of the odd half (wave 1: (z[j] - z[j + 256]) W_512^j) straight from the
//                staged input, so the step costs no exchange — and then a 256-point radix-4 transform per wave: four points a lane in
//                registers, three exchanges through the wave's own padded LDS buffer (fm_pad). Z[2k + h] ends at ex[h][fm_pad(k)].
//                Four such transforms run per frame, all forward: (1) w x -> X, split into the 513 bins of the real transform;
//                (2) L = ln|X| extended evenly -> the cepstrum: L is real and even, so c = Re DFT(L) / N, and the lifter keeps
//                c[0..40] alone — 41 lanes split 41 bins; (3) the liftered cepstrum, again real and even -> E = Re DFT, the real part
//                of the split alone; (4) Y = g X through the transform run backwards (conj . fft . conj) -> the frame, windowed, to
//                the push's scratch [frame][1024]. Twiddles and window come from a table built on the host in f64 (FmTab): no
//                sincosf here; logf / expf are the library's accurate ones, their arguments formed by single rounded operations.
//   k_fm_ola     one workgroup per hop of 256 samples, a thread a sample: the row's kept partial sum (or 0), then the frames of this
//                push that cover the sample IN ASCENDING FRAME ORDER, each add rounded once. A sample whose four frames are done
//                leaves as half the sum; the others' sums go to the other copy of the row's state. Tile 0 also writes the next tail.
//                A sample has one owner: no atomics.
// The frame grid and the order of the sums are fixed by the sample index alone, so a row's output does not depend on how its input
// was cut into pushes. Ordinary launches on the caller's stream.
#include "q3_engine.h"

namespace {
constexpr int FM_THREADS = 128, FM_M = FM_N / 2, FM_K = FM_M + 1, FM_LIFT = 40;
constexpr int FM_XPAD = 320;                            // float2 of a wave's exchange buffer: fm_pad(255) = 315
constexpr float FM_CLAMP = (float)2.0723265836946414;   // ln 10^(18/20)

// tw[t] = exp(-2 pi i t / 1024); win[i] = sqrt(0.5 - 0.5 cos(2 pi i / 1024)): f64 on the host, rounded once
struct FmTab { float2 tw[FM_N]; float win[FM_N]; };

__device__ __forceinline__ int fm_pad(int p) { return p + ((p >> 4) << 2); }
__device__ __forceinline__ float2 fm_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// sample q of the row's stream into the step: zeros outside [0, n_total), the new samples from `base`, the kept tail (from sample
// 256 k0 - 768 on) below; a non-finite sample enters as 0. Bounds: src at [0, n_new); tail_in at k <= base - 1 - (256 k0 - 768) <= 1022.
__device__ __forceinline__ float fm_x_at(const FmDesc& d, long long q) {
    if (q < 0 || q >= d.n_total) return 0.0f;
    float v = 0.0f;
    if (q >= d.base) v = d.src[q - d.base];
    else {
        const long long k = q - (d.k0 * FM_H - (FM_N - FM_H));
        if (k >= 0 && d.tail_in) v = d.tail_in[k];
    }
    return __builtin_isfinite(v) ? v : 0.0f;
}

// The 256-point complex transform of a wave: v[r] = z[l + 64 r] in, Z[idx] at buf[fm_pad(idx)] out. Stage s works on groups of
// 4 q = 256, 64, 16, 4 points: lane l holds points (l / q) 4 q + l % q + q r, takes their 4-point transform, turns output r by
// W_4q^((l % q) r) = tw[(l % q) r 256 / q] (at most 63 * 3 * 4 < 1024) and leaves it where it was; the last stage stores position p
// at its base-4 digits reversed. Both waves of the block call it together (the barriers are the block's).
__device__ __forceinline__ void fm_fft256(float2 v[4], int l, float2* __restrict__ buf, const float2* __restrict__ tw) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int q = 64 >> (2 * s);
        const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
        const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), a3 = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
        float2 y[4];
        y[0] = make_float2(a0.x + a2.x, a0.y + a2.y);
        y[1] = make_float2(a1.x + a3.y, a1.y - a3.x);            // a1 - i a3
        y[2] = make_float2(a0.x - a2.x, a0.y - a2.y);
        y[3] = make_float2(a1.x - a3.y, a1.y + a3.x);            // a1 + i a3
        if (s < 3) {
            const int j = l & (q - 1), step = 256 / q;
#pragma unroll
            for (int r = 1; r < 4; ++r) y[r] = fm_cmul(y[r], tw[j * r * step]);
            const int base = (l / q) * 4 * q + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[fm_pad(base + q * r)] = y[r];
            __syncthreads();
            const int q2 = q >> 2, base2 = (l / q2) * 4 * q2 + (l & (q2 - 1));
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = buf[fm_pad(base2 + q2 * r)];
        } else {
            const int idx = ((l & 3) << 4) + (((l >> 2) & 3) << 2) + (l >> 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[fm_pad(idx + 64 * r)] = y[r];
            __syncthreads();
        }
    }
}

// The 512-point transform of the block: z[0 .. 512) in LDS (written before the caller's last barrier) -> Z[2 k + h] at
// ex[h][fm_pad(k)]. Wave h takes the half h of the radix-2 step; z is free again behind the first barrier inside.
__device__ __forceinline__ void fm_fft512(const float2* __restrict__ z, float2 (*ex)[FM_XPAD], const float2* __restrict__ tw, int tid) {
    const int l = tid & 63, h = tid >> 6;
    float2 v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = l + 64 * r;
        const float2 a = z[j], b = z[j + FM_M / 2];
        v[r] = h == 0 ? make_float2(a.x + b.x, a.y + b.y) : fm_cmul(make_float2(a.x - b.x, a.y - b.y), tw[2 * j]);
    }
    fm_fft256(v, l, ex[h], tw);
}
__device__ __forceinline__ float2 fm_z(const float2 (*ex)[FM_XPAD], int k) { return ex[k & 1][fm_pad((k >> 1) & 255)]; }
// bin k = 0 .. 512 of the real transform: A[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[512 - k]) / 2, O = -i (Z[k] - conj Z[512 - k]) / 2
__device__ __forceinline__ float2 fm_bin(const float2 (*ex)[FM_XPAD], const float2* __restrict__ tw, int k) {
    const float2 zk = fm_z(ex, k & (FM_M - 1)), zn = fm_z(ex, (FM_M - k) & (FM_M - 1));
    const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
    const float2 o = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
    const float2 t = fm_cmul(tw[k], o);
    return make_float2(e.x + t.x, e.y + t.y);
}

// Frame m = k0 + blockIdx.x of the row: samples [256 m - 768, 256 m + 256) -> fr[blockIdx.x][1024]. Bounds: a at [0, 1024); ex[h] at
// fm_pad(<= 255) = 315 < 320; Xs and Es at k <= 512; the gain reads Es[i + 1] with i <= 511 (u < 512); fr of frames below k1 alone.
__global__ __launch_bounds__(FM_THREADS) void k_fm_frame(const FmDesc* __restrict__ descs, const FmTab* __restrict__ tab) {
    __shared__ __align__(8) float a[FM_N];                       // a transform's input: 1024 reals = 512 complex points
    __shared__ __align__(8) float2 ex[2][FM_XPAD];
    __shared__ __align__(8) float2 Xs[FM_K];                     // X, then Y = g X
    __shared__ float Es[FM_K];
    __shared__ float cs[FM_LIFT + 1];
    const FmDesc d = descs[blockIdx.y];
    const long long m = d.k0 + blockIdx.x;
    if (m >= d.k1) return;                                       // (uniform over the block)
    const int tid = threadIdx.x;
    const long long s0 = m * FM_H - (FM_N - FM_H);
    for (int i = tid; i < FM_N; i += FM_THREADS) a[i] = mul_rn(tab->win[i], fm_x_at(d, s0 + i));
    __syncthreads();
    fm_fft512((const float2*)a, ex, tab->tw, tid);               // (1) X = DFT(w x)
    for (int k = tid; k < FM_K; k += FM_THREADS) {
        const float2 X = fm_bin(ex, tab->tw, k);
        Xs[k] = X;
        const float P = add_rn(mul_rn(X.x, X.x), mul_rn(X.y, X.y));
        const float L = mul_rn(0.5f, logf(fmaxf(P, 1e-12f)));
        a[k] = L;
        if (k > 0 && k < FM_M) a[FM_N - k] = L;                  // extended evenly
    }
    __syncthreads();
    fm_fft512((const float2*)a, ex, tab->tw, tid);               // (2) c = Re DFT(L) / N, the quefrencies the lifter keeps
    if (tid <= FM_LIFT) cs[tid] = mul_rn(fm_bin(ex, tab->tw, tid).x, 1.0f / FM_N);
    __syncthreads();
    for (int i = tid; i < FM_N; i += FM_THREADS) {
        const int n = i < FM_N - i ? i : FM_N - i;
        a[i] = n <= FM_LIFT ? cs[n] : 0.0f;
    }
    __syncthreads();
    fm_fft512((const float2*)a, ex, tab->tw, tid);               // (3) E = Re DFT(liftered c)
    for (int k = tid; k < FM_K; k += FM_THREADS) Es[k] = fm_bin(ex, tab->tw, k).x;
    __syncthreads();
    for (int k = tid; k < FM_K; k += FM_THREADS) {               // Y = g X, g from E at k omega against E at k
        const float u = mul_rn((float)k, d.omega);
        float Ew = Es[FM_M];
        if (u < (float)FM_M) {
            const float fl = floorf(u);
            const int i = (int)fl;
            Ew = fmaf(sub_rn(u, fl), sub_rn(Es[i + 1], Es[i]), Es[i]);
        }
        const float g = expf(fminf(fmaxf(sub_rn(Ew, Es[k]), -FM_CLAMP), FM_CLAMP));
        const float2 X = Xs[k];
        Xs[k] = make_float2(mul_rn(g, X.x), mul_rn(g, X.y));
    }
    __syncthreads();
    // (4) Z'[k] = (Y[k] + conj Y[512 - k]) + i conj(W^k) (Y[k] - conj Y[512 - k]); z = conj(fft(conj(Z'))) / N
    for (int k = tid; k < FM_M; k += FM_THREADS) {
        const float2 yk = Xs[k], yn = Xs[FM_M - k], tw = tab->tw[k];
        const float2 t = fm_cmul(make_float2(tw.x, -tw.y), make_float2(yk.x - yn.x, yk.y + yn.y));
        ((float2*)a)[k] = make_float2(((yk.x + yn.x) - t.y) * (1.0f / FM_N), -((yk.y - yn.y) + t.x) * (1.0f / FM_N));
    }
    __syncthreads();
    fm_fft512((const float2*)a, ex, tab->tw, tid);
    float2* out = (float2*)(d.fr + (size_t)blockIdx.x * FM_N);
    for (int j = tid; j < FM_M; j += FM_THREADS) {
        const float2 z = fm_z(ex, j), wv = *(const float2*)&tab->win[2 * j];
        out[j] = make_float2(mul_rn(z.x, wv.x), mul_rn(-z.y, wv.y));
    }
}

// Samples o_base + 256 blockIdx.x + tid of the row's output, up to pend = 256 k1 (with `last`: n_total). o_base = 256 max(0, k0 - 3)
// is where the row's kept partial sums start; they reach to 256 k0. Bounds: part_in at n - o_base < 768 for n < 256 k0; fr at frames
// k0 <= m < k1 and offsets n - (256 m - 768) in [0, 1024) for h <= m <= h + 3; y at n - o_base < n_y (final samples lie below
// 256 (k1 - 3), with `last` below n_total); part_out at n - 256 max(0, k1 - 3) in [0, 768); tail_out at fewer than 1024 floats.
__global__ __launch_bounds__(FM_H) void k_fm_ola(const FmDesc* __restrict__ descs) {
    const FmDesc d = descs[blockIdx.y];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && d.tail_out) {                         // what frame k1 will read of the stream so far
        const long long lo = d.k1 * FM_H - (FM_N - FM_H);
        const int cnt = (int)(d.n_total - lo);
        for (int i = tid; i < cnt; i += FM_H) d.tail_out[i] = fm_x_at(d, lo + i);
    }
    const long long h = d.o_base / FM_H + blockIdx.x, n = h * FM_H + tid;
    if (n >= (d.last ? d.n_total : d.k1 * FM_H)) return;
    float acc = n < d.k0 * FM_H ? d.part_in[n - d.o_base] : 0.0f;
    const long long m0 = h > d.k0 ? h : d.k0, m1 = h + 3 < d.k1 - 1 ? h + 3 : d.k1 - 1;
    for (long long m = m0; m <= m1; ++m) acc = add_rn(acc, d.fr[(size_t)(m - d.k0) * FM_N + (size_t)(n - (m * FM_H - (FM_N - FM_H)))]);
    if (d.last || h + 3 < d.k1) d.y[n - d.o_base] = mul_rn(0.5f, acc);
    else d.part_out[n - (d.k1 > 3 ? d.k1 - 3 : 0) * FM_H] = acc;
}
}  // namespace

long long formant_frames(long long F, bool ended) { return ended ? (F > 0 ? (F + FM_H - 1) / FM_H + 3 : 0) : F / FM_H; }
long long formant_emitted(long long F, bool ended) { return ended ? F : FM_H * std::max<long long>(0, F / FM_H - 3); }

float formant_omega(int t, int te, int keep, int fcents) {
    return (float)((keep ? (double)t / (double)te : 1.0) / pow(2.0, (double)fcents / 1200.0));
}

q3_status formant_checked(const char* who, int keep, int fcents) {
    if (keep != 0 && keep != 1) return set_err(Q3_INVALID_ARG, "%s: keep must be 0 or 1, not %d", who, keep);
    if (fcents < -FM_CENTS_MAX || fcents > FM_CENTS_MAX)
        return set_err(Q3_INVALID_ARG, "%s: formant shift %d cents out of range (%d..%d; 0 = none)", who, fcents, -FM_CENTS_MAX, FM_CENTS_MAX);
    return Q3_OK;
}

void formant_tables(std::vector<float>& tab) {
    tab.assign(FM_TAB_FLOATS, 0.0f);
    for (int i = 0; i < FM_N; ++i) {
        const double a = 2.0 * 3.14159265358979323846 * (double)i / (double)FM_N;
        tab[2 * (size_t)i] = (float)cos(a); tab[2 * (size_t)i + 1] = (float)-sin(a);
        tab[2 * (size_t)FM_N + (size_t)i] = (float)sqrt(0.5 - 0.5 * cos(a));
    }
}

hipError_t formant_launch(const FmDesc* descs_dev, int n_rows, int max_frames, int max_tiles, const float* tab_dev, hipStream_t st) {
    static_assert(sizeof(FmTab) == FM_TAB_FLOATS * 4, "the table's layout");
    if (max_frames > 0) {
        hipLaunchKernelGGL(k_fm_frame, dim3((unsigned)max_frames, (unsigned)n_rows), dim3(FM_THREADS), 0, st, descs_dev, (const FmTab*)tab_dev);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_fm_ola, dim3((unsigned)max_tiles, (unsigned)n_rows), dim3(FM_H), 0, st, descs_dev);
    return hipGetLastError();
}

extern "C" q3_status q3_pcm_stage_formant_count(size_t n_in_total, int ended, size_t* n_out) {
    if (!n_out) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_formant_count: null argument");
    if (n_in_total > ((size_t)1 << 48)) return set_err(Q3_INVALID_ARG, "q3_pcm_stage_formant_count: n_in_total above 2^48");
    *n_out = (size_t)formant_emitted((long long)n_in_total, ended != 0);
    return Q3_OK;
}

extern "C" q3_status q3_pcm_stage_formant_tables(float* twiddles, size_t cap1, float* window, size_t cap2, int* N, int* H) {
    if (N) *N = FM_N;
    if (H) *H = FM_H;
    if (!twiddles && !window) return Q3_OK;                      // N / H query
    if ((twiddles && cap1 < 2 * (size_t)FM_N) || (window && cap2 < (size_t)FM_N))
        return set_err(Q3_INVALID_ARG, "q3_pcm_stage_formant_tables: buffer too small (%d and %d floats needed)", 2 * FM_N, FM_N);
    std::vector<float> tab;
    formant_tables(tab);
    if (twiddles) memcpy(twiddles, tab.data(), 2 * (size_t)FM_N * 4);
    if (window) memcpy(window, tab.data() + 2 * (size_t)FM_N, (size_t)FM_N * 4);
    return Q3_OK;
}
