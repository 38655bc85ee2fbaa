// q3_denoise.hip — spectral noise suppression of a reference clip on the device
// (a unit of the engine: q3_engine.h says which holds what)
//
// The step between the intake (q3_intake.hip) and the two encoders: a q3_ref_audio's 24 kHz samples through a short-time Fourier
// analysis, a minimum-statistics noise floor, a Wiener-style gain with a floor of its own, and the overlap-add synthesis. The
// definition is include/q3tts.h's (q3_ref_audio_denoise); the constants below are its N, H, K, D and c_bias.
//
// Three kernels, each packed over the clips of a call (a descriptor per clip, the clip is the last grid dimension):
//   k_dn_analysis   four frames a workgroup, a wave a frame. The 896 samples the four frames share are staged once; a wave takes its
//                   windowed frame as 256 complex points z[j] = x[2j] + i x[2j+1], runs four radix-4 decimation-in-frequency stages
//                   with four points a lane in registers, exchanges between stages through its own LDS buffer (dn_pad: four
//                   float2 of padding per 16, which keeps the stride-64 and stride-16 exchanges off shared banks; the last,
//                   stride-4 one meets a bank four times), leaves Z in natural order and splits it into the 257 bins of the real
//                   transform. Twiddles and window come from a table built on the host in f64 (DnTab): no sincosf here.
//   k_dn_gain       a tile of 64 frames x 16 bins. The frames its minima reach — the window of 2 D + 1 valid frames is shifted, not
//                   shrunk, at a clip's ends, so at most 64 + 2 D rows — are staged from P with the box mean's halo (2 frames, 1
//                   bin), S is computed once per element into LDS, and the sliding minimum is a log-step doubling minimum over
//                   the time axis between two LDS buffers: W_2s[j] = min(W_s[j], W_s[j + s]) up to the largest power of two p
//                   below the window's length w, then min(W_p[a], W_p[a + w - p]).
//   k_dn_synthesis  a workgroup owns 13 hops (1664 samples) and transforms the 16 frames that cover them, four at a time, through
//                   the same transform run backwards (conj . fft . conj); each wave leaves its windowed frame in LDS and the
//                   thread that owns an output sample adds the four frames of a round IN ASCENDING FRAME ORDER into a register
//                   (the sample has one owner, so the accumulator needs no LDS and no atomics). 3 of 16 frames are transformed by
//                   two neighbours: the price of having no atomics.
//   k_dn_level      (q3_ref_audio_noise) sums lambda and P over 64 valid frames a workgroup in one fixed order.
// Every sum has one fixed order and no kernel reads another clip's data: a clip has the same bits alone and inside any batch.
// Ordinary launches on the intake's stream; workspace from the device-memory cache, back before the call returns.
#include "q3_engine.h"

namespace {
constexpr int DN_N = 512, DN_H = 128, DN_K = 257, DN_D = 94, DN_W = 2 * DN_D + 1;
constexpr float DN_BIAS = 4.0f;
constexpr long long DN_MAX_N = 24000LL * 120;
constexpr int DN_MAX_CLIPS = 64;
constexpr int DN_THREADS = 256;
constexpr int DN_XPAD = 320;                            // float2 of a wave's exchange buffer: dn_pad(255) = 315
constexpr int DG_TT = 64, DG_KB = 16;                   // k_dn_gain: frames x bins of a tile
constexpr int DG_RS = DG_TT + 2 * DN_D, DG_RP = DG_RS + 4, DG_PC = DG_KB + 2;
constexpr int DL_FR = 64;                               // k_dn_level: valid frames of a workgroup
constexpr int DS_R = 13, DS_OUT = DS_R * DN_H, DS_ROUNDS = (DS_R + 3) / 4, DS_Q = (DS_OUT + DN_THREADS - 1) / DN_THREADS;

// one clip of a launch (device-visible, 8-byte aligned)
struct DnDesc {
    const float* x; float* y;                           // the clip, the result (null: analysis only)
    float2* X; float* P; float* G; float* lam; float* part;     // [T][K] each; G / lam null: not written; part: k_dn_level's sums
    long long n;
    int T, lo, hi;
    float floor_g;                                      // 10^(-reduce_db / 20)
};
// tw[t] = exp(-2 pi i t / 512); win[i] = sqrt(0.5 - 0.5 cos(2 pi i / 512)): f64 on the host, rounded once
struct DnTab { float2 tw[DN_N]; float win[DN_N]; };

__device__ __forceinline__ int dn_pad(int p) { return p + ((p >> 4) << 2); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// The 256-point complex transform of a wave: v[r] = z[l + 64 r] in, Z[idx] at buf[dn_pad(idx)] out. Stage s works on groups of
// 4 q = 256, 64, 16, 4 points: lane l holds points (l / q) 4 q + l % q + q r, r = 0..3, takes their 4-point transform, turns output
// r by W_4q^((l % q) r) and leaves it where it was; after the last stage position p holds Z[p's base-4 digits reversed], and is
// stored there. Every wave of the block calls it together (the barriers are the block's).
__device__ __forceinline__ void dn_fft256(float2 v[4], int l, float2* __restrict__ buf, const float2* __restrict__ tw) {
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
            const int j = l & (q - 1), step = 2 * (64 / q);      // W_4q = tw[step]; j r step <= 63 * 3 * 2 < 512
#pragma unroll
            for (int r = 1; r < 4; ++r) y[r] = cmul(y[r], tw[j * r * step]);
            const int base = (l / q) * 4 * q + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[dn_pad(base + q * r)] = y[r];
            __syncthreads();
            const int q2 = q >> 2, base2 = (l / q2) * 4 * q2 + (l & (q2 - 1));
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = buf[dn_pad(base2 + q2 * r)];
        } else {
            const int idx = ((l & 3) << 4) + (((l >> 2) & 3) << 2) + (l >> 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[dn_pad(idx + 64 * r)] = y[r];
            __syncthreads();
        }
    }
}

// X[m][k] and P[m][k] of four frames. Bounds: x is read at [0, n) alone; xs at w 128 + 2 j + 1 <= 3 * 128 + 511 < 896; X / P of
// frames below T alone.
__global__ __launch_bounds__(DN_THREADS) void k_dn_analysis(const DnDesc* __restrict__ descs, const DnTab* __restrict__ tab) {
    __shared__ __align__(8) float xs[4 * DN_H + DN_N - DN_H];
    __shared__ __align__(8) float2 ex[4][DN_XPAD];
    const DnDesc d = descs[blockIdx.y];
    const int m0 = blockIdx.x * 4;
    if (m0 >= d.T) return;                                       // (uniform over the block)
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const long long s0 = (long long)m0 * DN_H - (DN_N - DN_H);
    for (int i = tid; i < 4 * DN_H + DN_N - DN_H; i += DN_THREADS) {
        const long long g = s0 + i;
        xs[i] = (g >= 0 && g < d.n) ? d.x[g] : 0.0f;
    }
    __syncthreads();
    float2 v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = l + 64 * r;
        const float2 xx = *(const float2*)&xs[w * DN_H + 2 * j], wv = *(const float2*)&tab->win[2 * j];
        v[r] = make_float2(xx.x * wv.x, xx.y * wv.y);
    }
    dn_fft256(v, l, ex[w], tab->tw);
    const int m = m0 + w;
    if (m >= d.T) return;                                        // (no barrier follows)
    // X[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[256 - k]) / 2, O = -i (Z[k] - conj Z[256 - k]) / 2; k = 256 is lane 0's
    for (int k = l; k < DN_K; k += 64) {
        const float2 zk = ex[w][dn_pad(k & 255)], zn = ex[w][dn_pad((256 - k) & 255)];
        const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
        const float2 o = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
        const float2 t = cmul(tab->tw[k], o);
        const float2 X = make_float2(e.x + t.x, e.y + t.y);
        d.X[(size_t)m * DN_K + k] = X;
        d.P[(size_t)m * DN_K + k] = X.x * X.x + X.y * X.y;
    }
}

// G[m][k] (and lambda[m][k]) of a tile. Rows of the tile in LDS: frames bot .. top, bot = min(a(m0), m0), top = max(b(m1), m1), a / b
// the window's ends of the definition; top - bot + 1 <= 64 + 2 D = DG_RS (interior: a(m1) - a(m0) <= m1 - m0; first tile: b = lo +
// 2 D = 191; last tile: m1 - a(m0) <= 191). P rows bot - 2 .. top + 2 and bins k0 - 1 .. k0 + 16, zeros where there is no entry.
__global__ __launch_bounds__(DN_THREADS) void k_dn_gain(const DnDesc* __restrict__ descs) {
    __shared__ float Pb[DG_RP][DG_PC];
    __shared__ float Wa[DG_RS][DG_KB], Wb[DG_RS][DG_KB];
    const DnDesc d = descs[blockIdx.z];
    const int m0 = blockIdx.x * DG_TT, k0 = blockIdx.y * DG_KB, tid = threadIdx.x;
    if (m0 >= d.T) return;                                       // (uniform over the block)
    const int m1 = min(m0 + DG_TT - 1, d.T - 1);
    if (d.hi < d.lo) {                                           // too short to estimate: G = 1
        for (int i = tid; i < DG_TT * DG_KB; i += DN_THREADS) {
            const int m = m0 + i / DG_KB, k = k0 + i % DG_KB;
            if (m <= m1 && k < DN_K && d.G) d.G[(size_t)m * DN_K + k] = 1.0f;
        }
        return;
    }
    const int span = min(DN_W, d.hi - d.lo + 1);                 // the window's length
    const int a0 = span < DN_W ? d.lo : max(d.lo, min(m0 - DN_D, d.hi - 2 * DN_D));
    const int a1 = span < DN_W ? d.lo : max(d.lo, min(m1 - DN_D, d.hi - 2 * DN_D));
    const int bot = min(a0, m0), top = max(a1 + span - 1, m1), rows = top - bot + 1;
    for (int i = tid; i < (rows + 4) * DG_PC; i += DN_THREADS) {
        const int r = i / DG_PC, c = i - r * DG_PC, m = bot - 2 + r, k = k0 - 1 + c;
        Pb[r][c] = (m >= 0 && m < d.T && k >= 0 && k < DN_K) ? d.P[(size_t)m * DN_K + k] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < rows * DG_KB; i += DN_THREADS) {
        const int r = i / DG_KB, c = i % DG_KB, m = bot + r, k = k0 + c;
        float s = 0.0f;
        if (k < DN_K) {
#pragma unroll
            for (int dr = 0; dr < 5; ++dr) s += (Pb[r + dr][c] + Pb[r + dr][c + 1]) + Pb[r + dr][c + 2];
            const int cnt = (min(m + 2, d.T - 1) - max(m - 2, 0) + 1) * (min(k + 1, DN_K - 1) - max(k - 1, 0) + 1);
            s = __fdiv_rn(s, (float)cnt);
        }
        Wa[r][c] = s;
    }
    __syncthreads();
    float own[DG_TT * DG_KB / DN_THREADS];                       // S of this thread's outputs, before the minima overwrite it
#pragma unroll
    for (int q = 0; q < DG_TT * DG_KB / DN_THREADS; ++q) {
        const int i = tid + DN_THREADS * q, m = m0 + i / DG_KB;
        own[q] = m <= m1 ? Wa[m - bot][i % DG_KB] : 0.0f;
    }
    float (*cur)[DG_KB] = Wa;
    float (*nxt)[DG_KB] = Wb;
    int p = 1;
    for (; 2 * p <= span; p *= 2) {                              // (uniform over the block)
        for (int i = tid; i < rows * DG_KB; i += DN_THREADS) {
            const int r = i / DG_KB, c = i % DG_KB;
            nxt[r][c] = r + p < rows ? fminf(cur[r][c], cur[r + p][c]) : cur[r][c];
        }
        __syncthreads();
        float (*t)[DG_KB] = cur; cur = nxt; nxt = t;
    }
#pragma unroll
    for (int q = 0; q < DG_TT * DG_KB / DN_THREADS; ++q) {
        const int i = tid + DN_THREADS * q, m = m0 + i / DG_KB, c = i % DG_KB, k = k0 + c;
        if (m > m1 || k >= DN_K) continue;
        const int a = (span < DN_W ? d.lo : max(d.lo, min(m - DN_D, d.hi - 2 * DN_D))) - bot;     // a + span - 1 <= top - bot
        const float lam = DN_BIAS * fminf(cur[a][c], cur[a + span - p][c]);
        // xi / (1 + xi) with xi = r - 1 > 0 is 1 - 1 / r, which also holds when r is infinite
        const float r = __fdiv_rn(own[q], fmaxf(lam, 1e-30f));
        const float g = r > 1.0f ? 1.0f - __fdiv_rn(1.0f, r) : 0.0f;
        if (d.G) d.G[(size_t)m * DN_K + k] = fmaxf(g, d.floor_g);
        if (d.lam) d.lam[(size_t)m * DN_K + k] = lam;
    }
}

// part[2 c], part[2 c + 1] = the sums of lambda and of P over the bins of valid frames lo + 64 c .. : a thread sums its bins frame
// after frame, the block joins them by halving. Frames lo .. hi alone are read.
__global__ __launch_bounds__(DN_THREADS) void k_dn_level(const DnDesc* __restrict__ descs) {
    __shared__ float red[2][DN_THREADS];
    const DnDesc d = descs[blockIdx.y];
    const int f0 = d.lo + blockIdx.x * DL_FR, tid = threadIdx.x;
    if (f0 > d.hi) return;                                       // (uniform over the block)
    const int f1 = min(f0 + DL_FR - 1, d.hi);
    float sl = 0.0f, sp = 0.0f;
    for (int m = f0; m <= f1; ++m)
        for (int k = tid; k < DN_K; k += DN_THREADS) { sl += d.lam[(size_t)m * DN_K + k]; sp += d.P[(size_t)m * DN_K + k]; }
    red[0][tid] = sl; red[1][tid] = sp;
    __syncthreads();
    for (int o = DN_THREADS / 2; o >= 1; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { d.part[2 * blockIdx.x] = red[0][0]; d.part[2 * blockIdx.x + 1] = red[1][0]; }
}

// y of hops h0 .. h0 + 12. Round j transforms frames h0 + 4 j + w; frame f covers the tile's samples (f - h0 - 3) 128 .. + 511.
// Bounds: X / G of frames below T alone; ex[w] at k <= 256 < 320 while staging; fo at 0 <= i < 512; y below n.
__global__ __launch_bounds__(DN_THREADS) void k_dn_synthesis(const DnDesc* __restrict__ descs, const DnTab* __restrict__ tab) {
    __shared__ __align__(8) float2 ex[4][DN_XPAD];
    __shared__ __align__(8) float fo[4][DN_N];
    const DnDesc d = descs[blockIdx.y];
    const int h0 = blockIdx.x * DS_R;
    if ((long long)h0 * DN_H >= d.n) return;                     // (uniform over the block)
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    float acc[DS_Q];
#pragma unroll
    for (int q = 0; q < DS_Q; ++q) acc[q] = 0.0f;
    for (int j = 0; j < DS_ROUNDS; ++j) {
        const int f = h0 + 4 * j + w;
        for (int k = l; k < DN_K; k += 64) {                     // Y = G X, zeros for a frame the clip does not have
            float2 y = make_float2(0.0f, 0.0f);
            if (f < d.T) {
                const float2 X = d.X[(size_t)f * DN_K + k];
                const float g = d.G[(size_t)f * DN_K + k];
                y = make_float2(g * X.x, g * X.y);
            }
            ex[w][k] = y;
        }
        __syncthreads();
        // Z'[k] = (Y[k] + conj Y[256 - k]) + i conj(W^k) (Y[k] - conj Y[256 - k]); z = conj(fft(conj(Z'))) / 512
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = l + 64 * r;
            const float2 yk = ex[w][k], yn = ex[w][256 - k];
            const float2 tw = tab->tw[k];
            const float2 t = cmul(make_float2(tw.x, -tw.y), make_float2(yk.x - yn.x, yk.y + yn.y));
            v[r] = make_float2(((yk.x + yn.x) - t.y) * (1.0f / DN_N), -((yk.y - yn.y) + t.x) * (1.0f / DN_N));
        }
        __syncthreads();
        dn_fft256(v, l, ex[w], tab->tw);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int jj = l + 64 * c;
            const float2 z = ex[w][dn_pad(jj)], wv = *(const float2*)&tab->win[2 * jj];
            *(float2*)&fo[w][2 * jj] = make_float2(z.x * wv.x, -z.y * wv.y);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < DS_Q; ++q) {
            const int s = tid + DN_THREADS * q;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) {                     // ascending frame order
                const int i = s - (4 * j + ww - 3) * DN_H;
                if (s < DS_OUT && h0 + 4 * j + ww < d.T && i >= 0 && i < DN_N) acc[q] = add_rn(acc[q], fo[ww][i]);
            }
        }
        __syncthreads();                                         // (fo and ex are written again)
    }
#pragma unroll
    for (int q = 0; q < DS_Q; ++q) {
        const int s = tid + DN_THREADS * q;
        const long long g = (long long)h0 * DN_H + s;
        if (s < DS_OUT && g < d.n) d.y[g] = 0.5f * acc[q];
    }
}

const DnTab& dn_tab() {
    static const DnTab* t = [] {
        DnTab* p = new DnTab();
        for (int i = 0; i < DN_N; ++i) {
            const double a = 2.0 * M_PI * (double)i / (double)DN_N;
            p->tw[i] = make_float2((float)cos(a), (float)-sin(a));
            p->win[i] = (float)sqrt(0.5 - 0.5 * cos(a));
        }
        return p;
    }();
    return *t;
}

struct DnPlan { int T = 0, lo = 3, hi = 0; size_t bytes = 0; };
DnPlan dn_plan(long long n) {
    DnPlan p;
    p.T = (int)((n + DN_H - 1) / DN_H) + 3; p.hi = p.T - 4;
    p.bytes = (size_t)p.T * DN_K * 16;                           // X (8) + P (4) + G (4) a bin: a multiple of 16
    return p;
}
size_t up16d(size_t v) { return (v + 15) & ~(size_t)15; }

// descriptors | tables | per clip X, P, G or lambda, the sums: one block, one upload, the launches, a wait. outs: the new objects
// with their samples allocated (denoise), or null (noise: sums[2 i], sums[2 i + 1] = the sums of lambda and P over valid frames).
q3_status dn_run(int device, int n, q3_ref_audio* const* in, const float* floors, q3_ref_audio* const* outs, double* sums, char** block) {
    std::vector<DnPlan> plans((size_t)n);
    std::vector<size_t> off((size_t)n), part_off((size_t)n);
    std::vector<int> chunks((size_t)n, 0);
    size_t bytes = up16d((size_t)n * sizeof(DnDesc));
    const size_t tab_off = bytes; bytes += up16d(sizeof(DnTab));
    const size_t host_bytes = bytes;
    int max_T = 1; long long max_n = 1; int max_chunks = 1;
    for (int i = 0; i < n; ++i) {
        plans[(size_t)i] = dn_plan(in[i]->n);
        off[(size_t)i] = bytes; bytes += plans[(size_t)i].bytes;
        if (!outs) {
            chunks[(size_t)i] = (plans[(size_t)i].hi - plans[(size_t)i].lo + DL_FR) / DL_FR;
            part_off[(size_t)i] = bytes; bytes += up16d((size_t)chunks[(size_t)i] * 8);
        }
        max_T = std::max(max_T, plans[(size_t)i].T); max_n = std::max(max_n, (long long)in[i]->n); max_chunks = std::max(max_chunks, chunks[(size_t)i]);
    }
    q3_relax_capture_mode();
    HIPC(dev_malloc((void**)block, bytes));
    char* dev = *block;
    std::vector<char> host(host_bytes);
    DnDesc* desc = (DnDesc*)host.data();
    for (int i = 0; i < n; ++i) {
        const DnPlan& p = plans[(size_t)i];
        const size_t tk = (size_t)p.T * DN_K;
        DnDesc& d = desc[i];
        d.x = in[i]->dev; d.y = outs ? outs[i]->dev : nullptr;
        d.X = (float2*)(dev + off[(size_t)i]); d.P = (float*)(dev + off[(size_t)i] + tk * 8);
        float* third = (float*)(dev + off[(size_t)i] + tk * 12);
        d.G = outs ? third : nullptr; d.lam = outs ? nullptr : third;
        d.part = outs ? nullptr : (float*)(dev + part_off[(size_t)i]);
        d.n = in[i]->n; d.T = p.T; d.lo = p.lo; d.hi = p.hi; d.floor_g = floors ? floors[i] : 1.0f;
    }
    memcpy(host.data() + tab_off, &dn_tab(), sizeof(DnTab));
    hipStream_t st = nullptr;
    Q3C(intake_stream(device, &st));
    HIPC(hipMemcpyAsync(dev, host.data(), host_bytes, hipMemcpyHostToDevice, st));
    const DnDesc* dd = (const DnDesc*)dev;
    const DnTab* dt = (const DnTab*)(dev + tab_off);
    hipLaunchKernelGGL(k_dn_analysis, dim3((unsigned)((max_T + 3) / 4), (unsigned)n), dim3(DN_THREADS), 0, st, dd, dt);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(k_dn_gain, dim3((unsigned)((max_T + DG_TT - 1) / DG_TT), (unsigned)((DN_K + DG_KB - 1) / DG_KB), (unsigned)n), dim3(DN_THREADS), 0, st, dd);
    HIPC(hipGetLastError());
    if (outs) {
        const long long hops = (max_n + DN_H - 1) / DN_H;
        hipLaunchKernelGGL(k_dn_synthesis, dim3((unsigned)((hops + DS_R - 1) / DS_R), (unsigned)n), dim3(DN_THREADS), 0, st, dd, dt);
        HIPC(hipGetLastError());
        HIPC(hipStreamSynchronize(st));
        return Q3_OK;
    }
    hipLaunchKernelGGL(k_dn_level, dim3((unsigned)max_chunks, (unsigned)n), dim3(DN_THREADS), 0, st, dd);
    HIPC(hipGetLastError());
    for (int i = 0; i < n; ++i) {
        std::vector<float> part((size_t)chunks[(size_t)i] * 2);
        HIPC(hipMemcpyAsync(part.data(), dev + part_off[(size_t)i], part.size() * 4, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        double sl = 0.0, sp = 0.0;
        for (int c = 0; c < chunks[(size_t)i]; ++c) { sl += (double)part[2 * (size_t)c]; sp += (double)part[2 * (size_t)c + 1]; }
        sums[2 * i] = sl; sums[2 * i + 1] = sp;
    }
    return Q3_OK;
}
}  // namespace

extern "C" q3_status q3_denoise_plan(int64_t n_samples, int* frames, int* valid_lo, int* valid_hi, size_t* workspace_bytes) {
    if (n_samples < 1 || n_samples > DN_MAX_N)
        return set_err(Q3_INVALID_ARG, "q3_denoise_plan: %lld samples (1 .. %lld: 120 s at 24 kHz)", (long long)n_samples, DN_MAX_N);
    const DnPlan p = dn_plan(n_samples);
    if (frames) *frames = p.T;
    if (valid_lo) *valid_lo = p.lo;
    if (valid_hi) *valid_hi = p.hi;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return Q3_OK;
}

extern "C" q3_status q3_ref_audio_denoise(q3_ref_audio* const* in, int n, const float* reduce_db, q3_ref_audio** out) {
    const char* who = "q3_ref_audio_denoise";
    if (!in || !out) return set_err(Q3_INVALID_ARG, "%s: null argument", who);
    if (n < 1 || n > DN_MAX_CLIPS) return set_err(Q3_INVALID_ARG, "%s: %d clips (1 .. %d)", who, n, DN_MAX_CLIPS);
    std::vector<float> floors((size_t)n);
    for (int i = 0; i < n; ++i) {
        const float db = reduce_db ? reduce_db[i] : 12.0f;
        if (!(db >= 0.0f && db <= 30.0f)) return set_err(Q3_INVALID_ARG, "%s: clip %d: reduce_db %g (0 .. 30)", who, i, (double)db);
        floors[(size_t)i] = (float)pow(10.0, -(double)db / 20.0);
    }
    for (int i = 0; i < n; ++i) {
        if (!in[i]) return set_err(Q3_INVALID_ARG, "%s: clip %d: null handle", who, i);
        if (in[i]->device != in[0]->device) return set_err(Q3_INVALID_ARG, "%s: clip %d is on device %d, clip 0 on device %d", who, i, in[i]->device, in[0]->device);
    }
    const int device = in[0]->device;
    HIPC(hipSetDevice(device));
    std::vector<q3_ref_audio*> objs;
    char* block = nullptr;
    q3_status st = Q3_OK;
    for (int i = 0; i < n && st == Q3_OK; ++i) {
        q3_ref_audio* r = new q3_ref_audio(*in[i]);              // the source's rate / format / channels
        r->dev = nullptr;
        objs.push_back(r);
        q3_relax_capture_mode();
        const hipError_t e = dev_malloc((void**)&r->dev, (size_t)r->n * 4);
        if (e != hipSuccess) st = set_err(Q3_HIP_ERROR, "%s: %lld samples on the device: %s", who, (long long)r->n, hipGetErrorString(e));
    }
    if (st == Q3_OK) st = dn_run(device, n, in, floors.data(), objs.data(), nullptr, &block);
    dev_free(block);                                             // (the call has waited for the launches)
    if (st != Q3_OK) { for (q3_ref_audio* r : objs) q3_ref_audio_free(r); return st; }
    for (int i = 0; i < n; ++i) out[i] = objs[(size_t)i];
    return Q3_OK;
}

extern "C" q3_status q3_ref_audio_noise(q3_ref_audio* r, double* noise_dbfs, double* snr_db) {
    const char* who = "q3_ref_audio_noise";
    if (!r || (!noise_dbfs && !snr_db)) return set_err(Q3_INVALID_ARG, "%s: null argument", who);
    const DnPlan p = dn_plan(r->n);
    if (p.hi < p.lo) return set_err(Q3_UNSUPPORTED, "%s: clip of %lld samples is too short to estimate a noise floor (more than %d)", who, (long long)r->n, DN_N - DN_H);
    HIPC(hipSetDevice(r->device));
    char* block = nullptr;
    double sums[2] = {0.0, 0.0};
    const q3_status st = dn_run(r->device, 1, &r, nullptr, nullptr, sums, &block);
    dev_free(block);
    Q3C(st);
    // means over the valid frames; a bin's power over N * sum(w^2) / 2 = 65536 is its share of the mean square of the samples
    const double frames = (double)(p.hi - p.lo + 1);
    const double nz = std::max(sums[0] / frames, 1e-30), sig = std::max(sums[1] / frames - nz, 1e-30);
    if (noise_dbfs) *noise_dbfs = 10.0 * log10(nz / 65536.0);
    if (snr_db) *snr_db = 10.0 * log10(sig / nz);
    return Q3_OK;
}
