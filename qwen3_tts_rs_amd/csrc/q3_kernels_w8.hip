// q3_kernels_w8.hip — FP8 (OCP e4m3fn) block-scaled weights for the M <= 16 decode GEMVs: LinArgs::tiled == 3, and
// their 4-row-tile form for M <= 8, LinArgs::tiled == 4 (k_gemv_w8r4, at the end of this file).
// Part of the q3_kernels_gemv.hip translation unit (included at its end): the B operand — x in three exact bf16 planes,
// the half-row form, the LDS-crossbar move — is the family's own code, used here as it stands.
//
//   * Format ("mode 3"). One power-of-two scale 2^e per weight row and 128-wide K block, e the smallest integer with
//     amax(block) * 2^-e <= 448 (0 for an all-zero block, never below W8_EMIN), code = RNE_e4m3(W * 2^-e). The quotient is exact
//     in f32 and code * 2^e is exact in bf16, so v_cvt_scalef32_pk_bf16_fp8 — two codes times the scale into two bf16 values, one
//     VALU instruction — is the whole dequantisation, and the values enter the family's bf16x3 MFMA arithmetic unrounded.
//   * Image. 1 KiB tiles of 16 rows x 64 k, [ceil(N/16)][Kpad/64][64 lanes][16 bytes], Kpad = K rounded up to 128, zero codes in
//     the padding. Slot `lane` = (row = lane & 15, k-group = lane >> 4) holds the A operand of TWO k-steps of
//     v_mfma_f32_16x16x32_bf16: bytes 0-7 = W[row][64 t + 8 kg .. +8), bytes 8-15 = W[row][64 t + 32 + 8 kg .. +8) — the k
//     order of the bf16 tiles inside each step, so the B operand is the siblings'. One global_load_dwordx4 per lane streams a
//     tile. Scales: one E8M0 byte (e + 127) per row and block, [ceil(N/16)][Kpad/128][16 rows] — a lane's scale is one byte load
//     whose 16 addresses share a 16-byte run.
//   * Work split. A workgroup = 8 waves owns one 16-row tile (two for SwiGLU, which share the B operand) and splits K over the
//     waves in whole 128-k blocks (two tile loads, one scale, four k-steps of x). A wave keeps TWO blocks in flight: the next
//     block's x, scale and tiles are requested before the current block is split and multiplied — at half the bytes per row a
//     block's registers are 8 per matrix instead of 16, which is what makes the second buffer affordable. Requests go out x
//     first, then scale, then tiles: vmcnt retires in issue order, and the split needs only x.
//   * Contract: the family's. f32-exact products of x with the dequantised weights, f32 MFMA accumulation, cross-wave
//     reduction through LDS in fixed wave order; ksplit == 2 adds two addends onto zeros (k_gemv_sk2's rule).

namespace q3 {

constexpr int W8_EMIN = -120;        // keeps 2^-e a normal f32 and (smallest code) * 2^e a bf16 value; amax < 448 * 2^-120 only

// The first 14 dwords of the arguments arrive preloaded in SGPRs (see Q3_LIN_PRE): the pointers and sizes the first requests need
#define Q3_W8_PRE const uint8_t* pW, const uint8_t* pW2, const float* px, const float* pnw, const uint8_t* pS, int pM, int pK, int pKpad, int pldx
#define Q3_W8_PASS(a) reinterpret_cast<const uint8_t*>((a).W), reinterpret_cast<const uint8_t*>((a).W2), (a).x, (a).norm_w, (a).S, (a).M, (a).K, (a).Kpad, (a).ldx, (a)

// eight codes (two dwords) times 2^e -> the A operand of one k-step; exact
__device__ __forceinline__ u32x4_t w8_dequant(uint32_t c0, uint32_t c1, float scale) {
    u32x4_t r;
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c0, scale, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c0, scale, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c1, scale, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c1, scale, true));
    return r;
}

// HALF (M <= 8): the half-row x form of k_gemv_mfma; CO: x requested row-contiguous and moved through the LDS crossbar
// (M >= 3; k_gemv_sk2); SK: this workgroup owns half of the blocks (blockIdx.y) and ADDS its result onto zeros.
template <int EPI, bool RMS, bool HALF, bool CO, bool SK>
__global__ __launch_bounds__(512) void k_gemv_w8(Q3_W8_PRE, LinArgs a_in) {
    LinArgs a = a_in;
    a.W = reinterpret_cast<const uint16_t*>(pW); a.W2 = reinterpret_cast<const uint16_t*>(pW2); a.x = px; a.norm_w = pnw; a.S = pS;
    a.M = pM; a.K = pK; a.Kpad = pKpad; a.ldx = pldx;
    constexpr int NWAVES = 8;
    constexpr int NW = (EPI == EPI_SWIGLU) ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float red[NWAVES][NW][256];
    __shared__ float ssq[NWAVES][16];
    Q3T_DECL Q3T(0); Q3T_K(7, a.Kpad);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 15, kg = lane >> 4;         // B operand: batch column m; A operand: weight row m; k-group kg of a step
    const int NB = a.Kpad >> 7;                      // blocks of 128 k
    const int half = SK ? (int)blockIdx.y : 0;
    const int h0 = SK ? (half * NB) / 2 : 0, h1 = SK ? ((half + 1) * NB) / 2 : NB;
    const int b0 = h0 + (wave * (h1 - h0)) / NWAVES, b1 = h0 + ((wave + 1) * (h1 - h0)) / NWAVES;
    const size_t tile_base = (size_t)blockIdx.x * NB * 128 + lane;        // two 64-slot tiles per block
    const u32x4_t* __restrict__ wp = reinterpret_cast<const u32x4_t*>(a.W) + tile_base;
    const u32x4_t* __restrict__ wp2 = NW == 2 ? reinterpret_cast<const u32x4_t*>(a.W2) + tile_base : wp;
    const uint8_t* __restrict__ sp = a.S + (size_t)blockIdx.x * NB * 16 + m;
    const uint8_t* __restrict__ sp2 = NW == 2 ? a.S2 + (size_t)blockIdx.x * NB * 16 + m : sp;
    // x in B-operand order (M <= 2): lane (m, kg) asks for its own four (HALF) or eight floats of the k-group
    const int xrow = HALF ? (m & 7) : m, xhalf = HALF ? (m >> 3) * 4 : 0;
    const bool act = xrow < a.M;
    const __amdgpu_buffer_rsrc_t xres = act_rsrc(a.x);       // write-through / L1-bypassing transport: q3_kernels.h
    const int xr = (act ? xrow : 0) * a.ldx + kg * 8 + xhalf;
    // x in row-contiguous order (CO): lane l asks for row l / 8, chunk l % 8 (HALF) or row l / 4, chunks 2 (l % 4), 2 (l % 4) + 1
    const int crow = HALF ? lane >> 3 : lane >> 2, cchunk = HALF ? lane & 7 : 2 * (lane & 3);
    const bool cact = crow < a.M;
    const int xc = __mul24(cact ? crow : 0, a.ldx) + cchunk * 4;
    const int bsrc = HALF ? ((xrow * 8) + 2 * kg + (m >> 3)) * 4 : (m * 4 + kg) * 4;
    const int kn = kg * 8 + xhalf;                   // this lane's first k inside a step (B order): norm weight, masks

    // epilogue operands requested up front (and not combined here: see k_gemv_sk2)
    float pre_b = 0.0f, pre_r = 0.0f;
    {
        const int col = tid >> 4, n = blockIdx.x * 16 + (tid & 15);
        if (half == 0 && tid < 256 && col < a.M && n < a.N) {
            if (a.bias) pre_b = a.bias[n];
            if constexpr (EPI == EPI_RESID) pre_r = act_ld1(act_rsrc(a.resid), (col * a.ldr + n) * 4);
        }
    }
    f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    float ss = 0.0f;
    const float4 z4 = {0.f, 0.f, 0.f, 0.f};
    struct Blk { float4 xa[4], xb[4], na[4], nb[4]; uint32_t e, e2; u32x4_t wa[2], wb[2]; };
    // every request of block b, in the order their data is needed: x (+ norm weight), scale, tiles. Nothing is read at or
    // beyond K or in rows >= M: those lanes hold zeros, so the split needs no mask of its own.
    auto request = [&](Blk& g, int b) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k0 = (b * 4 + i) * 32;
            if constexpr (CO) {
                const bool ok = cact && (k0 + cchunk * 4) < a.K;
                g.xa[i] = ok ? act_ld4(xres, (xc + k0) * 4) : z4;
                if constexpr (!HALF) g.xb[i] = ok ? act_ld4(xres, (xc + k0) * 4 + 16) : z4;
            } else {
                const bool ok = act && (k0 + kn) < a.K;
                g.xa[i] = ok ? act_ld4(xres, (xr + k0) * 4) : z4;
                if constexpr (!HALF) g.xb[i] = ok ? act_ld4(xres, (xr + k0) * 4 + 16) : z4;
            }
            if constexpr (RMS) {
                const int ko = (k0 + kn) < a.K ? k0 + kn : 0;             // past K: x is zero there, any finite weight will do
                g.na[i] = *reinterpret_cast<const float4*>(a.norm_w + ko);
                if constexpr (!HALF) g.nb[i] = *reinterpret_cast<const float4*>(a.norm_w + ko + 4);
            }
        }
        g.e = sp[(size_t)b * 16];
        if constexpr (NW == 2) g.e2 = sp2[(size_t)b * 16];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            g.wa[j] = Q3_WLOAD(wp + (size_t)(2 * b + j) * 64);
            if constexpr (NW == 2) g.wb[j] = Q3_WLOAD(wp2 + (size_t)(2 * b + j) * 64);
        }
    };
    auto multiply = [&](Blk& g) {
        Split3 s3[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (CO) { g.xa[i] = x_to_b_order(g.xa[i], bsrc); if constexpr (!HALF) g.xb[i] = x_to_b_order(g.xb[i], bsrc); }
            if constexpr (HALF) s3[i] = gemv_prep_half<RMS>(true, g.xa[i], RMS ? g.na[i] : g.xa[i], ss);
            else s3[i] = gemv_prep<RMS>(true, g.xa[i], g.xb[i], RMS ? g.na[i] : g.xa[i], RMS ? g.nb[i] : g.xb[i], ss);
        }
        __builtin_amdgcn_sched_barrier(0);          // the splits run under the tiles' latency; only the converts and MFMAs wait for HBM
        Q3T(1);
        const float sc = __uint_as_float(g.e << 23), sc2 = NW == 2 ? __uint_as_float(g.e2 << 23) : sc;      // E8M0 -> 2^e
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                acc0 = mfma3(w8_dequant(g.wa[j][2 * h], g.wa[j][2 * h + 1], sc), s3[2 * j + h], acc0);
                if constexpr (NW == 2) acc1 = mfma3(w8_dequant(g.wb[j][2 * h], g.wb[j][2 * h + 1], sc2), s3[2 * j + h], acc1);
            }
    };
    if (b0 < b1) {                                   // wave-uniform
        Blk A, B;
        request(A, b0);
        for (int b = b0; b < b1; b += 2) {
            if (b + 1 < b1) request(B, b + 1);
            __builtin_amdgcn_sched_barrier(0);      // the next block's requests are out before this block's first use
            multiply(A);
            if (b + 1 >= b1) break;
            if (b + 2 < b1) request(A, b + 2);
            __builtin_amdgcn_sched_barrier(0);
            multiply(B);
        }
    }
    Q3T_W(2);
    // side job behind the last request (vmcnt retires in issue order: k_gemv_mfma)
    zero_job(a.zero, a.zero_n, SK ? blockIdx.y * gridDim.x + blockIdx.x : blockIdx.x, SK ? gridDim.x * 2 : gridDim.x, tid, NWAVES * 64);
    // partial tile -> LDS, layout [col m][row]: lane (m, kg) owns rows kg*4 .. kg*4+3
    *reinterpret_cast<f32x4_t*>(&red[wave][0][m * 16 + kg * 4]) = acc0;
    if constexpr (NW == 2) *reinterpret_cast<f32x4_t*>(&red[wave][1][m * 16 + kg * 4]) = acc1;
    if constexpr (RMS) {
        float sc = HALF ? gemv_ss_half(ss) : ss;
        sc += __shfl_xor(sc, 16); sc += __shfl_xor(sc, 32);
        if (kg == 0) ssq[wave][m] = sc;
    }
    Q3T(6);
    __syncthreads();
    Q3T(5);
    if (tid < 256) {
        const int col = tid >> 4, row = tid & 15, n = blockIdx.x * 16 + row;
        if (col < a.M && n < a.N) {
            float v = 0.0f, v2 = 0.0f;
#pragma unroll
            for (int w = 0; w < NWAVES; ++w) {       // fixed wave order: deterministic
                v += red[w][0][tid];
                if constexpr (NW == 2) v2 += red[w][1][tid];
            }
            if constexpr (RMS) {
                float tot = 0.0f;
#pragma unroll
                for (int w = 0; w < NWAVES; ++w) tot += ssq[w][col];
                const float den = sqrtf(tot / (float)a.K + a.eps);
                v = v / den;
                if constexpr (NW == 2) v2 = v2 / den;
            }
            if constexpr (SK) {
                if (half == 0) { const float pre = EPI == EPI_RESID ? pre_r + pre_b : pre_b; v = pre + v; }
                unsafeAtomicAdd(&a.y[(size_t)col * a.ldy + n], v);
            } else {
                if (a.bias) v = v + pre_b;
                if constexpr (EPI == EPI_RESID) v = pre_r + v;
                if constexpr (EPI == EPI_SILU) v = v / (1.0f + expf(-v));
                if constexpr (EPI == EPI_SWIGLU) v = (v / (1.0f + expf(-v))) * v2;
                act_st1(act_rsrc(a.y), (col * a.ldy + n) * 4, v);
            }
        }
    }
    Q3T(3); act_drain(); Q3T_W(4); Q3T_FLUSH(a, SK ? blockIdx.y * gridDim.x + blockIdx.x : blockIdx.x);
}

template <int EPI, bool RMS, bool SK>
static hipError_t launch_gemv_w8_t(const LinArgs& a, hipStream_t st) {
    const dim3 grid((a.N + 15) / 16, SK ? 2 : 1), blk(512);
    if (a.M <= 2) hipLaunchKernelGGL((k_gemv_w8<EPI, RMS, true, false, SK>), grid, blk, 0, st, Q3_W8_PASS(a));
    else if (a.M <= 8) hipLaunchKernelGGL((k_gemv_w8<EPI, RMS, true, true, SK>), grid, blk, 0, st, Q3_W8_PASS(a));
    else hipLaunchKernelGGL((k_gemv_w8<EPI, RMS, false, true, SK>), grid, blk, 0, st, Q3_W8_PASS(a));
    return hipGetLastError();
}

// Everything outside the family is refused with hipErrorNotSupported — more than 16 rows, a norm in front of +residual / SiLU,
// split-K with a norm, another epilogue or fewer than 16 k-steps — and nothing is launched.
hipError_t launch_gemv_w8(const LinArgs& a, hipStream_t st) {
    if (a.tiled != 3 || a.M < 1 || a.M > 16 || a.N < 1 || !a.W || !a.S || !a.x || !a.y) return hipErrorNotSupported;
    if (a.Kpad % 128 != 0 || a.K % 8 != 0 || a.K < 8 || a.K > a.Kpad || a.Kpad - a.K >= 128 || a.ldx % 4 != 0) return hipErrorNotSupported;
    if (a.epi == EPI_SWIGLU && (!a.W2 || !a.S2)) return hipErrorNotSupported;
    if (a.epi != EPI_SWIGLU && (a.W2 || a.S2)) return hipErrorNotSupported;
    if (a.epi == EPI_RESID && !a.resid) return hipErrorNotSupported;
    const bool rms = a.norm_w != nullptr;
    if (a.ksplit == 2) {
        if (rms || a.Kpad < 512) return hipErrorNotSupported;
        if (a.epi == EPI_NONE) return launch_gemv_w8_t<EPI_NONE, false, true>(a, st);
        if (a.epi == EPI_RESID) return launch_gemv_w8_t<EPI_RESID, false, true>(a, st);
        return hipErrorNotSupported;
    }
    if (a.ksplit != 1) return hipErrorNotSupported;
    switch (a.epi) {
        case EPI_NONE: return rms ? launch_gemv_w8_t<EPI_NONE, true, false>(a, st) : launch_gemv_w8_t<EPI_NONE, false, false>(a, st);
        case EPI_RESID: return rms ? hipErrorNotSupported : launch_gemv_w8_t<EPI_RESID, false, false>(a, st);
        case EPI_SILU: return rms ? hipErrorNotSupported : launch_gemv_w8_t<EPI_SILU, false, false>(a, st);
        case EPI_SWIGLU: return rms ? launch_gemv_w8_t<EPI_SWIGLU, true, false>(a, st) : launch_gemv_w8_t<EPI_SWIGLU, false, false>(a, st);
        default: return hipErrorNotSupported;
    }
}

// ------------------------------------------------------------------------------------------------
// Quantiser: the mode-3 image and its scales from the resident mode-1 bf16 image, on the device — every data-parallel rank
// derives the same bytes from the weights it was sent, and no host pass walks GB of weights.
// One wave per (16-row tile, 128-k block): lane (row, kg) reads its slot of the block's four bf16 tiles (the 32 values it will
// also write: no value changes lanes), the row's amax is a two-step butterfly over the four k-groups, and the exponent comes
// from the amax's own exponent and mantissa — integer work, so the bytes do not depend on the device or the host that checks.
// ------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8_t;

// smallest e with amax * 2^-e <= 448 = 0.875 * 2^9: amax = f * 2^x, f in [0.5, 1) -> e = x - 9, one more if f > 0.875
__device__ __forceinline__ int w8_block_exp(float amax) {
    int ex = 0;
    if (amax > 0.0f) {
        int x; const float f = frexpf(amax, &x);
        ex = x - 9 + (f > 0.875f ? 1 : 0);
        ex = ex < W8_EMIN ? W8_EMIN : ex;
    }
    return ex;
}

__global__ __launch_bounds__(256) void k_w8_build(const uint16_t* __restrict__ t1, int tiles, int S32, int NB, uint8_t* __restrict__ codes,
                                                  uint8_t* __restrict__ scales) {
    const int item = (int)blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (item >= tiles * NB) return;                  // wave-uniform
    const int tile = item / NB, b = item - tile * NB;
    float w[4][8];
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int s = b * 4 + i;                     // bf16 k-step; the mode-1 image ends at up32(K): zeros beyond
        u16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (s < S32) v = *reinterpret_cast<const u16x8_t*>(t1 + (((size_t)tile * S32 + s) * 64 + lane) * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) { w[i][e] = __uint_as_float((uint32_t)v[e] << 16); amax = fmaxf(amax, fabsf(w[i][e])); }
    }
    amax = fmaxf(amax, __shfl_xor(amax, 16)); amax = fmaxf(amax, __shfl_xor(amax, 32));
    const int ex = w8_block_exp(amax);
    const float inv = __uint_as_float((uint32_t)(127 - ex) << 23);       // 2^-e, a normal f32 for every e in [W8_EMIN, 120]
    u32x4_t out[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int lo = __builtin_amdgcn_cvt_pk_fp8_f32(w[i][0] * inv, w[i][1] * inv, 0, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(w[i][2] * inv, w[i][3] * inv, lo, true);
        int hi = __builtin_amdgcn_cvt_pk_fp8_f32(w[i][4] * inv, w[i][5] * inv, 0, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(w[i][6] * inv, w[i][7] * inv, hi, true);
        out[i >> 1][2 * (i & 1)] = (uint32_t)lo; out[i >> 1][2 * (i & 1) + 1] = (uint32_t)hi;
    }
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(codes) + ((size_t)tile * NB * 2 + 2 * b) * 64 + lane;
    dst[0] = out[0]; dst[64] = out[1];
    if (lane < 16) scales[((size_t)tile * NB + b) * 16 + lane] = (uint8_t)(ex + 127);
}

size_t w8_code_bytes(int N, int K) { return (size_t)((N + 15) & ~15) * ((K + 127) & ~127); }
size_t w8_scale_bytes(int N, int K) { return w8_code_bytes(N, K) / 128; }

hipError_t launch_w8_build(const uint16_t* t1, int N, int K, uint8_t* codes, uint8_t* scales, hipStream_t st) {
    if (!t1 || !codes || !scales || N < 1 || K < 8 || K % 8) return hipErrorInvalidValue;
    const int tiles = (N + 15) / 16, S32 = (K + 31) / 32, NB = (K + 127) / 128;
    if ((long long)tiles * NB > 0x7fffffffLL / 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_w8_build, dim3((tiles * NB + 3) / 4), dim3(256), 0, st, t1, tiles, S32, NB, codes, scales);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// 4-row-tile form ("mode 4", LinArgs::tiled == 4, M <= 8): the work split of k_gemv_mfma4 over FP8 codes.
//   * Image. The quantisation rule of mode 3 (same codes and exponents per row and 128-wide K block) in 1 KiB tiles of 4 rows x
//     256 k, [ceil(N/4)][Kpad/256][64 lanes][16 bytes], Kpad = K rounded up to 256, zero codes in the padding: lane 4b + i holds
//     the 16 codes W[n0 + i][256 t + 16 b .. +16) — the bf16 4-row tile's lane order (block b = K slice, i = row) at twice the k
//     per lane, one coalesced 16-byte load per lane. Scales [ceil(N/4)][Kpad/128][4 rows]: lane (b, i) of tile t reads the byte of
//     block 2 t + (b >> 3).
//   * Work split. A workgroup owns one 4-row tile (two for SwiGLU, sharing the B operand); its waves split the 256-k tiles in
//     contiguous ranges; the 16 blocks of v_mfma_f32_4x4x4_16b_bf16 are 16 K slices. Lane 4b + j supplies
//     x[4 mg + j][256 t + 16 b .. +16) in three exact bf16 planes. Per lane and tile: one tile load, one scale byte, four
//     v_cvt_scalef32_pk_bf16_fp8 pairs (16 bf16 values, exact) and 12 MFMAs per x row group.
//   * Pipeline. Two tiles in flight per wave, requests in the order x, scale, codes (k_gemv_w8's).
//   * Reduction. The transposing butterfly over the 16 blocks (tsum_blocks), then across waves through LDS in fixed order.
// ------------------------------------------------------------------------------------------------
template <int EPI, bool RMS, int MG>
__global__ __launch_bounds__(512) void k_gemv_w8r4(Q3_W8_PRE, LinArgs a_in) {
    LinArgs a = a_in;
    a.W = reinterpret_cast<const uint16_t*>(pW); a.W2 = reinterpret_cast<const uint16_t*>(pW2); a.x = px; a.norm_w = pnw; a.S = pS;
    a.M = pM; a.K = pK; a.Kpad = pKpad; a.ldx = pldx;
    constexpr int NW = (EPI == EPI_SWIGLU) ? 2 : 1;
    __shared__ float red[8][NW][MG][4][4];
    __shared__ float ssq[8][MG][4];
    Q3T_DECL Q3T(0); Q3T_K(7, a.Kpad);
    const int nwv = blockDim.x >> 6;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 3, kb = lane >> 2;          // A operand: weight row j; B operand: batch column j; K slice kb
    const int T = a.Kpad >> 8;                       // tiles of 256 k
    const int t0 = (wave * T) / nwv, t1 = ((wave + 1) * T) / nwv;
    const size_t tile_base = (size_t)blockIdx.x * T * 64 + lane;
    const u32x4_t* __restrict__ wp = reinterpret_cast<const u32x4_t*>(a.W) + tile_base;
    const u32x4_t* __restrict__ wp2 = NW == 2 ? reinterpret_cast<const u32x4_t*>(a.W2) + tile_base : wp;
    const size_t scale_base = ((size_t)blockIdx.x * 2 * T + (kb >> 3)) * 4 + j;       // + 8 t: block 2 t + (kb >> 3), row j
    const uint8_t* __restrict__ sp = a.S + scale_base;
    const uint8_t* __restrict__ sp2 = NW == 2 ? a.S2 + scale_base : sp;
    const __amdgpu_buffer_rsrc_t xres = act_rsrc(a.x);       // write-through / L1-bypassing transport: q3_kernels.h
    int xr[MG]; bool act[MG];                                 // byte offsets into x
#pragma unroll
    for (int g = 0; g < MG; ++g) {
        const int m = g * 4 + j;
        act[g] = m < a.M;
        xr[g] = (act[g] ? m : 0) * a.ldx * 4;
    }

    float pre_b = 0.0f, pre_r = 0.0f;     // epilogue operands requested up front (see k_gemv_mfma)
    if (tid < 16 * MG) {
        const int m = tid >> 2, n = blockIdx.x * 4 + (tid & 3);
        if (m < a.M && n < a.N) {
            if (a.bias) pre_b = a.bias[n];
            if constexpr (EPI == EPI_RESID) pre_r = act_ld1(act_rsrc(a.resid), (m * a.ldr + n) * 4);
        }
    }
    f32x4_t acc[NW][MG];
    float ss[MG];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int g = 0; g < MG; ++g) acc[w][g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < MG; ++g) ss[g] = 0.0f;
    const float4 z4 = {0.f, 0.f, 0.f, 0.f};
    struct Tile { float4 x[MG][4], n[4]; uint32_t e, e2; u32x4_t w, w2; };
    // every request of tile t, in the order their data is needed: x (+ norm weight), scale, codes. Nothing is read at or beyond
    // K or in rows >= M: those lanes hold zeros, so the split needs no mask of its own (K % 8 == 0: a half of 8 k is in or out whole).
    auto request = [&](Tile& g, int t) {
        const int k0 = t * 256 + kb * 16;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool ok = (k0 + 8 * h) < a.K;
#pragma unroll
            for (int mg = 0; mg < MG; ++mg)
#pragma unroll
                for (int q = 0; q < 2; ++q) g.x[mg][2 * h + q] = (act[mg] && ok) ? act_ld4(xres, xr[mg] + (k0 + 8 * h + 4 * q) * 4) : z4;
            if constexpr (RMS) {
                const int ko = ok ? k0 + 8 * h : 0;                       // past K: x is zero there, any finite weight will do
                g.n[2 * h] = *reinterpret_cast<const float4*>(a.norm_w + ko);
                g.n[2 * h + 1] = *reinterpret_cast<const float4*>(a.norm_w + ko + 4);
            }
        }
        g.e = sp[(size_t)t * 8];
        if constexpr (NW == 2) g.e2 = sp2[(size_t)t * 8];
        g.w = Q3_WLOAD(wp + (size_t)t * 64);
        if constexpr (NW == 2) g.w2 = Q3_WLOAD(wp2 + (size_t)t * 64);
    };
    auto multiply = [&](Tile& g) {
        Split3 s3[MG][2];
#pragma unroll
        for (int mg = 0; mg < MG; ++mg)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                s3[mg][h] = gemv_prep<RMS>(true, g.x[mg][2 * h], g.x[mg][2 * h + 1], RMS ? g.n[2 * h] : g.x[mg][2 * h], RMS ? g.n[2 * h + 1] : g.x[mg][2 * h + 1], ss[mg]);
        __builtin_amdgcn_sched_barrier(0);          // the splits run under the tile's latency; only the converts and MFMAs wait for HBM
        Q3T(1);
        const float sc = __uint_as_float(g.e << 23), sc2 = NW == 2 ? __uint_as_float(g.e2 << 23) : sc;      // E8M0 -> 2^e
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32x4_t wa = w8_dequant(g.w[2 * h], g.w[2 * h + 1], sc);
            const u32x4_t wb = NW == 2 ? w8_dequant(g.w2[2 * h], g.w2[2 * h + 1], sc2) : wa;
#pragma unroll
            for (int mg = 0; mg < MG; ++mg) {
                acc[0][mg] = mfma4_tile(wa, s3[mg][h], acc[0][mg]);
                if constexpr (NW == 2) acc[1][mg] = mfma4_tile(wb, s3[mg][h], acc[1][mg]);
            }
        }
    };
    if (t0 < t1) {                                   // wave-uniform
        Tile A, B;
        request(A, t0);
        for (int t = t0; t < t1; t += 2) {
            if (t + 1 < t1) request(B, t + 1);
            __builtin_amdgcn_sched_barrier(0);      // the next tile's requests are out before this tile's first use
            multiply(A);
            if (t + 1 >= t1) break;
            if (t + 2 < t1) request(A, t + 2);
            __builtin_amdgcn_sched_barrier(0);
            multiply(B);
        }
    }
    Q3T_W(2);
    zero_job(a.zero, a.zero_n, blockIdx.x, gridDim.x, tid, blockDim.x);
    // the 16 k-blocks of the V = 4 * NW * MG values a lane holds: the transposing butterfly of k_gemv_mfma4
    constexpr int V = 4 * NW * MG;
    float vals[V];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int g = 0; g < MG; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) vals[(w * MG + g) * 4 + i] = acc[w][g][i];
    int idx = 0;
    tsum_blocks<V, V, 32>(vals, lane, idx);
    constexpr int PLAIN_MASK = V >= 16 ? 0 : V == 8 ? 4 : 12;       // canonical writer of (idx, j): plainly-reduced block bits zero
    if ((lane & PLAIN_MASK) == 0) (&red[wave][0][0][0][0])[idx * 4 + j] = vals[0];
    if constexpr (RMS) {
#pragma unroll
        for (int g = 0; g < MG; ++g) {
            const float v = sum_over_blocks(ss[g]);
            if (lane < 4) ssq[wave][g][lane] = v;
        }
    }
    Q3T(6);
    __syncthreads();
    Q3T(5);
    if (tid < 16 * MG) {
        const int m = tid >> 2, i = tid & 3, g = m >> 2, jj = m & 3;
        const int n = blockIdx.x * 4 + i;
        if (m < a.M && n < a.N) {
            float v = 0.0f, v2 = 0.0f;
            for (int w = 0; w < nwv; ++w) {          // fixed wave order: deterministic
                v += red[w][0][g][i][jj];
                if constexpr (NW == 2) v2 += red[w][1][g][i][jj];
            }
            if constexpr (RMS) {
                float tot = 0.0f;
                for (int w = 0; w < nwv; ++w) tot += ssq[w][g][jj];
                const float den = sqrtf(tot / (float)a.K + a.eps);
                v = v / den;
                if constexpr (NW == 2) v2 = v2 / den;
            }
            if (a.bias) v = v + pre_b;
            if constexpr (EPI == EPI_RESID) v = pre_r + v;
            if constexpr (EPI == EPI_SILU) v = v / (1.0f + expf(-v));
            if constexpr (EPI == EPI_SWIGLU) v = (v / (1.0f + expf(-v))) * v2;
            act_st1(act_rsrc(a.y), (m * a.ldy + n) * 4, v);
        }
    }
    Q3T(3); act_drain(); Q3T_W(4); Q3T_FLUSH(a, blockIdx.x);
}

template <int EPI, bool RMS>
static hipError_t launch_gemv_w8r4_t(const LinArgs& a, hipStream_t st) {
    const int T = a.Kpad >> 8;
    const dim3 grid((a.N + 3) / 4), blk((T >= 8 ? 8 : T >= 4 ? 4 : T >= 2 ? 2 : 1) * 64);
    if (a.M <= 4) hipLaunchKernelGGL((k_gemv_w8r4<EPI, RMS, 1>), grid, blk, 0, st, Q3_W8_PASS(a));
    else hipLaunchKernelGGL((k_gemv_w8r4<EPI, RMS, 2>), grid, blk, 0, st, Q3_W8_PASS(a));
    return hipGetLastError();
}

// What k_gemv_mfma4's launcher takes at M <= 8 — no split-K, no norm in front of +residual / SiLU; the rest is refused with
// hipErrorNotSupported and nothing is launched.
hipError_t launch_gemv_w8r4(const LinArgs& a, hipStream_t st) {
    if (a.tiled != 4 || a.M < 1 || a.M > 8 || a.N < 1 || !a.W || !a.S || !a.x || !a.y || a.ksplit != 1) return hipErrorNotSupported;
    if (a.Kpad % 256 != 0 || a.K % 8 != 0 || a.K < 8 || a.K > a.Kpad || a.Kpad - a.K >= 256 || a.ldx % 4 != 0) return hipErrorNotSupported;
    if (a.epi == EPI_SWIGLU && (!a.W2 || !a.S2)) return hipErrorNotSupported;
    if (a.epi != EPI_SWIGLU && (a.W2 || a.S2)) return hipErrorNotSupported;
    if (a.epi == EPI_RESID && !a.resid) return hipErrorNotSupported;
    const bool rms = a.norm_w != nullptr;
    switch (a.epi) {
        case EPI_NONE: return rms ? launch_gemv_w8r4_t<EPI_NONE, true>(a, st) : launch_gemv_w8r4_t<EPI_NONE, false>(a, st);
        case EPI_RESID: return rms ? hipErrorNotSupported : launch_gemv_w8r4_t<EPI_RESID, false>(a, st);
        case EPI_SILU: return rms ? hipErrorNotSupported : launch_gemv_w8r4_t<EPI_SILU, false>(a, st);
        case EPI_SWIGLU: return rms ? launch_gemv_w8r4_t<EPI_SWIGLU, true>(a, st) : launch_gemv_w8r4_t<EPI_SWIGLU, false>(a, st);
        default: return hipErrorNotSupported;
    }
}

// Quantiser of the mode-4 image from the resident mode-2 bf16 image (4 rows x 128 k per tile, lane = (k-group << 2) | row, 8 values).
// One wave per (4-row tile, 256-k tile): lane 4b + i loads the two 16-byte mode-2 slots that hold its own 16 values — tile
// 2 t + (b >> 3), k-groups 2 (b & 7) and 2 (b & 7) + 1 — so nothing changes lanes; the row / block amax is a butterfly over the eight
// lanes of one row and one half (xor 4, 8, 16); exponent and rounding are k_w8_build's. One 16-byte store per lane, no atomics.
__global__ __launch_bounds__(256) void k_w8_build4(const uint16_t* __restrict__ t2, int tiles, int S2, int T4, uint8_t* __restrict__ codes,
                                                   uint8_t* __restrict__ scales) {
    const int item = (int)blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (item >= tiles * T4) return;                  // wave-uniform
    const int tile = item / T4, t = item - tile * T4;
    const int i = lane & 3, b = lane >> 2, s = 2 * t + (b >> 3);      // the mode-2 image ends at up128(K): zeros beyond
    float w[16];
    float amax = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        u16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (s < S2) v = *reinterpret_cast<const u16x8_t*>(t2 + (((size_t)tile * S2 + s) * 64 + (((2 * (b & 7) + h) << 2) | i)) * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) { w[8 * h + e] = __uint_as_float((uint32_t)v[e] << 16); amax = fmaxf(amax, fabsf(w[8 * h + e])); }
    }
    amax = fmaxf(amax, __shfl_xor(amax, 4)); amax = fmaxf(amax, __shfl_xor(amax, 8)); amax = fmaxf(amax, __shfl_xor(amax, 16));
    const int ex = w8_block_exp(amax);
    const float inv = __uint_as_float((uint32_t)(127 - ex) << 23);       // 2^-e, a normal f32 for every e in [W8_EMIN, 120]
    u32x4_t out;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        int c = __builtin_amdgcn_cvt_pk_fp8_f32(w[4 * d] * inv, w[4 * d + 1] * inv, 0, false);
        c = __builtin_amdgcn_cvt_pk_fp8_f32(w[4 * d + 2] * inv, w[4 * d + 3] * inv, c, true);
        out[d] = (uint32_t)c;
    }
    reinterpret_cast<u32x4_t*>(codes)[((size_t)tile * T4 + t) * 64 + lane] = out;
    if ((lane & 28) == 0) scales[((size_t)tile * 2 * T4 + s) * 4 + i] = (uint8_t)(ex + 127);      // lanes 0-3: block 2 t, lanes 32-35: block 2 t + 1
}

size_t w8r4_code_bytes(int N, int K) { return (size_t)((N + 3) & ~3) * ((K + 255) & ~255); }
size_t w8r4_scale_bytes(int N, int K) { return w8r4_code_bytes(N, K) / 128; }

hipError_t launch_w8_build4(const uint16_t* t2, int N, int K, uint8_t* codes, uint8_t* scales, hipStream_t st) {
    if (!t2 || !codes || !scales || N < 1 || K < 8 || K % 8) return hipErrorInvalidValue;
    const int tiles = (N + 3) / 4, S2 = (K + 127) / 128, T4 = (K + 255) / 256;
    if ((long long)tiles * T4 > 0x7fffffffLL / 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_w8_build4, dim3((tiles * T4 + 3) / 4), dim3(256), 0, st, t2, tiles, S2, T4, codes, scales);
    return hipGetLastError();
}

}  // namespace q3
