// q3_kernels_kv8.hip — FP8 (OCP e4m3fn) talker K/V pages ("KV8") and their decode attention.
// Part of the q3_kernels_lm.hip translation unit (included at its end): the prologue's rounding helpers, the activation
// transport and the zero side job are that unit's own code, used here as it stands.
//
//   * Format. One power-of-two scale 2^e per cached ROW (one position, layer, K or V, KV head: 128 elements), e the smallest
//     integer with amax(row) * 2^-e <= 448 (0 for an all-zero row, never below KV8_EMIN), code = RNE_e4m3(x * 2^-e), the scale
//     stored as the E8M0 byte e + 127 — the rule of the FP8 weights. The quotient is exact in f32, so host and
//     device produce the same bytes, and code * 2^e is exact in f32: v_cvt_scalef32_pk_f32_fp8 is the whole dequantisation.
//   * Pages. The pool's geometry with 1-byte elements (same slab order, same kv_rot row rotation, K -> V and layer distances
//     off powers of two), and behind the nkv * 128 * 128 code bytes of a (page, layer, K | V) run its nkv * 128 scale bytes,
//     [kvh][rotated position]: a run is nkv * 128 * 129 bytes, and a row's scale address follows from the page pointer and the
//     layer offset like the row itself — no second table.
//   * Work split of k_attn_kv8. A lane asks for 16 codes of a row (one 16-byte load), 8 lanes hold a row, a wave covers 8
//     consecutive positions per request, the 256-thread workgroup 32 per round. The row's scale byte goes out with the codes
//     as one byte load per lane: the 8 lanes of a row ask for the same address, which the texture addresser serves as one
//     request (a single lane plus a DPP broadcast would put a cross-lane move behind every load's return).
//     Each lane keeps 16 q values and 16 accumulators per q head; a dot product is reduced over 8 lanes in three DPP steps.

namespace q3 {

constexpr int KV8_EMIN = -120;                       // keeps 2^-e a normal f32 (W8_EMIN's reason)
constexpr int KV8_RUN_CODES = KV_PAGE_POS * HEAD_DIM;   // code bytes of one (page, layer, K | V, kv head)

typedef __attribute__((ext_vector_type(4))) unsigned int kv8_u4_t;
typedef __attribute__((ext_vector_type(2))) float kv8_f2_t;

template <int CTRL> __device__ __forceinline__ float kv8_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// sum over aligned groups of 8 lanes, identical bits in every lane of a group: quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror (every lane of a quad then holds the quad's sum, and lane i reads lane 7 - i: the other quad)
__device__ __forceinline__ float kv8_sum8(float v) {
    v += kv8_dpp<0xB1>(v); v += kv8_dpp<0x4E>(v); v += kv8_dpp<0x141>(v);
    return v;
}
__device__ __forceinline__ float kv8_wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
// the row's exponent from its amax: amax = f * 2^x, f in [0.5, 1) -> e = x - 9, one more if f > 0.875 (448 = 0.875 * 2^9)
__device__ __forceinline__ int kv8_exponent(float amax) {
    int ex = 0;
    if (amax > 0.0f) {
        int x; const float f = frexpf(amax, &x);
        ex = x - 9 + (f > 0.875f ? 1 : 0);
        ex = ex < KV8_EMIN ? KV8_EMIN : (ex > 120 ? 120 : ex);      // (120: the largest a finite f32 amax gives)
    }
    return ex;
}
__device__ __forceinline__ float kv8_pow2(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }
// four codes (one dword) times 2^e; exact
__device__ __forceinline__ void kv8_dequant4(uint32_t c, float scale, float* o) {
    const kv8_f2_t lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c, scale, false);
    const kv8_f2_t hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c, scale, true);
    o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
}

// Fused decode attention over KV8 pages: k_attn_fused's paged path (prologue, page-table forms, dummy row, slice sums, zero side
// job, write-through stores, partial record) with its own split of the key range, see the head of this file.
// Leading scalars: k_attn_fused's 14 preloaded dwords — position array, page table, the layer's BYTE offset inside a page,
// q|k|v rows, norm weights, the K -> V distance in bytes and n_splits | nkv << 8 | nh << 16.
template <int NREP, int PAGED>
__global__ __launch_bounds__(256) void k_attn_kv8(const int* p_pos, const unsigned long long* p_tab, size_t p_layer_off, const float* p_qkv,
                                                  const float* p_qw, const float* p_kw, int p_vdelta, int p_pk, AttnArgs a_in) {
    AttnArgs a = a_in;
    a.pos_dev = p_pos; a.qkv = p_qkv; a.q_norm_w = p_qw; a.k_norm_w = p_kw;
    a.n_splits = p_pk & 255; a.nkv = (p_pk >> 8) & 255; a.nh = (p_pk >> 16) & 255;
    uint32_t tab_lo = 0, tab_hi = 0;
    {
        const unsigned long long* trow = p_tab + (size_t)blockIdx.z * KV_MAX_PAGES;
        if constexpr (PAGED == 1) {       // rows of at most 8 pages: one scalar load spread over lanes 0..7
            unsigned long long e[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) e[i] = trow[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) if ((int)(threadIdx.x & 63) == i) { tab_lo = (uint32_t)e[i]; tab_hi = (uint32_t)(e[i] >> 32); }
        } else {
            const unsigned long long e = trow[threadIdx.x & 63];
            tab_lo = (uint32_t)e; tab_hi = (uint32_t)(e >> 32);
        }
    }
    constexpr int RP = NREP >= 2 ? 2 : 1;            // q heads merged per pass of the cross-group merge
    __shared__ __attribute__((aligned(16))) float s_q[NREP][HEAD_DIM];
    __shared__ __attribute__((aligned(16))) float s_k[HEAD_DIM], s_v[HEAD_DIM];
    __shared__ float sm_m[RP][32], sm_l[RP][32];
    __shared__ __attribute__((aligned(16))) float sm_acc[RP][32][HEAD_DIM];
    Q3T_DECL Q3T(0);
    const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, grp = tid >> 3, li = tid & 7, wave = tid >> 6, lane = tid & 63;
    const int QD = a.nh * HEAD_DIM, KD = a.nkv * HEAD_DIM;
    const int pos = a.pos_dev ? a.pos_dev[b] : a.pos_static;
    const int len = pos + 1;
    const int chunk = (len + a.n_splits - 1) / a.n_splits;
    const int start = split * chunk;
    const int end = (start + chunk) < len ? (start + chunk) : len;
    const float scale = 0.08838834764831845f;
    const size_t code_off = p_layer_off + (size_t)kvh * KV8_RUN_CODES;                           // this head's rows, from the page pointer
    const size_t scale_off = p_layer_off + (size_t)a.nkv * KV8_RUN_CODES + (size_t)kvh * KV_PAGE_POS;   // ... and their scale bytes
    const size_t vd = (size_t)p_vdelta;
    // Row of position p <= pos. The 8 groups of a wave ask for 8 consecutive positions pw .. pw + 7, so a wave needs at most
    // TWO pages per request: page i = min(pw, pos) / 128 — wave-uniform, read from the table lanes with v_readlane — and
    // page i + 1; a lane picks by its own position. A lane with nothing to fetch reads row 0 of page 0 (k_attn_fused's dummy).
    const int pos_page = pos >> KV_PAGE_SHIFT;
    const unsigned long long pg_zero = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)tab_hi, 0) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)tab_lo, 0);
    // byte offsets of (codes, scale) of the row from the page table's own pointer (a kernel argument, known to be global: the
    // loads are global_load, not flat_load — see k_attn_fused)
    const char* gbase = reinterpret_cast<const char*>(p_tab);
    auto row_of = [&](int p, int pw, bool ok, ptrdiff_t& codes, ptrdiff_t& sc) {
        int ib = pw >> KV_PAGE_SHIFT; ib = ib < pos_page ? ib : pos_page;
        ib = __builtin_amdgcn_readfirstlane(ib);
        const int ib1 = ib + 1 < KV_MAX_PAGES ? ib + 1 : ib;
        const unsigned long long p0 = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)tab_hi, ib) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)tab_lo, ib);
        const unsigned long long p1 = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)tab_hi, ib1) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)tab_lo, ib1);
        const unsigned long long pg = ok ? ((p >> KV_PAGE_SHIFT) == ib ? p0 : p1) : pg_zero;
        const ptrdiff_t page = (ptrdiff_t)(pg - reinterpret_cast<unsigned long long>(gbase));
        const int row = ((ok ? p : 0) + kv_rot(pg, kvh)) & (KV_PAGE_POS - 1);
        codes = page + (ptrdiff_t)code_off + (ptrdiff_t)row * HEAD_DIM;
        sc = page + (ptrdiff_t)scale_off + row;
    };
    struct KV8Reg { kv8_u4_t k, v; uint32_t ks, vs; };      // one position in flight: 16 K codes, 16 V codes, the two scale bytes
    // Every request is UNCONDITIONAL and the loop below is wave-uniform (a position past the range, or the new position,
    // reads the dummy row and the result is dropped): `s_waitcnt vmcnt` counts in issue order — k_attn_fused's reasons.
    auto request = [&](int pw, KV8Reg& r) {
        const int p = pw + (lane >> 3);
        ptrdiff_t codes, sc;
        row_of(p, pw, p < end && p != pos, codes, sc);
        r.k = *reinterpret_cast<const kv8_u4_t*>(gbase + codes + li * 16);
        r.v = *reinterpret_cast<const kv8_u4_t*>(gbase + codes + vd + li * 16);
        r.ks = *reinterpret_cast<const uint8_t*>(gbase + sc);
        r.vs = *reinterpret_cast<const uint8_t*>(gbase + sc + vd);
    };
    auto kv_st = [](auto* p, auto v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };

    // jobs 0..NREP-1: q heads; job NREP: the k head (+ raw v). The prologue's own loads go out FIRST, the K/V requests follow,
    // then the arithmetic (k_attn_fused).
    constexpr int NJ = (NREP + 1 + 3) / 4;
    const bool from_slices = a.qkv_part != nullptr;
    const __amdgpu_buffer_rsrc_t qkv_res = act_rsrc(a.qkv + (size_t)b * a.ld_qkv);
    float jx1[NJ], jx2[NJ], jv1[NJ], jv2[NJ], jn1[NJ], jn2[NJ];
    const float rc = a.rope_cos[(size_t)pos * 64 + lane], rs = a.rope_sin[(size_t)pos * 64 + lane];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int j = wave + 4 * jj;
        jx1[jj] = jx2[jj] = jv1[jj] = jv2[jj] = jn1[jj] = jn2[jj] = 0.0f;
        if (j <= NREP) {
            const bool is_q = j < NREP;
            const int scol = is_q ? (kvh * NREP + j) * HEAD_DIM : QD + kvh * HEAD_DIM;
            const int vcol = QD + KD + kvh * HEAD_DIM;
            if (from_slices) {          // the k job brings its v along: one round trip
                const int cols[4] = {scol + lane, scol + lane + 64, is_q ? scol + lane : vcol + lane, is_q ? scol + lane + 64 : vcol + lane + 64};
                float o[4]; qkv_from_slices<float, 4>(a, b, cols, o);
                jx1[jj] = o[0]; jx2[jj] = o[1]; jv1[jj] = o[2]; jv2[jj] = o[3];
            } else {
                jx1[jj] = act_ld1(qkv_res, (scol + lane) * 4); jx2[jj] = act_ld1(qkv_res, (scol + lane + 64) * 4);
                if (!is_q) { jv1[jj] = act_ld1(qkv_res, (vcol + lane) * 4); jv2[jj] = act_ld1(qkv_res, (vcol + lane + 64) * 4); }
            }
            const float* nw = is_q ? a.q_norm_w : a.k_norm_w;
            jn1[jj] = nw[lane]; jn2[jj] = nw[lane + 64];
        }
    }
    // one row of the new position (elements lane, lane + 64 of x): quantised by the format's rule; LDS gets the DEQUANTISED
    // values — the position is attended as the cache will hold it — and the split that owns `pos` stores codes and scale byte
    auto append = [&](float x1, float x2, float* s_row, ptrdiff_t codes, ptrdiff_t sc, bool store) {
        const int ex = kv8_exponent(kv8_wave_max(fmaxf(fabsf(x1), fabsf(x2))));
        const float inv = kv8_pow2(-ex);
        const uint32_t c2 = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x1 * inv, x2 * inv, 0, false);
        const kv8_f2_t dq = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c2, kv8_pow2(ex), false);
        s_row[lane] = dq[0]; s_row[lane + 64] = dq[1];
        if (store) {
            uint8_t* row = reinterpret_cast<uint8_t*>(const_cast<char*>(gbase) + codes);
            kv_st(&row[lane], (uint8_t)(c2 & 0xffu)); kv_st(&row[lane + 64], (uint8_t)((c2 >> 8) & 0xffu));
            if (lane == 0) kv_st(reinterpret_cast<uint8_t*>(const_cast<char*>(gbase) + sc), (uint8_t)(ex + 127));
        }
    };
    auto prologue_math = [&]() {
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = wave + 4 * jj;
            if (j > NREP) continue;
            const bool is_q = j < NREP;
            float x1 = jx1[jj], x2 = jx2[jj];
            const float ss = wave_sum(x1 * x1 + x2 * x2);
            const float den = sqrtf(ss / (float)HEAD_DIM + a.eps);
            x1 = x1 / den * jn1[jj];
            x2 = x2 / den * jn2[jj];
            const float o1 = sub_rn(mul_rn(x1, rc), mul_rn(x2, rs));
            const float o2 = add_rn(mul_rn(x2, rc), mul_rn(x1, rs));
            if (is_q) { s_q[j][lane] = o1; s_q[j][lane + 64] = o2; }
            else {
                ptrdiff_t codes, sc;
                row_of(pos, pos, true, codes, sc);
                const bool own = split == pos / chunk;
                append(o1, o2, s_k, codes, sc, own);
                append(jv1[jj], jv2[jj], s_v, codes + (ptrdiff_t)vd, sc + (ptrdiff_t)vd, own);
            }
        }
        zero_job(a.zero, a.zero_n, (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, gridDim.x * gridDim.y * gridDim.z, tid, 256);
        __syncthreads();
        Q3T(1);
    };
    float q[NREP][16], acc[NREP][16], m[NREP], l[NREP];
    auto consume = [&](int pw, const KV8Reg& r) {
        const int p = pw + (lane >> 3);
        if (p >= end) return;                                     // (uniform over the 8 lanes of a row: the DPP steps stay inside it)
        float kk[16], vv[16];
        if (p == pos) {                                            // the new position: from LDS
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<float4*>(&kk[4 * i]) = *reinterpret_cast<const float4*>(&s_k[li * 16 + 4 * i]);
                *reinterpret_cast<float4*>(&vv[4 * i]) = *reinterpret_cast<const float4*>(&s_v[li * 16 + 4 * i]);
            }
        } else {
            const float ksc = __uint_as_float(r.ks << 23), vsc = __uint_as_float(r.vs << 23);
#pragma unroll
            for (int i = 0; i < 4; ++i) { kv8_dequant4(r.k[i], ksc, &kk[4 * i]); kv8_dequant4(r.v[i], vsc, &vv[4 * i]); }
        }
#pragma unroll
        for (int rr = 0; rr < NREP; ++rr) {
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) s += q[rr][i] * kk[i];
            s = kv8_sum8(s) * scale;
            const float mn = fmaxf(m[rr], s);
            const float corr = expf(m[rr] - mn);
            const float pe = expf(s - mn);
            l[rr] = l[rr] * corr + pe;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rr][i] = acc[rr][i] * corr + pe * vv[i];
            m[rr] = mn;
        }
    };
    {
        // three register sets in rotation, the loop unrolled by three so that no set is ever copied: a group asks for
        // positions p, p + 32, p + 64; the first two go out before the prologue's arithmetic (k_attn_fused)
        KV8Reg A, B, C;
        int pw = start + wave * 8;
        request(pw, A);
        request(pw + 32, B);
        prologue_math();
#pragma unroll
        for (int rr = 0; rr < NREP; ++rr) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&q[rr][4 * i]) = *reinterpret_cast<const float4*>(&s_q[rr][li * 16 + 4 * i]);
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rr][i] = 0.0f;
            m[rr] = -INFINITY; l[rr] = 0.0f;
        }
        for (; pw < end; pw += 96) {
            request(pw + 64, C); consume(pw, A);
            if (pw + 32 >= end) break;
            request(pw + 96, A); consume(pw + 32, B);
            if (pw + 64 >= end) break;
            request(pw + 128, B); consume(pw + 64, C);
        }
    }
    Q3T(2);
    // cross-group merge through LDS in fixed group order, RP q heads per pass (32 groups x 128 floats per head)
#pragma unroll
    for (int r0 = 0; r0 < NREP; r0 += RP) {
        if (r0 > 0) __syncthreads();
#pragma unroll
        for (int rr = 0; rr < RP; ++rr) {
            if (li == 0) { sm_m[rr][grp] = m[r0 + rr]; sm_l[rr][grp] = l[r0 + rr]; }
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&sm_acc[rr][grp][li * 16 + 4 * i]) = *reinterpret_cast<const float4*>(&acc[r0 + rr][4 * i]);
        }
        __syncthreads();
        if (tid < RP * HEAD_DIM) {
            const int rr = tid / HEAD_DIM, d = tid % HEAD_DIM;
            float M = -INFINITY;
#pragma unroll
            for (int g = 0; g < 32; ++g) M = fmaxf(M, sm_m[rr][g]);
            float L = 0.0f, Av = 0.0f;
            if (M != -INFINITY) {
#pragma unroll
                for (int g = 0; g < 32; ++g) {
                    const float wgt = sm_m[rr][g] == -INFINITY ? 0.0f : expf(sm_m[rr][g] - M);
                    L += sm_l[rr][g] * wgt;
                    Av += sm_acc[rr][g][d] * wgt;
                }
            }
            const int h = kvh * NREP + r0 + rr;
            if (a.n_splits == 1) {
                act_st1(act_rsrc(a.out), (b * a.ld_out + h * HEAD_DIM + d) * 4, Av / L);
            } else {
                const __amdgpu_buffer_rsrc_t rec = act_rsrc(a.part + (((size_t)b * a.nh + h) * a.n_splits + split) * PART_STRIDE);
                act_st1(rec, d * 4, Av);
                if (d == 0) { act_st1(rec, HEAD_DIM * 4, M); act_st1(rec, (HEAD_DIM + 1) * 4, L); }
            }
        }
    }
    Q3T(3); act_drain(); Q3T_W(4); Q3T_FLUSH(a, (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

hipError_t launch_attn_kv8(const AttnArgs& a, hipStream_t st) {
    // the folded gather is the code predictor's (never paged); rows of one sequence depend on each other's K/V; no contiguous form
    if (a.g_logits || a.rows_per_seq > 1 || !a.kv_pages) return hipErrorNotSupported;
    const int nrep = a.nkv > 0 ? a.nh / a.nkv : 0;
    if (a.n_splits < 1 || a.n_splits > 255 || a.nh > 255 || a.nkv < 1 || a.nkv > 255 || a.kv_vdelta > 0x7fffffffu || a.B < 1) return hipErrorInvalidValue;
    if (a.qkv_part && (a.qkv_S < 1 || a.qkv_S > 8)) return hipErrorInvalidValue;
    dim3 grid(a.n_splits, a.nkv, a.B);
    const int pk = a.n_splits | (a.nkv << 8) | (a.nh << 16);
    const bool few = a.kv_row_pages > 0 && a.kv_row_pages <= 8;
#define Q3_AK8(R, P) hipLaunchKernelGGL((k_attn_kv8<R, P>), grid, dim3(256), 0, st, a.pos_dev, a.kv_pages, a.kv_layer_off, a.qkv, a.q_norm_w, a.k_norm_w, (int)a.kv_vdelta, pk, a)
    if (nrep == 1) { if (few) Q3_AK8(1, 1); else Q3_AK8(1, 2); }
    else if (nrep == 2) { if (few) Q3_AK8(2, 1); else Q3_AK8(2, 2); }
    else if (nrep == 4) { if (few) Q3_AK8(4, 1); else Q3_AK8(4, 2); }
    else return hipErrorInvalidValue;
#undef Q3_AK8
    return hipGetLastError();
}

// f32 pages -> KV8 pages (the prefill always runs on f32 pages; a KV8 session converts once, when its prompt is in): grid
// (pages, layers * nkv * 2), one 128 x 128 run per workgroup, one wave per row and four rows of a wave in flight; a lane holds
// two neighbouring elements, the amax is a wave reduction, and rows move from the source page's rotation to the destination's.
__global__ __launch_bounds__(256) void k_kv_pages_to_fp8(const unsigned long long* __restrict__ src_pages, const unsigned long long* __restrict__ dst_pages,
                                                         int nkv, size_t src_layer_stride, size_t src_v_delta, size_t dst_layer_stride, size_t dst_v_delta) {
    const int pgi = blockIdx.x, run = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int is_v = run & 1, kvh = (run >> 1) % nkv, layer = (run >> 1) / nkv;
    const unsigned long long sp = src_pages[pgi], dp = dst_pages[pgi];
    const float* src = reinterpret_cast<const float*>(sp) + (size_t)layer * src_layer_stride + (is_v ? src_v_delta : 0) + (size_t)kvh * KV8_RUN_CODES;
    uint8_t* run8 = reinterpret_cast<uint8_t*>(dp) + (size_t)layer * dst_layer_stride + (is_v ? dst_v_delta : 0);
    uint8_t* dst = run8 + (size_t)kvh * KV8_RUN_CODES;
    uint8_t* dsc = run8 + (size_t)nkv * KV8_RUN_CODES + (size_t)kvh * KV_PAGE_POS;
    const int rsrc = kv_rot(sp, kvh), rdst = kv_rot(dp, kvh);
    for (int p0 = wave * 4; p0 < KV_PAGE_POS; p0 += 16) {
        float2 x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const float2*>(src + (size_t)((p0 + i + rsrc) & (KV_PAGE_POS - 1)) * HEAD_DIM + lane * 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ex = kv8_exponent(kv8_wave_max(fmaxf(fabsf(x[i].x), fabsf(x[i].y))));
            const float inv = kv8_pow2(-ex);
            const uint32_t c2 = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[i].x * inv, x[i].y * inv, 0, false);
            const int row = (p0 + i + rdst) & (KV_PAGE_POS - 1);
            *reinterpret_cast<uint16_t*>(dst + (size_t)row * HEAD_DIM + lane * 2) = (uint16_t)(c2 & 0xffffu);
            if (lane == 0) dsc[row] = (uint8_t)(ex + 127);
        }
    }
}
hipError_t launch_kv_pages_to_fp8(const unsigned long long* src_pages, const unsigned long long* dst_pages, int n_pages, int n_layers, int nkv,
                                  size_t src_layer_stride, size_t src_v_delta, size_t dst_layer_stride, size_t dst_v_delta, hipStream_t st) {
    if (n_pages < 1) return hipSuccess;
    if (!src_pages || !dst_pages || n_layers < 1 || nkv < 1 || (long long)n_layers * nkv * 2 > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_kv_pages_to_fp8, dim3(n_pages, n_layers * nkv * 2), dim3(256), 0, st, src_pages, dst_pages, nkv, src_layer_stride, src_v_delta,
                       dst_layer_stride, dst_v_delta);
    return hipGetLastError();
}

}  // namespace q3
