// q3_testapi.hip — low-level entry points of the parity tests, submission / profiling read-outs, bench.py roofline replays
// (one of the units of the engine: q3_engine.h says which holds what)
#include "q3_engine.h"

extern "C" q3_status q3_talker_step(q3_session* s, const float* embeds_host, float* hidden_host, float* logits_host) {
    if (!s || !embeds_host) return set_err(Q3_INVALID_ARG, "null argument");
    if (!s->prefilled) return set_err(Q3_INVALID_ARG, "session not prefilled");
    const q3_config& c = s->m->cfg;
    HIPC(hipSetDevice(s->m->device));
    // the step writes K/V at `pos`: refuse BEFORE running when that slot does not exist (a step at pos == max_seq - 1 is valid)
    std::vector<int> posv(s->B);
    HIPC(sync_frames(s));
    HIPC(q3_hipMemcpy(posv.data(), s->pos, s->B * 4, hipMemcpyDeviceToHost));
    for (int p : posv) if (p >= s->max_seq) return set_err(Q3_KV_OVERFLOW, "KV cache full (%d)", s->max_seq);
    for (int b = 0; b < s->B; ++b) Q3C(kv_reserve_row(s, b, posv[(size_t)b] + 1));       // paged KV: the slot this step writes
    HIPC(hipMemcpyAsync(s->tb.X, embeds_host, (size_t)s->B * c.hidden * 4, hipMemcpyHostToDevice, s->stream));
    Q3C(talker_step(s, s->pos, 0, true));
    // advance positions by one (host-driven teacher forcing)
    HIPC(sync_frames(s));
    for (int& p : posv) p += 1;
    HIPC(q3_hipMemcpy(s->pos, posv.data(), s->B * 4, hipMemcpyHostToDevice));
    if (hidden_host) HIPC(q3_hipMemcpy(hidden_host, s->LASTH, (size_t)s->B * c.hidden * 4, hipMemcpyDeviceToHost));
    if (logits_host) HIPC(q3_hipMemcpy(logits_host, s->LOGITS, (size_t)s->B * c.codec_vocab * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_cp_generate(q3_session* s, const float* last_hidden_host, const float* sem_embed_host,
                                    uint32_t* codes15_host, float* cp_logits_host) {
    if (!s || !last_hidden_host || !codes15_host) return set_err(Q3_INVALID_ARG, "null argument");
    const q3_model* m = s->m; const q3_config& c = m->cfg;
    HIPC(hipSetDevice(m->device));
    // the semantic embedding is looked up from tok on device; teacher forcing passes it as an embedding
    // row, so run pass 1 from an explicit buffer: temporarily stage it through CP_IN/cb.X.
    const int B = s->B, H = c.hidden, CH = c.cp_hidden, V = c.cp_vocab;
    HIPC(hipMemcpyAsync(s->LASTH, last_hidden_host, (size_t)B * H * 4, hipMemcpyHostToDevice, s->stream));
    const LmDims d = cp_dims(c);
    float* sem_dev = nullptr;
    if (sem_embed_host) { HIPC(hipMalloc((void**)&sem_dev, (size_t)B * H * 4)); HIPC(q3_hipMemcpy(sem_dev, sem_embed_host, (size_t)B * H * 4, hipMemcpyHostToDevice)); }
    q3_status st = Q3_OK;
    auto run = [&]() -> q3_status {
        for (int p = 0; p < c.n_groups; ++p) {
            CpGatherArgs g{};
            g.pass = p; g.last_hidden = s->LASTH; g.H = H; g.codec_emb = m->codec_emb; g.tok = s->tok;
            g.cp_emb = p >= 2 ? m->cp_emb[p - 2] : nullptr;
            g.cp_logits = p >= 2 ? s->CP_LOGITS + (size_t)(p - 2) * B * V : nullptr;
            g.cp_vocab = V; g.codes = s->codes; g.frame_idx = s->frame_idx; g.max_frames = s->max_frames; g.B = B;
            float* dst = m->mtp_w.t1 ? s->CP_IN : s->cb.X; const int ld = m->mtp_w.t1 ? H : CH;
            g.out = dst; g.ld_out = ld;
            if (p == 1 && sem_dev) HIPC(launch_copy_rows(sem_dev, H, dst, ld, B, H, s->stream));
            else HIPC(launch_cp_gather(g, s->stream));
            if (m->mtp_w.t1) {
                LinArgs a;
                a.N = CH; a.K = H; set_w(a, m->mtp_w, B, CH, H); a.x = s->CP_IN; a.ldx = H; a.bias = m->mtp_b; a.y = s->cb.X; a.ldy = CH; a.M = B; a.epi = EPI_NONE;
                HIPC(launch_linear(a, s->stream));
            }
            for (int i = 0; i < c.cp_layers; ++i)
                Q3C(lm_layer(s, d, m->cl[i], s->cb, s->ckcache + (size_t)i * s->ckv_layer_stride, s->cvcache + (size_t)i * s->ckv_layer_stride,
                             c.n_groups + 1, nullptr, p, 1));
            if (p >= 1) {
                LinArgs h;
                h.N = V; h.K = CH; set_w(h, m->cp_head[p - 1], B, V, CH); h.x = s->cb.X; h.ldx = CH; h.norm_w = m->cp_norm; h.eps = c.rms_eps;
                h.y = s->CP_LOGITS + (size_t)(p - 1) * B * V; h.ldy = V; h.M = B; h.epi = EPI_NONE;
                HIPC(launch_linear(h, s->stream));
            }
        }
        HIPC(sync_frames(s));
        return Q3_OK;
    };
    st = run();
    if (sem_dev) hipFree(sem_dev);
    Q3C(st);
    std::vector<float> lg((size_t)15 * B * V);
    HIPC(q3_hipMemcpy(lg.data(), s->CP_LOGITS, lg.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
        for (int g = 0; g < 15; ++g) {
            const float* row = &lg[((size_t)g * B + b) * V];
            int best = 0; for (int i = 1; i < V; ++i) if (row[i] > row[best]) best = i;
            codes15_host[(size_t)b * 15 + g] = (uint32_t)best;
            if (cp_logits_host) memcpy(cp_logits_host + ((size_t)b * 15 + g) * V, row, (size_t)V * 4);
        }
    return Q3_OK;
}

extern "C" q3_status q3_frame_embed(q3_model* m, uint32_t sem_token, const uint32_t* codes15, const float* text_add_host, float* out_host) {
    if (!m || !m->finalized || !codes15 || !text_add_host || !out_host) return set_err(Q3_INVALID_ARG, "bad argument");
    const q3_config& c = m->cfg;
    HIPC(hipSetDevice(m->device));
    const int H = c.hidden, V = c.cp_vocab;
    if (sem_token >= (uint32_t)c.codec_vocab) return set_err(Q3_INVALID_ARG, "semantic token out of range");
    DevPool pool;
    float *rows, *logits, *out; uint32_t *tok, *codes; int *zero, *one;
    HIPC(pool.alloc(&rows, (size_t)H)); HIPC(pool.alloc(&logits, (size_t)V)); HIPC(pool.alloc(&out, (size_t)H));
    HIPC(pool.alloc(&tok, 1)); HIPC(pool.alloc(&codes, 16)); HIPC(pool.alloc(&zero, 1)); HIPC(pool.alloc(&one, 1));
    // codes 0..13 pre-written; code 14 enters through a one-hot logits row
    uint32_t frame[16] = {0};
    for (int g = 0; g < 14; ++g) { if (codes15[g] >= (uint32_t)V) return set_err(Q3_INVALID_ARG, "code out of range"); frame[1 + g] = codes15[g]; }
    if (codes15[14] >= (uint32_t)V) return set_err(Q3_INVALID_ARG, "code out of range");
    std::vector<float> lg((size_t)V, 0.0f); lg[codes15[14]] = 1.0f;
    const int h_one = 1;
    HIPC(q3_hipMemcpy(rows, text_add_host, (size_t)H * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(logits, lg.data(), (size_t)V * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(tok, &sem_token, 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(codes, frame, 64, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(one, &h_one, 4, hipMemcpyHostToDevice));
    FrameEmbedArgs f{};
    f.codec_emb = m->codec_emb; f.tok = tok; f.cp_logits_last = logits; f.cp_vocab = V;
    for (int g = 0; g < 15; ++g) f.cp_embs[g] = g < (int)m->cp_emb.size() ? m->cp_emb[(size_t)g] : nullptr;
    f.codes = codes; f.frame_idx = zero; f.max_frames = 1; f.text_rows = rows; f.trail_base = zero; f.trail_len = one; f.pad_row = zero;
    f.out = out; f.H = H; f.B = 1; f.n_acoustic = 15;
    HIPC(launch_frame_embed(f, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(out_host, out, (size_t)H * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_sample(int device, const float* logits_host, const uint8_t* seen_host, const float* u_host, int rows, int vocab,
                               const q3_options* o, int token_count, uint32_t* tokens_host) {
    if (!logits_host || !u_host || !o || !tokens_host || rows < 1) return set_err(Q3_INVALID_ARG, "bad argument");
    if (vocab < 2 || vocab > 4096) return set_err(Q3_UNSUPPORTED, "vocab %d unsupported by the device sampler (2..4096)", vocab);
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *lg, *u; uint8_t* seen = nullptr; uint32_t* tok;
    HIPC(pool.alloc(&lg, (size_t)rows * vocab)); HIPC(pool.alloc(&u, (size_t)rows)); HIPC(pool.alloc(&tok, (size_t)rows));
    HIPC(q3_hipMemcpy(lg, logits_host, (size_t)rows * vocab * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(u, u_host, (size_t)rows * 4, hipMemcpyHostToDevice));
    if (seen_host) { HIPC(pool.alloc(&seen, (size_t)rows * vocab)); HIPC(q3_hipMemcpy(seen, seen_host, (size_t)rows * vocab, hipMemcpyHostToDevice)); }
    SampleArgs a; memset(&a, 0, sizeof a);
    a.logits = lg; a.ld = vocab; a.seen = seen; a.u = u; a.u_stride = 1; a.tok = tok; a.token_count_static = token_count < 0 ? 0 : token_count;
    a.vocab = vocab; a.B = rows;
    a.apply_temp = (o->temperature != 1.0 && o->temperature > 0.0) ? 1 : 0;
    a.inv_temp = (float)(1.0 / o->temperature);
    a.greedy = o->temperature < 0.01 ? 1 : 0;
    a.top_k = o->top_k; a.use_top_p = (o->top_p < 1.0 && o->top_p > 0.0) ? 1 : 0; a.top_p = (float)o->top_p;
    const bool pen = token_count >= 0;     // token_count < 0: plain `sample` without the penalty pipeline
    a.use_rep = (pen && seen && o->repetition_penalty != 1.0 && !(fabs(o->repetition_penalty - 1.0) < 1e-9)) ? 1 : 0;
    a.rep_pen = (float)o->repetition_penalty; a.rep_inv = 1.0f / (float)o->repetition_penalty;
    a.eos_id = pen ? o->eos_token_id : -1; a.min_new_tokens = pen ? o->min_new_tokens : 0; a.codec_eos = CODEC_EOS; a.use_suppress = pen ? 1 : 0;
    HIPC(launch_sample(a, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(tokens_host, tok, (size_t)rows * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_fused_residual_rmsnorm(int device, int dtype, const void* x_host, const void* res_host, const void* w_host,
                                               int rows, int cols, float eps, void* normed_host, void* sum_host) {
    if (!x_host || !res_host || !w_host || !normed_host || !sum_host || rows < 1 || cols < 1) return set_err(Q3_INVALID_ARG, "bad argument");
    if (dtype != Q3_DTYPE_F32 && dtype != Q3_DTYPE_BF16) return set_err(Q3_UNSUPPORTED, "dtype %d unsupported", dtype);
    HIPC(hipSetDevice(device));
    const size_t es = dtype == Q3_DTYPE_F32 ? 4 : 2, n = (size_t)rows * cols;
    DevPool pool;
    char *x, *r, *w, *nm, *sm;
    HIPC(pool.alloc(&x, n * es)); HIPC(pool.alloc(&r, n * es)); HIPC(pool.alloc(&w, (size_t)cols * es)); HIPC(pool.alloc(&nm, n * es)); HIPC(pool.alloc(&sm, n * es));
    HIPC(q3_hipMemcpy(x, x_host, n * es, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(r, res_host, n * es, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(w, w_host, (size_t)cols * es, hipMemcpyHostToDevice));
    if (dtype == Q3_DTYPE_F32) HIPC(launch_fused_residual_rmsnorm_f32((float*)x, (float*)r, (float*)w, (float*)nm, (float*)sm, rows, cols, eps, 0));
    else HIPC(launch_fused_residual_rmsnorm_bf16((uint16_t*)x, (uint16_t*)r, (uint16_t*)w, (uint16_t*)nm, (uint16_t*)sm, rows, cols, eps, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(normed_host, nm, n * es, hipMemcpyDeviceToHost)); HIPC(q3_hipMemcpy(sum_host, sm, n * es, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_linear(int device, const float* x_host, const uint16_t* w_host, const float* bias_host, int M, int N, int K, float* y_host) {
    if (!x_host || !w_host || !y_host || M < 1 || N < 1 || K < 8 || K % 8) return set_err(Q3_INVALID_ARG, "bad argument (K must be a multiple of 8)");
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *x, *y, *b = nullptr; uint16_t* w;
    // the engine's own choice (pick_mode): 4-row tiles for narrow projections at small M — not for short-K wide ones, not beyond 16 rows
    const int mode = (M <= 16 && N < 4096 && !short_k_wide(N, K) && (M <= 2 || (N <= 1024 && M <= 8))) ? 2 : 1;
    const size_t wt_elems = tiled_elems(mode, N, K);
    std::vector<uint16_t> wt(wt_elems);
    retile_bf16(w_host, N, K, wt.data(), mode);
    HIPC(pool.alloc(&x, (size_t)M * K)); HIPC(pool.alloc(&y, (size_t)M * N)); HIPC(pool.alloc(&w, wt_elems));
    HIPC(q3_hipMemcpy(x, x_host, (size_t)M * K * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(w, wt.data(), wt_elems * 2, hipMemcpyHostToDevice));
    if (bias_host) { HIPC(pool.alloc(&b, (size_t)N)); HIPC(q3_hipMemcpy(b, bias_host, (size_t)N * 4, hipMemcpyHostToDevice)); }
    const int step = mode == 1 ? Q3_MAX_BATCH : 16;          // up to 64 rows per launch on the 16-row tiles (wide-session kernels beyond 16)
    float* ws = nullptr; size_t ws_bytes = 0;
    if (M > 16 && N % 128 == 0 && K % 128 == 0) { ws_bytes = gemm_wide_ws_bytes(M < step ? M : step, N, K, EPI_NONE); HIPC(pool.alloc(&ws, ws_bytes / 4)); }
    for (int m0 = 0; m0 < M; m0 += step) {
        LinArgs a;
        a.W = w; a.N = N; a.K = K; a.x = x + (size_t)m0 * K; a.ldx = K; a.bias = b; a.y = y + (size_t)m0 * N; a.ldy = N; a.M = (M - m0) < step ? (M - m0) : step; a.epi = EPI_NONE;
        a.tiled = mode; a.Kpad = kpad_for(mode, K); a.ws = ws; a.ws_bytes = ws_bytes;
        HIPC(launch_linear(a, 0));
    }
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(y_host, y, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// One launch_linear call through a complete LinArgs (op-level tests of every GEMV family: tests/test_gpu_linear_paths.py).
// A launch the dispatcher refuses comes back as a status — never another kernel in its place — and leaves the host y alone.
extern "C" q3_status q3_linear_ex(int device, const q3_linear_ex_args* p) {
    if (!p || !p->x || !p->w || !p->y) return set_err(Q3_INVALID_ARG, "q3_linear_ex: null argument");
    const int M = p->M, N = p->N, K = p->K;
    if (M < 1 || M > Q3_MAX_BATCH || N < 1 || K < 8 || K % 8) return set_err(Q3_INVALID_ARG, "q3_linear_ex: bad shape (1 <= M <= %d, K a multiple of 8)", Q3_MAX_BATCH);
    if (p->ldx < K || p->ldx % 4 || p->ldy < N || p->M_alloc < M) return set_err(Q3_INVALID_ARG, "q3_linear_ex: bad pitch (ldx >= K, ldx %% 4 == 0, ldy >= N, M_alloc >= M)");
    if (p->epi < EPI_NONE || p->epi > EPI_SWIGLU || p->tiled < -1 || p->tiled > 2 || p->ksplit < 1) return set_err(Q3_INVALID_ARG, "q3_linear_ex: epi 0..3, tiled -1..2, ksplit >= 1");
    if (p->epi == EPI_SWIGLU && !p->w2) return set_err(Q3_INVALID_ARG, "q3_linear_ex: SwiGLU needs a second matrix");
    if (p->epi == EPI_RESID && (!p->resid || p->ldr < N)) return set_err(Q3_INVALID_ARG, "q3_linear_ex: residual epilogue needs resid with ldr >= N");
    if (p->zero_n < 0 || p->zero_n % 4 || p->zero_guard < 0 || (p->zero_n > 0 && !p->zero_buf)) return set_err(Q3_INVALID_ARG, "q3_linear_ex: zero_n must be a multiple of 4 with a buffer");
    int mode = p->tiled;
    if (mode < 0) mode = (M <= 16 && N < 4096 && !short_k_wide(N, K) && (M <= 2 || (N <= 1024 && M <= 8))) ? 2 : 1;      // pick_mode
    if (mode == 0 && p->ksplit != 1) return set_err(Q3_UNSUPPORTED, "q3_linear_ex: the row-major kernel has no split-K form");
    HIPC(hipSetDevice(device));
    DevPool pool;
    const int nmat = p->epi == EPI_SWIGLU ? 2 : 1;
    const size_t welems = mode == 0 ? (size_t)N * K : tiled_elems(mode, N, K);
    uint16_t* w; float *x, *y, *b = nullptr, *nw = nullptr, *res = nullptr, *zb = nullptr, *ws = nullptr;
    HIPC(pool.alloc(&w, welems * nmat));
    for (int i = 0; i < nmat; ++i) {
        const uint16_t* src = i ? p->w2 : p->w;
        if (mode == 0) HIPC(q3_hipMemcpy(w + (size_t)i * welems, src, welems * 2, hipMemcpyHostToDevice));
        else {
            std::vector<uint16_t> wt(welems);
            retile_bf16(src, N, K, wt.data(), mode);
            HIPC(q3_hipMemcpy(w + (size_t)i * welems, wt.data(), welems * 2, hipMemcpyHostToDevice));
        }
    }
    const size_t xn = (size_t)M * p->ldx, yn = (size_t)p->M_alloc * p->ldy;
    HIPC(pool.alloc(&x, xn)); HIPC(q3_hipMemcpy(x, p->x, xn * 4, hipMemcpyHostToDevice));
    HIPC(pool.alloc(&y, yn)); HIPC(q3_hipMemcpy(y, p->y, yn * 4, hipMemcpyHostToDevice));
    if (p->bias) { HIPC(pool.alloc(&b, (size_t)N)); HIPC(q3_hipMemcpy(b, p->bias, (size_t)N * 4, hipMemcpyHostToDevice)); }
    if (p->norm_w) { HIPC(pool.alloc(&nw, (size_t)K)); HIPC(q3_hipMemcpy(nw, p->norm_w, (size_t)K * 4, hipMemcpyHostToDevice)); }
    if (p->epi == EPI_RESID) { HIPC(pool.alloc(&res, (size_t)M * p->ldr)); HIPC(q3_hipMemcpy(res, p->resid, (size_t)M * p->ldr * 4, hipMemcpyHostToDevice)); }
    const size_t zn = (size_t)p->zero_n + p->zero_guard;
    if (p->zero_n > 0) { HIPC(pool.alloc(&zb, zn)); HIPC(q3_hipMemcpy(zb, p->zero_buf, zn * 4, hipMemcpyHostToDevice)); }
    size_t ws_bytes = 0;
    if (p->use_ws && M > 16) {      // outside the GEMM's shapes the workspace is still passed: the dispatcher itself must fall back to k_gemv_wide
        if (N >= 128 && K >= 128) ws_bytes = gemm_wide_ws_bytes(M, N, K, p->epi);
        HIPC(pool.alloc(&ws, (ws_bytes ? ws_bytes : 256) / 4));
    }
    // split-K adds into y: zeros under the M x N result only, so that the caller's sentinels around it survive
    if (p->ksplit == 2) for (int m = 0; m < M; ++m) HIPC(q3_null_stream_memset(y + (size_t)m * p->ldy, (size_t)N * 4, m == M - 1));
    LinArgs a;
    a.W = w; a.W2 = nmat == 2 ? w + welems : nullptr; a.x = x; a.ldx = p->ldx; a.norm_w = nw; a.eps = p->eps; a.bias = b;
    a.resid = res; a.ldr = res ? p->ldr : 0; a.y = y; a.ldy = p->ldy; a.M = M; a.N = N; a.K = K; a.epi = p->epi;
    a.tiled = mode; a.Kpad = mode == 0 ? K : kpad_for(mode, K); a.ksplit = p->ksplit;
    a.zero = zb; a.zero_n = zb ? p->zero_n : 0; a.ws = ws; a.ws_bytes = ws_bytes;
    HIPC(q3_hipDeviceSynchronize());
    const hipError_t e = launch_linear(a, 0);
    if (e == hipErrorInvalidValue || e == hipErrorNotSupported) {
        (void)hipGetLastError();
        return set_err(Q3_UNSUPPORTED, "q3_linear_ex: launch_linear refused M=%d N=%d K=%d epi=%d norm=%d tiled=%d ksplit=%d (%s)", M, N, K, p->epi, nw ? 1 : 0,
                       mode, p->ksplit, hipGetErrorString(e));
    }
    HIPC(e);
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(p->y, y, yn * 4, hipMemcpyDeviceToHost));
    if (zb) HIPC(q3_hipMemcpy(p->zero_buf, zb, zn * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// One decode-attention step over a contiguous cache (tests/test_gpu_attention_op.py): q/k-norm + RoPE + append + GQA attention
// through the one-launch kernel (+ merge), the three-launch path, or the code predictor's single-wave kernel.
extern "C" q3_status q3_attn_step(int device, const q3_attn_step_args* p) {
    if (!p || !p->pos || !p->qkv || !p->q_norm_w || !p->k_norm_w || !p->rope_cos || !p->rope_sin || !p->kcache || !p->vcache || !p->out)
        return set_err(Q3_INVALID_ARG, "q3_attn_step: null argument");
    const int B = p->B, nh = p->nh, nkv = p->nkv;
    if (p->variant < 0 || p->variant > 2) return set_err(Q3_INVALID_ARG, "q3_attn_step: variant 0..2");
    if (B < 1 || B > Q3_MAX_BATCH || nkv < 1 || nh < nkv || nh > 64 || nh % nkv || p->max_seq < 1 || p->n_splits < 1 || p->n_splits > MAX_SPLITS)
        return set_err(Q3_INVALID_ARG, "q3_attn_step: bad shape");
    const int nrep = nh / nkv;
    if (nrep != 1 && nrep != 2 && nrep != 4) return set_err(Q3_UNSUPPORTED, "q3_attn_step: heads / kv heads must be 1, 2 or 4");
    for (int b = 0; b < B; ++b) if (p->pos[b] < 0 || p->pos[b] >= p->max_seq) return set_err(Q3_INVALID_ARG, "q3_attn_step: pos[%d] = %d outside the cache (%d)", b, p->pos[b], p->max_seq);
    if (p->variant == 2) for (int b = 1; b < B; ++b) if (p->pos[b] != p->pos[0]) return set_err(Q3_INVALID_ARG, "q3_attn_step: variant 2 takes one position for every row");
    HIPC(hipSetDevice(device));
    DevPool pool;
    const int ld_qkv = (nh + 2 * nkv) * HEAD_DIM, QD = nh * HEAD_DIM;
    const size_t cn = (size_t)B * nkv * p->max_seq * HEAD_DIM, rn = (size_t)p->max_seq * 64;
    int* pos; float *qkv, *qw, *kw, *rc, *rs, *kv, *qbuf, *part, *out;
    HIPC(pool.alloc(&pos, (size_t)B)); HIPC(pool.alloc(&qkv, (size_t)B * ld_qkv)); HIPC(pool.alloc(&qw, (size_t)HEAD_DIM)); HIPC(pool.alloc(&kw, (size_t)HEAD_DIM));
    HIPC(pool.alloc(&rc, rn)); HIPC(pool.alloc(&rs, rn)); HIPC(pool.alloc(&kv, 2 * cn));       // K and V in one block: their distance fits every kernel's 32-bit form
    HIPC(pool.alloc(&qbuf, (size_t)B * QD)); HIPC(pool.alloc(&part, (size_t)B * nh * p->n_splits * PART_STRIDE)); HIPC(pool.alloc(&out, (size_t)B * QD));
    HIPC(q3_hipMemcpy(pos, p->pos, (size_t)B * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(qkv, p->qkv, (size_t)B * ld_qkv * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(qw, p->q_norm_w, HEAD_DIM * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(kw, p->k_norm_w, HEAD_DIM * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(rc, p->rope_cos, rn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(rs, p->rope_sin, rn * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(kv, p->kcache, cn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(kv + cn, p->vcache, cn * 4, hipMemcpyHostToDevice));
    AttnArgs t{};
    t.qkv = qkv; t.ld_qkv = ld_qkv; t.q_norm_w = qw; t.k_norm_w = kw; t.eps = p->eps; t.rope_cos = rc; t.rope_sin = rs;
    t.pos_dev = p->variant == 2 ? nullptr : pos; t.pos_static = p->variant == 2 ? p->pos[0] : 0;
    t.kcache = kv; t.vcache = kv + cn; t.max_seq = p->max_seq; t.qbuf = qbuf; t.part = part; t.out = out; t.ld_out = QD;
    t.B = B; t.nh = nh; t.nkv = nkv; t.n_splits = p->n_splits; t.rows_per_seq = 1;
    if (p->variant == 2 && !attn_cp_ok(t)) return set_err(Q3_UNSUPPORTED, "q3_attn_step: arguments outside launch_attn_cp (one split, position < 16, max_seq < 256)");
    HIPC(q3_hipDeviceSynchronize());
    if (p->variant == 0) {
        HIPC(launch_attn_fused(t, 0));
        if (p->n_splits > 1) HIPC(launch_attn_merge(t, 0));
    } else if (p->variant == 1) {
        HIPC(launch_qknorm_rope_kv(t, 0));
        HIPC(launch_attn_decode(t, 0));
        HIPC(launch_attn_merge(t, 0));
    } else HIPC(launch_attn_cp(t, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(p->out, out, (size_t)B * QD * 4, hipMemcpyDeviceToHost));
    HIPC(q3_hipMemcpy(p->kcache, kv, cn * 4, hipMemcpyDeviceToHost)); HIPC(q3_hipMemcpy(p->vcache, kv + cn, cn * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// ---- decode attention in the forms a session runs (tests/test_gpu_attention_forms.py) ----
// Slabs of KvPool's geometry for a test entry: nothing is taken from the pool object, it only answers run_floats / v_delta() /
// layer_stride() / slab_bytes(), so that the layout under test is the engine's. Every 32-bit word of a slab starts as a hash of its
// index; cache rows are scattered over that, and whatever differs from the image afterwards outside those rows is a stray write.
namespace {
struct TestSlabs {
    KvPool geo;
    std::vector<char*> dev;                          // one device block per slab (owned by the caller's DevPool)
    std::vector<std::vector<uint32_t>> img;          // what the slab holds (host)
    static uint32_t pattern(size_t slab, size_t word) {
        uint32_t x = (uint32_t)(word + slab * 0x632be5abu) * 2654435761u + 0x9e3779b9u;
        x ^= x >> 15; x *= 0x85ebca6bu; x ^= x >> 13;
        return x;
    }
    void shape(int n_layers, int nkv, size_t elem_bytes) { geo.n_layers = n_layers; geo.run_floats = (size_t)nkv * KV_PAGE_POS * HEAD_DIM; geo.elem_bytes = elem_bytes; }
    hipError_t add_slab(DevPool& pool) {             // (allocation only: a page's rotation depends on its address, so the images follow once all slabs exist)
        char* d = nullptr;
        const hipError_t e = pool.alloc(&d, geo.slab_bytes());
        if (e == hipSuccess) dev.push_back(d);
        return e;
    }
    void fill_pattern() {
        const size_t words = geo.slab_bytes() / 4;
        for (size_t s = 0; s < dev.size(); ++s) {
            img.emplace_back(words);
            for (size_t w = 0; w < words; ++w) img[s][w] = pattern(s, w);
        }
    }
    size_t slab_elems() const { return geo.slab_bytes() / geo.elem_bytes; }
    unsigned long long page(int slot) const {        // a page is named by the address of its layer-0 K run
        return (unsigned long long)(uintptr_t)dev[(size_t)(slot / KvPool::SLAB_SLOTS)] + (size_t)(slot % KvPool::SLAB_SLOTS) * geo.run_floats * geo.elem_bytes;
    }
    // element offset, within its slab, of the row that holds position p of (slot, layer, K | V, kv head)
    size_t row_elem(int slot, int layer, int is_v, int kvh, int p) const {
        return (size_t)layer * geo.layer_stride() + (is_v ? geo.v_delta() : 0) + (size_t)(slot % KvPool::SLAB_SLOTS) * geo.run_floats +
               ((size_t)kvh * KV_PAGE_POS + (size_t)((p + kv_rot(page(slot), kvh)) & (KV_PAGE_POS - 1))) * HEAD_DIM;
    }
    // one row of 128 values between a host f32 row and an image (f32 elements, or bf16 = the high halves)
    void put_row(std::vector<std::vector<uint32_t>>& im, int slot, size_t elem, const float* row) const {
        char* base = reinterpret_cast<char*>(im[(size_t)(slot / KvPool::SLAB_SLOTS)].data());
        if (geo.elem_bytes == 4) memcpy(base + elem * 4, row, HEAD_DIM * 4);
        else for (int d = 0; d < HEAD_DIM; ++d) { uint32_t u; memcpy(&u, row + d, 4); const uint16_t h = (uint16_t)(u >> 16); memcpy(base + (elem + d) * 2, &h, 2); }
    }
    void get_row(const std::vector<std::vector<uint32_t>>& im, int slot, size_t elem, float* row) const {
        const char* base = reinterpret_cast<const char*>(im[(size_t)(slot / KvPool::SLAB_SLOTS)].data());
        if (geo.elem_bytes == 4) memcpy(row, base + elem * 4, HEAD_DIM * 4);
        else for (int d = 0; d < HEAD_DIM; ++d) { uint16_t h; memcpy(&h, base + (elem + d) * 2, 2); const uint32_t u = (uint32_t)h << 16; memcpy(row + d, &u, 4); }
    }
    void copy_row(std::vector<std::vector<uint32_t>>& to, const std::vector<std::vector<uint32_t>>& from, int slot, size_t elem) const {
        const size_t s = (size_t)(slot / KvPool::SLAB_SLOTS);
        memcpy(reinterpret_cast<char*>(to[s].data()) + elem * geo.elem_bytes, reinterpret_cast<const char*>(from[s].data()) + elem * geo.elem_bytes, HEAD_DIM * geo.elem_bytes);
    }
    hipError_t upload() const {
        for (size_t s = 0; s < dev.size(); ++s) { const hipError_t e = q3_hipMemcpy(dev[s], img[s].data(), geo.slab_bytes(), hipMemcpyHostToDevice); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
    hipError_t download(std::vector<std::vector<uint32_t>>& got) const {
        got.resize(dev.size());
        for (size_t s = 0; s < dev.size(); ++s) {
            got[s].resize(img[s].size());
            const hipError_t e = q3_hipMemcpy(got[s].data(), dev[s], geo.slab_bytes(), hipMemcpyDeviceToHost); if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // elements of `got` that differ from the image: count and the first offset (slab * slab_elems + element)
    void strays(const std::vector<std::vector<uint32_t>>& got, long long* out) const {
        long long n = 0, first = -1;
        for (size_t s = 0; s < img.size(); ++s) {
            if (memcmp(img[s].data(), got[s].data(), geo.slab_bytes()) == 0) continue;
            const char* a = reinterpret_cast<const char*>(img[s].data()); const char* b = reinterpret_cast<const char*>(got[s].data());
            for (size_t e = 0; e < slab_elems(); ++e)
                if (memcmp(a + e * geo.elem_bytes, b + e * geo.elem_bytes, geo.elem_bytes) != 0) { if (first < 0) first = (long long)(s * slab_elems() + e); ++n; }
        }
        out[0] = n; out[1] = first;
    }
};
bool slots_ok(const int* slots, int n, int limit) {
    std::vector<char> seen((size_t)limit, 0);
    for (int i = 0; i < n; ++i) { if (slots[i] < 0 || slots[i] >= limit || seen[(size_t)slots[i]]) return false; seen[(size_t)slots[i]] = 1; }
    return true;
}
}  // namespace

// One decode-attention step through a complete AttnArgs in any form lm_layer builds: contiguous / paged f32 / paged bf16 cache,
// q|k|v from a row, from K-slice sums or from a table row (folded gather), several rows per sequence, the zero side job. The
// launches are the session's own for the variant — a launcher's refusal is a status, never another kernel in its place.
extern "C" q3_status q3_attn_step_ex(int device, const q3_attn_step_ex_args* p) {
    if (!p || !p->pos || !p->q_norm_w || !p->k_norm_w || !p->rope_cos || !p->rope_sin || !p->kcache || !p->vcache || !p->out)
        return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: null argument");
    const int B = p->B, nh = p->nh, nkv = p->nkv, variant = p->variant, layout = p->layout, max_seq = p->max_seq;
    if (variant < 0 || variant > 3 || layout < 0 || layout > 2) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: variant 0..3, layout 0..2");
    if (B < 1 || B > Q3_MAX_BATCH || nkv < 1 || nh < nkv || nh > 64 || nh % nkv || max_seq < 1 || max_seq > (1 << 20) || p->n_splits < 1 || p->n_splits > MAX_SPLITS)
        return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: bad shape");
    const int nrep = nh / nkv;
    if (nrep != 1 && nrep != 2 && nrep != 4) return set_err(Q3_UNSUPPORTED, "q3_attn_step_ex: heads / kv heads must be 1, 2 or 4");
    const int rps = p->rows_per_seq <= 0 ? 1 : p->rows_per_seq;
    if (rps > 8 || B % rps) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: rows_per_seq 1..8, a divisor of B");
    if (rps > 1 && (variant == 0 || variant == 2)) return set_err(Q3_UNSUPPORTED, "q3_attn_step_ex: variants 0 and 2 take one row per sequence");
    if (variant == 3 && rps != 2) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: variant 3 takes exactly two rows per sequence");
    if (layout != 0 && variant >= 2) return set_err(Q3_UNSUPPORTED, "q3_attn_step_ex: variants 2 and 3 run on a contiguous cache only");
    if (layout == 2 && variant != 0) return set_err(Q3_UNSUPPORTED, "q3_attn_step_ex: only the one-launch kernel reads bf16 pages");
    const int n_seq = B / rps;
    for (int s = 0; s < n_seq; ++s)
        if (p->pos[s] < 0 || p->pos[s] > max_seq - rps) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: pos[%d] = %d (+ %d rows) outside the cache (%d)", s, p->pos[s], rps, max_seq);
    if (variant == 2) {
        for (int b = 1; b < B; ++b) if (p->pos[b] != p->pos[0]) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: variant 2 takes one position for every row");
        if (p->n_splits != 1 || p->pos[0] >= 16 || max_seq >= 256) return set_err(Q3_UNSUPPORTED, "q3_attn_step_ex: arguments outside launch_attn_cp (one split, position < 16, max_seq < 256)");
    }
    if (variant == 3) {
        for (int s = 0; s < n_seq; ++s) if (p->pos[s] != 0) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: variant 3 starts from an empty cache (pos 0)");
        if (p->n_splits != 1) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: variant 3 has no splits");
    }
    const int n_pg = (max_seq + KV_PAGE_POS - 1) / KV_PAGE_POS;
    const size_t cn = (size_t)n_seq * nkv * max_seq * HEAD_DIM;
    if (layout != 0) {
        if (max_seq > KV_MAX_PAGES * KV_PAGE_POS) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: a paged row holds at most %d positions", KV_MAX_PAGES * KV_PAGE_POS);
        if (p->n_layers < 1 || p->n_layers > 4 || p->layer < 0 || p->layer >= p->n_layers || p->n_slabs < 1 || p->n_slabs > 2)
            return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: n_layers 1..4, layer inside them, n_slabs 1..2");
        if (!p->page_slots || !p->stray) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: a paged layout needs page_slots and stray");
        if (p->kv_row_pages < 0 || p->kv_row_pages > KV_MAX_PAGES || (p->kv_row_pages >= 1 && p->kv_row_pages <= 8 && p->kv_row_pages < n_pg))
            return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: kv_row_pages 0..%d, and from 1 to 8 no fewer than the pages of max_seq (%d)", KV_MAX_PAGES, n_pg);
        if (!slots_ok(p->page_slots, n_seq * n_pg, KvPool::SLAB_SLOTS * p->n_slabs))
            return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: page_slots must be distinct slots of 0 .. %d", KvPool::SLAB_SLOTS * p->n_slabs - 1);
        if (layout == 2)
            for (size_t i = 0; i < cn; ++i) {
                uint32_t a, b; memcpy(&a, p->kcache + i, 4); memcpy(&b, p->vcache + i, 4);
                if ((a | b) & 0xffffu) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: cache element %zu is not exact in bf16", i);
            }
    }
    const bool slices = p->qkv_part != nullptr, g_l = p->g_logits != nullptr, g_t = p->g_tok != nullptr;
    if (slices && (variant == 1 || variant == 3)) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: slice sums belong to variants 0 and 2");
    if (g_l && (variant == 1 || variant == 3)) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: g_logits belongs to variants 0 and 2");
    if (g_t && variant != 3) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: g_tok belongs to variant 3");
    if (slices && g_l) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: slice sums and the folded gather exclude each other");
    if (slices && (!p->qkv_ssq || p->qkv_S < 1 || p->qkv_S > 8 || p->qkv_K < 1)) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: slice sums need qkv_ssq, qkv_S 1..8, qkv_K >= 1");
    if (g_l || g_t) {
        if (!p->g_qkv_tab || !p->g_proj_tab || !p->g_x) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: the gather needs g_qkv_tab, g_proj_tab and g_x");
        if (p->g_vocab < 1 || p->g_vocab > 65536 || p->g_proj_dim < 4 || p->g_proj_dim % 4 || p->g_ldx < p->g_proj_dim || p->g_ldx % 4 || p->g_ldx > 65536)
            return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: g_vocab 1..65536, g_proj_dim and g_ldx multiples of 4, g_proj_dim <= g_ldx <= 65536");
    }
    if (g_l) {
        if (!p->g_codes || !p->g_frame_idx || p->g_max_frames < 1 || p->g_max_frames > 4096 || p->g_code_slot < 0 || p->g_code_slot > 15)
            return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: g_logits needs g_codes, g_frame_idx, g_max_frames 1..4096, g_code_slot 0..15");
        for (int b = 0; b < B; ++b) if (p->g_frame_idx[b] < 0) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: g_frame_idx[%d] < 0", b);
    }
    if (g_t) for (int s = 0; s < n_seq; ++s) if (p->g_tok[s] >= (uint32_t)p->g_vocab) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: g_tok[%d] outside the table", s);
    if (!p->qkv && !slices && !g_l) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: null argument (qkv)");
    if (p->zero_n < 0 || p->zero_n % 4 || p->zero_guard < 0 || (p->zero_n > 0 && !p->zero_buf)) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: zero_n must be a multiple of 4 with a buffer");
    if (p->zero_n > 0 && variant == 1) return set_err(Q3_INVALID_ARG, "q3_attn_step_ex: the three-launch path has no zero side job");

    HIPC(hipSetDevice(device));
    DevPool pool;
    const int ld_qkv = (nh + 2 * nkv) * HEAD_DIM, QD = nh * HEAD_DIM;
    const size_t rn = (size_t)max_seq * 64;
    int* pos; float *qkv = nullptr, *qw, *kw, *rc, *rs, *kv = nullptr, *qbuf, *part, *out;
    unsigned long long* table = nullptr;
    TestSlabs slabs;
    // (slab, table, slab: with two slabs the pages of a row lie on both sides of the table the kernel forms their addresses from)
    if (layout != 0) {
        slabs.shape(p->n_layers, nkv, layout == 2 ? 2 : 4);
        for (int s = 0; s < p->n_slabs; ++s) {
            if (s == 1) HIPC(pool.alloc(&table, (size_t)n_seq * KV_MAX_PAGES));
            HIPC(slabs.add_slab(pool));
        }
        if (!table) HIPC(pool.alloc(&table, (size_t)n_seq * KV_MAX_PAGES));
        if (slabs.geo.v_delta() > 0x7fffffffu) return set_err(Q3_UNSUPPORTED, "q3_attn_step_ex: K -> V distance beyond the kernels' 32-bit form");
    } else HIPC(pool.alloc(&kv, 2 * cn));       // K and V in one block: their distance fits every kernel's 32-bit form
    HIPC(pool.alloc(&pos, (size_t)n_seq)); HIPC(pool.alloc(&qw, (size_t)HEAD_DIM)); HIPC(pool.alloc(&kw, (size_t)HEAD_DIM));
    HIPC(pool.alloc(&rc, rn)); HIPC(pool.alloc(&rs, rn));
    HIPC(pool.alloc(&qbuf, (size_t)B * QD)); HIPC(pool.alloc(&part, (size_t)B * nh * p->n_splits * PART_STRIDE)); HIPC(pool.alloc(&out, (size_t)B * QD));
    HIPC(q3_hipMemcpy(pos, p->pos, (size_t)n_seq * 4, hipMemcpyHostToDevice));
    if (p->qkv) { HIPC(pool.alloc(&qkv, (size_t)B * ld_qkv)); HIPC(q3_hipMemcpy(qkv, p->qkv, (size_t)B * ld_qkv * 4, hipMemcpyHostToDevice)); }
    HIPC(q3_hipMemcpy(qw, p->q_norm_w, HEAD_DIM * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(kw, p->k_norm_w, HEAD_DIM * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(rc, p->rope_cos, rn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(rs, p->rope_sin, rn * 4, hipMemcpyHostToDevice));
    auto cache_row = [&](float* c, int s, int g, int pp) { return c + (((size_t)s * nkv + g) * max_seq + pp) * HEAD_DIM; };
    auto each_row = [&](auto&& f) {             // every (sequence, kv head, position, K | V) of the logical cache with its slot and element offset
        for (int s = 0; s < n_seq; ++s) for (int g = 0; g < nkv; ++g) for (int pp = 0; pp < max_seq; ++pp) for (int v = 0; v < 2; ++v) {
            const int slot = p->page_slots[(size_t)s * n_pg + pp / KV_PAGE_POS];
            f(slot, slabs.row_elem(slot, p->layer, v, g, pp), cache_row(v ? p->vcache : p->kcache, s, g, pp));
        }
    };
    if (layout != 0) {
        slabs.fill_pattern();
        each_row([&](int slot, size_t elem, float* row) { slabs.put_row(slabs.img, slot, elem, row); });
        HIPC(slabs.upload());
        std::vector<unsigned long long> tab((size_t)n_seq * KV_MAX_PAGES);
        for (int s = 0; s < n_seq; ++s)
            for (int i = 0; i < KV_MAX_PAGES; ++i) tab[(size_t)s * KV_MAX_PAGES + i] = slabs.page(p->page_slots[(size_t)s * n_pg + (i < n_pg ? i : 0)]);      // beyond the row's pages: its first, as a session leaves them
        HIPC(q3_hipMemcpy(table, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
        if (p->rot_used)
            for (int s = 0; s < n_seq; ++s) for (int i = 0; i < n_pg; ++i) for (int g = 0; g < nkv; ++g)
                p->rot_used[((size_t)s * n_pg + i) * nkv + g] = kv_rot(slabs.page(p->page_slots[(size_t)s * n_pg + i]), g);
    } else {
        HIPC(q3_hipMemcpy(kv, p->kcache, cn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(kv + cn, p->vcache, cn * 4, hipMemcpyHostToDevice));
    }
    auto up = [&](const void* h, size_t bytes, void** d) -> q3_status {
        char* q; HIPC(pool.alloc(&q, bytes)); HIPC(q3_hipMemcpy(q, h, bytes, hipMemcpyHostToDevice)); *d = q;
        return Q3_OK;
    };
    AttnArgs t{};
    t.qkv = qkv; t.ld_qkv = ld_qkv; t.q_norm_w = qw; t.k_norm_w = kw; t.eps = p->eps; t.rope_cos = rc; t.rope_sin = rs;
    t.pos_dev = variant >= 2 ? nullptr : pos; t.pos_static = variant == 2 ? p->pos[0] : 0;
    t.max_seq = max_seq; t.qbuf = qbuf; t.part = part; t.out = out; t.ld_out = QD;
    t.B = B; t.nh = nh; t.nkv = nkv; t.n_splits = p->n_splits; t.rows_per_seq = rps;
    if (layout != 0) {
        t.kv_pages = table; t.kv_layer_off = (size_t)p->layer * slabs.geo.layer_stride(); t.kv_vdelta = slabs.geo.v_delta();
        t.kv_row_pages = p->kv_row_pages; t.kv_bf16 = layout == 2 ? 1 : 0;
    } else { t.kcache = kv; t.vcache = kv + cn; }
    void* d = nullptr;
    const size_t gx_rows = variant == 3 ? (size_t)n_seq : (size_t)B, zn = (size_t)p->zero_n + p->zero_guard;
    if (slices) {
        Q3C(up(p->qkv_part, (size_t)p->qkv_S * B * ld_qkv * 4, &d)); t.qkv_part = (const float*)d;
        Q3C(up(p->qkv_ssq, (size_t)p->qkv_S * B * 4, &d)); t.qkv_ssq = (const float*)d;
        t.qkv_S = p->qkv_S; t.qkv_K = p->qkv_K; t.qkv_eps = p->qkv_eps;
    }
    if (g_l || g_t) {
        Q3C(up(p->g_qkv_tab, (size_t)p->g_vocab * ld_qkv * 4, &d)); t.g_qkv_tab = (const float*)d;
        Q3C(up(p->g_proj_tab, (size_t)p->g_vocab * p->g_proj_dim * 4, &d)); t.g_proj_tab = (const float*)d;
        Q3C(up(p->g_x, gx_rows * p->g_ldx * 4, &d)); t.g_x = (float*)d;
        t.g_vocab = p->g_vocab; t.g_proj_dim = p->g_proj_dim; t.g_ldx = p->g_ldx;
    }
    if (g_l) {
        Q3C(up(p->g_logits, (size_t)B * p->g_vocab * 4, &d)); t.g_logits = (const float*)d;
        Q3C(up(p->g_codes, (size_t)B * p->g_max_frames * 16 * 4, &d)); t.g_codes = (uint32_t*)d;
        Q3C(up(p->g_frame_idx, (size_t)B * 4, &d)); t.g_frame_idx = (const int*)d;
        t.g_max_frames = p->g_max_frames; t.g_code_slot = p->g_code_slot;
    }
    if (g_t) { Q3C(up(p->g_tok, (size_t)n_seq * 4, &d)); t.g_tok = (const uint32_t*)d; }
    if (p->zero_n > 0) { Q3C(up(p->zero_buf, zn * 4, &d)); t.zero = (float*)d; t.zero_n = p->zero_n; }
    if (variant == 2 && !attn_cp_ok(t)) return set_err(Q3_UNSUPPORTED, "q3_attn_step_ex: arguments outside launch_attn_cp");
    HIPC(q3_hipDeviceSynchronize());
    hipError_t e = hipSuccess;
    if (variant == 0) {
        e = launch_attn_fused(t, 0);
        if (e == hipSuccess && p->n_splits > 1) e = launch_attn_merge(t, 0);
    } else if (variant == 1) {
        e = launch_qknorm_rope_kv(t, 0);
        if (e == hipSuccess) e = launch_attn_decode(t, 0);
        if (e == hipSuccess) e = launch_attn_merge(t, 0);
    } else if (variant == 2) e = launch_attn_cp(t, 0);
    else e = launch_attn_first2(t, 0);
    if (e == hipErrorInvalidValue || e == hipErrorNotSupported) {
        (void)hipGetLastError();
        (void)q3_hipDeviceSynchronize();
        return set_err(Q3_UNSUPPORTED, "q3_attn_step_ex: the launcher refused variant=%d layout=%d nh=%d nkv=%d splits=%d rows_per_seq=%d (%s)", variant, layout, nh, nkv,
                       p->n_splits, rps, hipGetErrorString(e));
    }
    HIPC(e);
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(p->out, out, (size_t)B * QD * 4, hipMemcpyDeviceToHost));
    if (layout != 0) {
        std::vector<std::vector<uint32_t>> got;
        HIPC(slabs.download(got));
        each_row([&](int slot, size_t elem, float* row) { slabs.get_row(got, slot, elem, row); slabs.copy_row(slabs.img, got, slot, elem); });
        slabs.strays(got, p->stray);
    } else {
        HIPC(q3_hipMemcpy(p->kcache, kv, cn * 4, hipMemcpyDeviceToHost)); HIPC(q3_hipMemcpy(p->vcache, kv + cn, cn * 4, hipMemcpyDeviceToHost));
        if (p->stray) { p->stray[0] = 0; p->stray[1] = -1; }
    }
    if (t.g_x) HIPC(q3_hipMemcpy(p->g_x, t.g_x, gx_rows * p->g_ldx * 4, hipMemcpyDeviceToHost));
    if (t.g_codes) HIPC(q3_hipMemcpy(p->g_codes, t.g_codes, (size_t)B * p->g_max_frames * 16 * 4, hipMemcpyDeviceToHost));
    if (t.zero) HIPC(q3_hipMemcpy(p->zero_buf, t.zero, zn * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// launch_kv_pages_to_bf16 between a slab of the f32 pool's geometry and one of the bf16 pool's
extern "C" q3_status q3_kv_pages_to_bf16_ex(int device, int n_layers, int nkv, int n_pages, const int* src_slots, const int* dst_slots,
                                            const float* src, uint16_t* dst, int* rot_used, long long* stray) {
    if (!src_slots || !dst_slots || !src || !dst || !stray) return set_err(Q3_INVALID_ARG, "q3_kv_pages_to_bf16_ex: null argument");
    if (n_layers < 1 || n_layers > 4 || nkv < 1 || nkv > 8 || n_pages < 1 || n_pages > KvPool::SLAB_SLOTS)
        return set_err(Q3_INVALID_ARG, "q3_kv_pages_to_bf16_ex: bad shape (n_layers 1..4, nkv 1..8, n_pages 1..%d)", KvPool::SLAB_SLOTS);
    if (!slots_ok(src_slots, n_pages, KvPool::SLAB_SLOTS) || !slots_ok(dst_slots, n_pages, KvPool::SLAB_SLOTS))
        return set_err(Q3_INVALID_ARG, "q3_kv_pages_to_bf16_ex: the slots of a list must be distinct slots of 0 .. %d", KvPool::SLAB_SLOTS - 1);
    HIPC(hipSetDevice(device));
    DevPool pool;
    TestSlabs a, b;
    a.shape(n_layers, nkv, 4); b.shape(n_layers, nkv, 2);
    HIPC(a.add_slab(pool)); HIPC(b.add_slab(pool));
    a.fill_pattern(); b.fill_pattern();
    auto each_row = [&](auto&& f) {
        for (int pg = 0; pg < n_pages; ++pg) for (int l = 0; l < n_layers; ++l) for (int v = 0; v < 2; ++v) for (int g = 0; g < nkv; ++g) for (int pp = 0; pp < KV_PAGE_POS; ++pp)
            f(pg, l, v, g, pp, (((((size_t)pg * n_layers + l) * 2 + v) * nkv + g) * KV_PAGE_POS + pp) * HEAD_DIM);
    };
    each_row([&](int pg, int l, int v, int g, int pp, size_t at) { a.put_row(a.img, src_slots[pg], a.row_elem(src_slots[pg], l, v, g, pp), src + at); });
    HIPC(a.upload()); HIPC(b.upload());
    std::vector<unsigned long long> lists((size_t)2 * n_pages);
    for (int pg = 0; pg < n_pages; ++pg) { lists[(size_t)pg] = a.page(src_slots[pg]); lists[(size_t)n_pages + pg] = b.page(dst_slots[pg]); }
    if (rot_used)
        for (int pg = 0; pg < n_pages; ++pg) for (int g = 0; g < nkv; ++g) {
            rot_used[(size_t)pg * nkv + g] = kv_rot(lists[(size_t)pg], g);
            rot_used[((size_t)n_pages + pg) * nkv + g] = kv_rot(lists[(size_t)n_pages + pg], g);
        }
    unsigned long long* dl; HIPC(pool.alloc(&dl, lists.size()));
    HIPC(q3_hipMemcpy(dl, lists.data(), lists.size() * 8, hipMemcpyHostToDevice));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_kv_pages_to_bf16(dl, dl + n_pages, n_pages, n_layers, nkv, a.geo.layer_stride(), a.geo.v_delta(), 0));
    HIPC(q3_hipDeviceSynchronize());
    std::vector<std::vector<uint32_t>> got;
    HIPC(b.download(got));
    std::vector<float> row((size_t)HEAD_DIM);
    each_row([&](int pg, int l, int v, int g, int pp, size_t at) {
        const size_t elem = b.row_elem(dst_slots[pg], l, v, g, pp);
        b.get_row(got, dst_slots[pg], elem, row.data());
        for (int dd = 0; dd < HEAD_DIM; ++dd) { uint32_t u; memcpy(&u, &row[(size_t)dd], 4); dst[at + dd] = (uint16_t)(u >> 16); }
        b.copy_row(b.img, got, dst_slots[pg], elem);
    });
    b.strays(got, stray);
    return Q3_OK;
}

// ---- the vocoder conv family, one launch at a time (tests/test_gpu_conv_ops.py) ----
// (L above 2^30 and a dilation beyond +-2^16 are refused here: the decision functions round L up to whole tiles and form
// (k - 1) * dil in int)
extern "C" int q3_conv_path(int cout, int cin, int L, int k, int dil, int phases, int packed, int has_resid, int planes, int aligned16) {
    if (L > (1 << 30) || dil > (1 << 16) || dil < -(1 << 16)) return 0;
    return conv_path_code(conv_pick(cout, cin, L, k, dil, phases, packed != 0, has_resid != 0, planes, aligned16 != 0, phases > 1));
}
extern "C" int q3_resunit_path(int C, int L, int dil, int packed, int ya_is_xa, int planes) {
    if (L > (1 << 30)) return 0;
    return conv_path_code(resunit_pick(C, L, dil, packed != 0, ya_is_xa != 0, planes));
}
extern "C" const char* q3_conv_path_name(int code) { return conv_path_name(code); }

// One launch_conv1d / launch_transconv1d_taps / launch_resunit call over host arrays. The weight packing, the transposed conv's
// per-phase rearrangement (the loader's own helper) and the snake tables are preparation; exactly one launch of the family runs.
// A launch the dispatcher refuses comes back as a status — never another kernel in its place — and leaves the host y / y2 alone.
// (resident / lds_bytes: q3_test_conv_resident below — the launch's residency cap, and the dynamic LDS it asked for)
static q3_status conv_ex_run(int device, const q3_conv_ex_args* p, int resident, int* lds_bytes) {
    if (!p || !p->x || !p->w || !p->y) return set_err(Q3_INVALID_ARG, "q3_conv_ex: null argument");
    if (p->path) *p->path = 0;
    const int kind = p->kind, cin = p->cin, cout = p->cout, L = p->L, k = p->k, dil = p->dil;
    if (kind < 0 || kind > 2) return set_err(Q3_INVALID_ARG, "q3_conv_ex: kind 0..2");
    if (cin < 1 || cin > 8192 || cout < 1 || cout > 8192 || L < 1 || L > (1 << 22) || k < 1 || k > 64 || dil < 1 || dil > 64 || p->act < 0 || p->act > 6)
        return set_err(Q3_INVALID_ARG, "q3_conv_ex: bad shape (channels 1..8192, L 1..2^22, k 1..64, dil 1..64, act 0..6)");
    const int stride = kind == 1 ? p->stride : 1;
    if (kind == 1 && (stride < 1 || stride > 16 || k % stride)) return set_err(Q3_INVALID_ARG, "q3_conv_ex: transposed conv needs 1 <= stride <= 16 and k %% stride == 0");
    const int taps = k / stride;
    if (kind == 2 && (cin != cout || k != 7 || !p->w2 || !p->mid_a || !p->mid_ib)) return set_err(Q3_INVALID_ARG, "q3_conv_ex: residual unit needs cin == cout, k == 7, w2 and the middle snake pair");
    if (!p->snake_a != !p->snake_b || !p->post_a != !p->post_ib || !p->mid_a != !p->mid_ib) return set_err(Q3_INVALID_ARG, "q3_conv_ex: half a snake pair");
    if (kind != 0 && (p->resid || p->resid_in_place || p->scale || p->act)) return set_err(Q3_INVALID_ARG, "q3_conv_ex: resid / scale / act belong to kind 0");
    if (kind != 0 && kind != 2 && p->y2_is_x) return set_err(Q3_INVALID_ARG, "q3_conv_ex: y2_is_x belongs to kind 2");
    if ((p->resid && p->resid_in_place) || (p->y2 && p->y2_is_x)) return set_err(Q3_INVALID_ARG, "q3_conv_ex: two residuals / two y2");
    const size_t out_n = (size_t)cout * L * stride, xn = (size_t)cin * L, wn = (size_t)cout * cin * k;
    if (p->y_front < 0 || p->y_front % 4 || p->y_elems < 0 || (size_t)p->y_elems < (size_t)p->y_front + out_n)
        return set_err(Q3_INVALID_ARG, "q3_conv_ex: y must hold y_front (a multiple of 4) + cout * L * stride floats");
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *x, *w, *w2 = nullptr, *b = nullptr, *b2 = nullptr, *res = nullptr, *scale = nullptr, *y, *y2 = nullptr;
    void *wpk = nullptr, *w2pk = nullptr;
    HIPC(pool.alloc(&x, xn)); HIPC(q3_hipMemcpy(x, p->x, xn * 4, hipMemcpyHostToDevice));
    HIPC(pool.alloc(&w, wn));
    if (kind == 1) {          // checkpoint layout in, the loader's rearrangement, per-phase weights up
        std::vector<float> wp(wn);
        transconv_phase_weights(p->w, cin, cout, k, stride, wp.data());
        HIPC(q3_hipMemcpy(w, wp.data(), wn * 4, hipMemcpyHostToDevice));
    } else HIPC(q3_hipMemcpy(w, p->w, wn * 4, hipMemcpyHostToDevice));
    if (kind == 2) { HIPC(pool.alloc(&w2, (size_t)cout * cin)); HIPC(q3_hipMemcpy(w2, p->w2, (size_t)cout * cin * 4, hipMemcpyHostToDevice)); }
    auto vec = [&](const float* h, int n, float** d) -> q3_status {
        *d = nullptr;
        if (!h) return Q3_OK;
        HIPC(pool.alloc(d, (size_t)n)); HIPC(q3_hipMemcpy(*d, h, (size_t)n * 4, hipMemcpyHostToDevice));
        return Q3_OK;
    };
    // a snake pair: the tables as given, or built from (alpha, beta) by the engine's own kernel
    auto pair = [&](const float* ha, const float* hb, int n, float** da, float** db) -> q3_status {
        Q3C(vec(ha, n, da)); Q3C(vec(hb, n, db));
        if (ha && p->snake_raw) {
            float *ta, *tb;
            HIPC(pool.alloc(&ta, (size_t)n)); HIPC(pool.alloc(&tb, (size_t)n));
            HIPC(launch_snake_tables(*da, *db, ta, tb, n, 0));
            *da = ta; *db = tb;
        }
        return Q3_OK;
    };
    float *sa, *sb, *pa, *pb, *ma, *mb;
    Q3C(vec(p->b, cout, &b)); Q3C(vec(p->b2, cout, &b2)); Q3C(vec(p->scale, cout, &scale)); Q3C(vec(p->resid, (int)out_n, &res));
    Q3C(pair(p->snake_a, p->snake_b, cin, &sa, &sb)); Q3C(pair(p->post_a, p->post_ib, cout, &pa, &pb)); Q3C(pair(p->mid_a, p->mid_ib, cout, &ma, &mb));
    const size_t yn = (size_t)p->y_elems;
    HIPC(pool.alloc(&y, yn)); HIPC(q3_hipMemcpy(y, p->y, yn * 4, hipMemcpyHostToDevice));
    if (p->y2) { HIPC(pool.alloc(&y2, yn)); HIPC(q3_hipMemcpy(y2, p->y2, yn * 4, hipMemcpyHostToDevice)); }
    float* yr = y + p->y_front; float* y2r = y2 ? y2 + p->y_front : nullptr;
    if (p->packed) {
        const int pk = kind == 1 ? taps : k;
        if (cout % 32 || cin % 16 || pk < 1) return set_err(Q3_UNSUPPORTED, "q3_conv_ex: cout %d / cin %d cannot be packed (cout %% 32, cin %% 16)", cout, cin);
        const size_t per = packed_conv_w_bytes(cout, cin, pk);
        char* d; HIPC(pool.alloc(&d, per * (size_t)stride)); wpk = d;
        for (int ph = 0; ph < stride; ++ph) HIPC(launch_pack_conv_w(w + (size_t)ph * cout * cin * pk, d + (size_t)ph * per, cout, cin, pk, 0));
        if (kind == 2) {
            char* d2; HIPC(pool.alloc(&d2, packed_conv_w_bytes(cout, cin, 1))); w2pk = d2;
            HIPC(launch_pack_conv_w(w2, d2, cout, cin, 1, 0));
        }
    }
    HIPC(q3_hipDeviceSynchronize());
    hipError_t e;
    int path = 0;
    if (kind == 0) {
        ConvArgs a;
        a.x = x; a.w = w; a.b = b; a.y = yr; a.cin = cin; a.cout = cout; a.L = L; a.k = k; a.dil = dil;
        a.snake_a = sa; a.snake_b = sb; a.resid = p->resid_in_place ? yr : res; a.scale = scale; a.act = p->act;
        a.post_a = pa; a.post_ib = pb; a.y2 = y2r; a.wpk = wpk; a.planes = p->planes; a.resident = resident;
        e = launch_conv1d(a, 0, &path);
    } else if (kind == 1) {
        e = launch_transconv1d_taps(x, w, b, yr, cin, cout, L, stride, taps, sa, sb, 0, pa, pb, y2r, wpk, p->planes, &path, resident);
    } else {
        ResUnitArgs r{};
        r.xa = x; r.y = yr; r.ya = p->y2_is_x ? x : y2r; r.w1pk = wpk; r.w2pk = w2pk; r.b1 = b; r.b2 = b2;
        r.mid_a = ma; r.mid_ib = mb; r.post_a = pa; r.post_ib = pb; r.C = cout; r.L = L; r.dil = dil; r.planes = p->planes; r.resident = resident;
        e = launch_resunit(r, 0, &path);
    }
    if (p->path) *p->path = path;
    if (e == hipErrorInvalidValue || e == hipErrorNotSupported) {
        (void)hipGetLastError();
        return set_err(Q3_UNSUPPORTED, "q3_conv_ex: the launcher refused kind=%d cin=%d cout=%d L=%d k=%d dil=%d stride=%d packed=%d planes=%d (%s)", kind, cin, cout,
                       L, k, dil, stride, p->packed, p->planes, hipGetErrorString(e));
    }
    HIPC(e);
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(p->y, y, yn * 4, hipMemcpyDeviceToHost));
    if (y2) HIPC(q3_hipMemcpy(p->y2, y2, yn * 4, hipMemcpyDeviceToHost));
    if (lds_bytes) *lds_bytes = (int)conv_last_dyn_lds();
    return Q3_OK;
}
extern "C" q3_status q3_conv_ex(int device, const q3_conv_ex_args* p) { return conv_ex_run(device, p, 0, nullptr); }
// q3_conv_ex under a residency cap (ConvArgs::resident; tests/test_decode_resident.py): only launches of the kernels with dynamic
// LDS (k_conv_bf16x3, k_resunit_bf16x3) take it — any other path is refused here, so a test never compares two uncapped launches.
extern "C" q3_status q3_test_conv_resident(int device, const q3_conv_ex_args* p, int resident, int* lds_bytes) {
    if (lds_bytes) *lds_bytes = 0;
    if (resident < 0 || resident > 8) return set_err(Q3_INVALID_ARG, "q3_test_conv_resident: resident 0..8");
    if (p && p->kind >= 0 && p->kind <= 2 && p->cin >= 1 && p->cout >= 1 && p->L >= 1 && p->k >= 1 && p->dil >= 1 && (p->kind != 1 || (p->stride >= 1 && p->k % p->stride == 0))) {
        const int code = p->kind == 2 ? conv_path_code(resunit_pick(p->cout, p->L, p->dil, p->packed != 0 && p->w2 && p->mid_a, p->y2_is_x != 0, p->planes))
                       : p->kind == 1 ? conv_path_code(conv_pick(p->cout, p->cin, p->L, p->k / p->stride, 1, p->stride, p->packed != 0, false, p->planes, false, true))
                                      : conv_path_code(conv_pick(p->cout, p->cin, p->L, p->k, p->dil, 1, p->packed != 0, p->resid || p->resid_in_place, p->planes, false, false));
        const int kern = code & CP_KERNEL_MASK;
        if (!((kern >= CK_BF16X3_96x128_TM4 && kern <= CK_BF16X3_96x128_6W) || kern == CK_RESUNIT_3W || kern == CK_RESUNIT_6W)) {
            if (p->path) *p->path = code;
            return set_err(Q3_UNSUPPORTED, "q3_test_conv_resident: %s has no dynamic LDS to cap", conv_path_name(code));
        }
    }
    return conv_ex_run(device, p, resident, lds_bytes);
}

static q3_status check_cl_out(const char* who, const void* x, const void* w, const void* y, int C, int L, int y_front, int y_elems) {
    if (!x || !w || !y) return set_err(Q3_INVALID_ARG, "%s: null argument", who);
    if (C < 1 || C > 8192 || L < 1 || L > (1 << 22)) return set_err(Q3_INVALID_ARG, "%s: bad shape (C 1..8192, L 1..2^22)", who);
    if (y_front < 0 || y_elems < 0 || (size_t)y_elems < (size_t)y_front + (size_t)C * L) return set_err(Q3_INVALID_ARG, "%s: y must hold y_front + C * L floats", who);
    return Q3_OK;
}

extern "C" q3_status q3_norm_c(int device, int layernorm, const float* x_host, const float* w_host, const float* b_host, int C, int L, float eps,
                               float* y_host, int y_front, int y_elems) {
    Q3C(check_cl_out("q3_norm_c", x_host, w_host, y_host, C, L, y_front, y_elems));
    if (layernorm && !b_host) return set_err(Q3_INVALID_ARG, "q3_norm_c: LayerNorm needs a bias");
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *x, *w, *b = nullptr, *y;
    const size_t n = (size_t)C * L;
    HIPC(pool.alloc(&x, n)); HIPC(pool.alloc(&w, (size_t)C)); HIPC(pool.alloc(&y, (size_t)y_elems));
    HIPC(q3_hipMemcpy(x, x_host, n * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(w, w_host, (size_t)C * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(y, y_host, (size_t)y_elems * 4, hipMemcpyHostToDevice));
    if (layernorm) { HIPC(pool.alloc(&b, (size_t)C)); HIPC(q3_hipMemcpy(b, b_host, (size_t)C * 4, hipMemcpyHostToDevice)); }
    HIPC(q3_hipDeviceSynchronize());
    if (layernorm) HIPC(launch_layernorm_c(x, w, b, y + y_front, C, L, eps, 0));
    else HIPC(launch_rmsnorm_c(x, w, y + y_front, C, L, eps, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(y_host, y, (size_t)y_elems * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_dwconv7(int device, const float* x_host, const float* w_host, const float* b_host, int C, int L, float* y_host, int y_front,
                                int y_elems) {
    Q3C(check_cl_out("q3_dwconv7", x_host, w_host, y_host, C, L, y_front, y_elems));
    if (!b_host) return set_err(Q3_INVALID_ARG, "q3_dwconv7: null argument");
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *x, *w, *b, *y;
    const size_t n = (size_t)C * L;
    HIPC(pool.alloc(&x, n)); HIPC(pool.alloc(&w, (size_t)C * 7)); HIPC(pool.alloc(&b, (size_t)C)); HIPC(pool.alloc(&y, (size_t)y_elems));
    HIPC(q3_hipMemcpy(x, x_host, n * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(w, w_host, (size_t)C * 7 * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(b, b_host, (size_t)C * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(y, y_host, (size_t)y_elems * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_dwconv7(x, w, b, y + y_front, C, L, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(y_host, y, (size_t)y_elems * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// ---- the long-prompt prefill kernels, one launch at a time (tests/test_gpu_prefill_ops.py) ----
static hipError_t fill_ff(void* dev, size_t bytes) {                 // 0xFF bytes: bf16 / f32 NaN wherever a kernel reads what nobody wrote
    std::vector<unsigned char> h(bytes, 0xFF);
    return q3_hipMemcpy(dev, h.data(), bytes, hipMemcpyHostToDevice);
}
static void gemm_path_out(const GemmPick& p, int* path) {
    if (!path) return;
    path[0] = p.geometry; path[1] = p.geometry == GEMM_G3 ? p.k_ranges : 1; path[2] = p.geometry == GEMM_G3 ? p.k_split : 1;
    path[3] = p.geometry == GEMM_G2 ? p.n_split : 1;
}
// the split-K workspace the entry passes — every range sum of the shape — when the stage count lets k_split != 1 be picked at all
static size_t gemm_ex_ws_bytes(int M, int N, int Kpad, int epi) {
    if (Kpad % 128 || (Kpad >> 6) % 16) return 0;
    return (size_t)8 * (epi == EPI_SWIGLU ? 2 : 1) * M * N * sizeof(float);
}

extern "C" int q3_gemm_path(int M, int N, int K, int epi, int norm, int w2, int planes, int* path) {
    if (path) path[0] = path[1] = path[2] = path[3] = 0;
    if (M < 1 || N < 1 || K < 4 || M > (1 << 24) || N > (1 << 24) || K > (1 << 24)) return -1;      // (beyond 2^24 the paddings leave int)
    // nothing is dereferenced by the pick: the pointers only say what the caller has
    static float dummy[4];
    GemmArgs g;
    g.W = reinterpret_cast<const uint16_t*>(dummy); g.W2 = w2 ? g.W : nullptr; g.x = dummy; g.ldx = up32(K); g.y = dummy; g.ldy = N;
    g.norm_w = norm ? dummy : nullptr; g.den = norm ? dummy : nullptr;
    g.M = M; g.N = N; g.K = K; g.Kpad = up32(K); g.epi = epi;
    if (planes) { g.xp = g.W; g.xp_plane = (size_t)up128(M) * g.Kpad; g.splitk_ws_bytes = gemm_ex_ws_bytes(M, N, g.Kpad, epi); g.splitk_ws = g.splitk_ws_bytes ? dummy : nullptr; }
    if (g.K % 4 || g.N % 64 || (planes && K % 8)) return -1;
    const bool rms = norm != 0;
    if (epi < EPI_NONE || epi > EPI_SWIGLU || ((epi == EPI_RESID || epi == EPI_SILU) && rms) || (epi == EPI_SWIGLU && (!rms || !w2))) return -1;
    const GemmPick p = lm_gemm_pick(g);
    gemm_path_out(p, path);
    return p.geometry;
}

// One launch_lm_gemm call over host arrays: the weights go through the loader's retile_bf16, a norm through launch_row_den, the
// planes through launch_split_rows into a NaN-filled buffer of whole 128-row tiles; exactly one GEMM launch (+ its split-K reduce)
// runs. A launch the dispatcher refuses comes back as a status — never another geometry in its place — and leaves the host y alone.
extern "C" q3_status q3_gemm_ex(int device, const q3_gemm_ex_args* p) {
    if (!p || !p->x || !p->w || !p->y) return set_err(Q3_INVALID_ARG, "q3_gemm_ex: null argument");
    if (p->path) p->path[0] = p->path[1] = p->path[2] = p->path[3] = 0;
    const int M = p->M, N = p->N, K = p->K;
    if (M < 1 || M > 8192 || N < 1 || N > 16384 || K < 4 || K > 16384) return set_err(Q3_INVALID_ARG, "q3_gemm_ex: bad shape (M 1..8192, N 1..16384, K 4..16384)");
    if (p->ldx < K || p->ldy < N || p->M_alloc < M) return set_err(Q3_INVALID_ARG, "q3_gemm_ex: bad pitch (ldx >= K, ldy >= N, M_alloc >= M)");
    if (p->epi < EPI_NONE || p->epi > EPI_SWIGLU || p->geometry < -1 || p->geometry > GEMM_G3 || p->k_split < 0 || p->sup_m < 0 || p->sup_n < 0 || !p->sup_m != !p->sup_n)
        return set_err(Q3_INVALID_ARG, "q3_gemm_ex: epi 0..3, geometry -1..3, k_split / sup_m / sup_n >= 0 (the super-tile as a pair)");
    if (p->epi == EPI_RESID && (!p->resid || p->ldr < N)) return set_err(Q3_INVALID_ARG, "q3_gemm_ex: residual epilogue needs resid with ldr >= N");
    const bool planes = p->geometry != GEMM_G1_SPLIT;
    // what no kernel of the family can address (vector loads and stores of 4 floats, 8 k per plane store) is refused here: the
    // launchers say the same, but the preparation launches would run first
    if (K % 4 || p->ldx % 4 || p->ldy % 4 || N % 64 || (p->resid && p->ldr % 4)) return set_err(Q3_UNSUPPORTED, "q3_gemm_ex: K, ldx, ldy, ldr multiples of 4 and N of 64");
    if (planes && K % 8) return set_err(Q3_UNSUPPORTED, "q3_gemm_ex: pre-split planes need K %% 8 == 0 (K = %d)", K);
    HIPC(hipSetDevice(device));
    DevPool pool;
    const int nmat = p->w2 ? 2 : 1, Kpad = up32(K);
    const size_t welems = tiled_elems(1, N, K);
    uint16_t* w; float *x, *y, *b = nullptr, *nw = nullptr, *den = nullptr, *res = nullptr, *ws = nullptr; uint16_t* xp = nullptr;
    HIPC(pool.alloc(&w, welems * nmat));
    for (int i = 0; i < nmat; ++i) {
        std::vector<uint16_t> wt(welems);
        retile_bf16(i ? p->w2 : p->w, N, K, wt.data(), 1);
        HIPC(q3_hipMemcpy(w + (size_t)i * welems, wt.data(), welems * 2, hipMemcpyHostToDevice));
    }
    const size_t xn = (size_t)M * p->ldx, yn = (size_t)p->M_alloc * p->ldy;
    HIPC(pool.alloc(&x, xn)); HIPC(q3_hipMemcpy(x, p->x, xn * 4, hipMemcpyHostToDevice));
    HIPC(pool.alloc(&y, yn)); HIPC(q3_hipMemcpy(y, p->y, yn * 4, hipMemcpyHostToDevice));
    if (p->bias) { HIPC(pool.alloc(&b, (size_t)N)); HIPC(q3_hipMemcpy(b, p->bias, (size_t)N * 4, hipMemcpyHostToDevice)); }
    if (p->norm_w) { HIPC(pool.alloc(&nw, (size_t)K)); HIPC(q3_hipMemcpy(nw, p->norm_w, (size_t)K * 4, hipMemcpyHostToDevice)); HIPC(pool.alloc(&den, (size_t)M)); }
    if (p->epi == EPI_RESID) { HIPC(pool.alloc(&res, (size_t)M * p->ldr)); HIPC(q3_hipMemcpy(res, p->resid, (size_t)M * p->ldr * 4, hipMemcpyHostToDevice)); }
    const size_t plane_elems = (size_t)up128(M) * Kpad;              // whole 128-row tiles (GemmArgs::xp)
    size_t ws_bytes = 0;
    if (planes) {
        HIPC(pool.alloc(&xp, plane_elems * 3)); HIPC(fill_ff(xp, plane_elems * 3 * 2));
        ws_bytes = gemm_ex_ws_bytes(M, N, Kpad, p->epi);
        if (ws_bytes) { HIPC(pool.alloc(&ws, ws_bytes / 4)); HIPC(fill_ff(ws, ws_bytes)); }
    }
    GemmArgs g;
    g.W = w; g.W2 = nmat == 2 ? w + welems : nullptr; g.x = x; g.ldx = p->ldx; g.norm_w = nw; g.den = den; g.bias = b;
    g.resid = res; g.ldr = res ? p->ldr : 0; g.y = y; g.ldy = p->ldy; g.M = M; g.N = N; g.K = K; g.Kpad = Kpad; g.epi = p->epi;
    g.xp = xp; g.xp_plane = xp ? plane_elems : 0; g.splitk_ws = ws; g.splitk_ws_bytes = ws_bytes;
    GemmPick pick = lm_gemm_pick(g, p->geometry);
    if (p->k_split) pick.k_split = p->k_split;
    if (p->sup_m) { pick.sup_m = p->sup_m; pick.sup_n = p->sup_n; }
    HIPC(q3_hipDeviceSynchronize());
    if (nw) HIPC(launch_row_den(x, p->ldx, den, M, K, p->eps, 0));
    if (xp) HIPC(launch_split_rows(x, p->ldx, nw, xp, plane_elems, M, K, Kpad, 0));
    const hipError_t e = launch_lm_gemm(g, pick, 0);
    if (e == hipErrorInvalidValue || e == hipErrorNotSupported) {
        (void)hipGetLastError();
        (void)q3_hipDeviceSynchronize();
        return set_err(Q3_UNSUPPORTED, "q3_gemm_ex: launch_lm_gemm refused M=%d N=%d K=%d epi=%d norm=%d geometry=%d k_ranges=%d k_split=%d sup=%dx%d (%s)", M, N, K,
                       p->epi, nw ? 1 : 0, pick.geometry, pick.k_ranges, pick.k_split, pick.sup_m, pick.sup_n, hipGetErrorString(e));
    }
    HIPC(e);
    HIPC(q3_hipDeviceSynchronize());
    gemm_path_out(pick, p->path);
    HIPC(q3_hipMemcpy(p->y, y, yn * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" int q3_attn_prefill_path(int nh, int nkv, int use_planes, int halves, int* path) {
    if (path) path[0] = path[1] = 0;
    if (nkv < 1 || nh < nkv || nh % nkv || halves < 1 || halves > 2) return -1;
    static float dummy[4];
    AttnArgs t{};
    t.nh = nh; t.nkv = nkv; t.n_splits = halves; t.part = halves == 2 ? dummy : nullptr; t.kvp = use_planes ? reinterpret_cast<const unsigned char*>(dummy) : nullptr;
    const AttnPrefillPick p = attn_prefill_pick(t);
    if (p.kernel == AP_VALU && nh / nkv > 2) return -1;              // what the launch refuses
    if (path) { path[0] = p.kernel; path[1] = p.halves; }
    return p.kernel;
}

// One prefill attention step: launch_qknorm_rope_kv (rows_per_seq = rps), launch_kv_planes for the bf16x3 kernel (into a NaN-filled
// buffer with more tiles allocated than used), ONE launch_attn_prefill, launch_attn_merge for two halves (over NaN-filled records).
// layout 0: one contiguous cache. layout 1: the logical cache rows of `layer` scattered over pattern-filled slabs of KvPool's
// geometry (TestSlabs, as q3_attn_step_ex), gathered back afterwards; pages of a cached prefix may be shared between sequences.
// Everything is validated before a device is touched. A refused launch comes back as a status and leaves the host caches and out alone.
extern "C" q3_status q3_attn_prefill_ex(int device, const q3_attn_prefill_ex_args* p) {
    if (!p || !p->qkv || !p->q_norm_w || !p->k_norm_w || !p->rope_cos || !p->rope_sin || !p->kcache || !p->vcache || !p->out)
        return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: null argument");
    if (p->path) p->path[0] = p->path[1] = 0;
    const int n_seq = p->n_seq, rps = p->rps, nh = p->nh, nkv = p->nkv, base = p->base_pos, layout = p->layout, max_seq = p->max_seq;
    if (p->kernel < -1 || p->kernel > AP_X3 || p->halves < 1 || p->halves > 2) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: kernel -1..3, halves 1..2");
    if (n_seq < 1 || n_seq > 64 || rps < 1 || rps > 8192 || nkv < 1 || nh < nkv || nh > 64 || nh % nkv || max_seq < 1 || max_seq > (1 << 20) || base < 0 || base > max_seq - rps)
        return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: bad shape (the chunk [base_pos, base_pos + rps) must lie inside max_seq <= 2^20)");
    const int ld_qkv = p->ld_qkv, QD = nh * HEAD_DIM, rows = n_seq * rps;
    if (ld_qkv < (nh + 2 * nkv) * HEAD_DIM || ld_qkv % 4 || p->ld_out < QD || p->ld_out % 4) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: bad pitch");
    if (layout < 0 || layout > 2) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: layout 0..2");
    if (layout == 2) return set_err(Q3_UNSUPPORTED, "q3_attn_prefill_ex: prefill never runs on bf16 pages");
    const int n_pg = (max_seq + KV_PAGE_POS - 1) / KV_PAGE_POS;
    auto cache_row = [&](float* c, int s, int g, int pp) { return c + (((size_t)s * nkv + g) * max_seq + pp) * HEAD_DIM; };
    TestSlabs slabs;
    if (layout == 1) {
        if (max_seq > KV_MAX_PAGES * KV_PAGE_POS) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: a paged row holds at most %d positions", KV_MAX_PAGES * KV_PAGE_POS);
        if (p->n_layers < 1 || p->n_layers > 4 || p->layer < 0 || p->layer >= p->n_layers || p->n_slabs < 1 || p->n_slabs > 2)
            return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: n_layers 1..4, layer inside them, n_slabs 1..2");
        if (!p->page_slots || !p->stray) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: a paged layout needs page_slots and stray");
        slabs.shape(p->n_layers, nkv, 4);
        if (slabs.geo.v_delta() > 0x7fffffffu) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: K -> V distance beyond the kernels' 32-bit form");
        // a slot serves one page — or page i of several sequences where that page is a wholly cached prefix page holding the same bits
        const int limit = KvPool::SLAB_SLOTS * p->n_slabs;
        std::vector<int> owner((size_t)limit, -1);          // the first (sequence * n_pg + page) that named the slot
        for (int s = 0; s < n_seq; ++s)
            for (int i = 0; i < n_pg; ++i) {
                const int slot = p->page_slots[(size_t)s * n_pg + i];
                if (slot < 0 || slot >= limit) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: page_slots[%d][%d] = %d outside 0 .. %d", s, i, slot, limit - 1);
                int& own = owner[(size_t)slot];
                if (own < 0) { own = s * n_pg + i; continue; }
                const int s0 = own / n_pg, i0 = own % n_pg;
                if (s0 == s || i0 != i || (i + 1) * KV_PAGE_POS > base)
                    return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: slot %d is named for page %d of sequence %d and page %d of sequence %d: only a whole page "
                                   "below base_pos (%d) may be shared, as the same page of different sequences", slot, i0, s0, i, s, base);
                const int p0 = i * KV_PAGE_POS;             // (a shared page lies below base_pos <= max_seq: all 128 rows exist)
                for (int g = 0; g < nkv; ++g)
                    if (memcmp(cache_row(p->kcache, s, g, p0), cache_row(p->kcache, s0, g, p0), (size_t)KV_PAGE_POS * HEAD_DIM * 4) != 0 ||
                        memcmp(cache_row(p->vcache, s, g, p0), cache_row(p->vcache, s0, g, p0), (size_t)KV_PAGE_POS * HEAD_DIM * 4) != 0)
                        return set_err(Q3_INVALID_ARG, "q3_attn_prefill_ex: sequences %d and %d share slot %d but their cache rows of page %d differ", s0, s, slot, i);
            }
    }
    HIPC(hipSetDevice(device));
    DevPool pool;
    const size_t cn = (size_t)n_seq * nkv * max_seq * HEAD_DIM, rn = (size_t)max_seq * 64, on = (size_t)rows * p->ld_out;
    float *qkv, *qw, *kw, *rc, *rs, *kv = nullptr, *qbuf, *part = nullptr, *out; unsigned char* kvp = nullptr;
    unsigned long long* table = nullptr;
    // (slab, table, slab: with two slabs the pages of a row lie on both sides of the table the kernels form their addresses from)
    if (layout == 1) {
        for (int s = 0; s < p->n_slabs; ++s) {
            if (s == 1) HIPC(pool.alloc(&table, (size_t)n_seq * KV_MAX_PAGES));
            HIPC(slabs.add_slab(pool));
        }
        if (!table) HIPC(pool.alloc(&table, (size_t)n_seq * KV_MAX_PAGES));
    } else HIPC(pool.alloc(&kv, 2 * cn));
    HIPC(pool.alloc(&qkv, (size_t)rows * ld_qkv)); HIPC(pool.alloc(&qw, (size_t)HEAD_DIM)); HIPC(pool.alloc(&kw, (size_t)HEAD_DIM));
    HIPC(pool.alloc(&rc, rn)); HIPC(pool.alloc(&rs, rn));
    HIPC(pool.alloc(&qbuf, (size_t)rows * QD)); HIPC(pool.alloc(&out, on));
    HIPC(q3_hipMemcpy(qkv, p->qkv, (size_t)rows * ld_qkv * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(qw, p->q_norm_w, HEAD_DIM * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(kw, p->k_norm_w, HEAD_DIM * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(rc, p->rope_cos, rn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(rs, p->rope_sin, rn * 4, hipMemcpyHostToDevice));
    auto each_row = [&](auto&& f) {             // every (sequence, kv head, position, K | V) of the logical cache with its slot and element offset
        for (int s = 0; s < n_seq; ++s) for (int g = 0; g < nkv; ++g) for (int pp = 0; pp < max_seq; ++pp) for (int v = 0; v < 2; ++v) {
            const int slot = p->page_slots[(size_t)s * n_pg + pp / KV_PAGE_POS];
            f(slot, slabs.row_elem(slot, p->layer, v, g, pp), cache_row(v ? p->vcache : p->kcache, s, g, pp));
        }
    };
    if (layout == 1) {
        slabs.fill_pattern();
        each_row([&](int slot, size_t elem, float* row) { slabs.put_row(slabs.img, slot, elem, row); });
        HIPC(slabs.upload());
        std::vector<unsigned long long> tab((size_t)n_seq * KV_MAX_PAGES);
        for (int s = 0; s < n_seq; ++s)
            for (int i = 0; i < KV_MAX_PAGES; ++i) tab[(size_t)s * KV_MAX_PAGES + i] = slabs.page(p->page_slots[(size_t)s * n_pg + (i < n_pg ? i : 0)]);      // beyond the row's pages: its first, as a session leaves them
        HIPC(q3_hipMemcpy(table, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
        if (p->rot_used)
            for (int s = 0; s < n_seq; ++s) for (int i = 0; i < n_pg; ++i) for (int g = 0; g < nkv; ++g)
                p->rot_used[((size_t)s * n_pg + i) * nkv + g] = kv_rot(slabs.page(p->page_slots[(size_t)s * n_pg + i]), g);
    } else {
        HIPC(q3_hipMemcpy(kv, p->kcache, cn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(kv + cn, p->vcache, cn * 4, hipMemcpyHostToDevice));
    }
    HIPC(q3_hipMemcpy(out, p->out, on * 4, hipMemcpyHostToDevice));
    AttnArgs t{};
    t.qkv = qkv; t.ld_qkv = ld_qkv; t.q_norm_w = qw; t.k_norm_w = kw; t.eps = p->eps; t.rope_cos = rc; t.rope_sin = rs;
    t.pos_dev = nullptr; t.pos_static = base; t.max_seq = max_seq; t.qbuf = qbuf; t.out = out; t.ld_out = p->ld_out;
    if (layout == 1) { t.kv_pages = table; t.kv_layer_off = (size_t)p->layer * slabs.geo.layer_stride(); t.kv_vdelta = slabs.geo.v_delta(); }
    else { t.kcache = kv; t.vcache = kv + cn; }
    t.B = rows; t.nh = nh; t.nkv = nkv; t.n_splits = 1; t.rows_per_seq = rps;
    const int tiles = (base + rps + 31) / 32, kvp_tiles = tiles + 2;
    const bool want_planes = p->kernel == AP_X3 || (p->kernel < 0 && p->use_planes);
    if (want_planes) {
        const size_t kb = (size_t)n_seq * nkv * kvp_tiles * KVP_TILE_BYTES;
        HIPC(pool.alloc(&kvp, kb)); HIPC(fill_ff(kvp, kb));
    }
    if (p->halves == 2) {
        const size_t pn = (size_t)rows * nh * 2 * PART_STRIDE;
        HIPC(pool.alloc(&part, pn)); HIPC(fill_ff(part, pn * 4));
    }
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_qknorm_rope_kv(t, 0));
    if (kvp) { HIPC(launch_kv_planes(t, n_seq * nkv, base + rps, kvp_tiles, kvp, 0)); t.kvp = kvp; t.kvp_tiles = kvp_tiles; }
    if (p->halves == 2) { t.part = part; t.n_splits = 2; }
    AttnPrefillPick pick = attn_prefill_pick(t);
    if (p->kernel >= 0) { pick.kernel = p->kernel; pick.halves = p->halves; }
    hipError_t e = pick.halves == p->halves ? launch_attn_prefill(t, pick, 0) : hipErrorInvalidValue;      // the engine's pick has no key halves here
    if (e == hipErrorInvalidValue || e == hipErrorNotSupported) {
        (void)hipGetLastError();
        (void)q3_hipDeviceSynchronize();
        return set_err(Q3_UNSUPPORTED, "q3_attn_prefill_ex: launch_attn_prefill refused kernel=%d halves=%d nh=%d nkv=%d rps=%d base_pos=%d (%s)", pick.kernel,
                       p->halves, nh, nkv, rps, base, hipGetErrorString(e));
    }
    HIPC(e);
    if (pick.halves == 2) HIPC(launch_attn_merge(t, 0));
    HIPC(q3_hipDeviceSynchronize());
    if (p->path) { p->path[0] = pick.kernel; p->path[1] = pick.halves; }
    HIPC(q3_hipMemcpy(p->out, out, on * 4, hipMemcpyDeviceToHost));
    if (layout == 1) {
        std::vector<std::vector<uint32_t>> got;
        HIPC(slabs.download(got));
        each_row([&](int slot, size_t elem, float* row) { slabs.get_row(got, slot, elem, row); slabs.copy_row(slabs.img, got, slot, elem); });
        slabs.strays(got, p->stray);
    } else {
        HIPC(q3_hipMemcpy(p->kcache, kv, cn * 4, hipMemcpyDeviceToHost)); HIPC(q3_hipMemcpy(p->vcache, kv + cn, cn * 4, hipMemcpyDeviceToHost));
        if (p->stray) { p->stray[0] = 0; p->stray[1] = -1; }
    }
    return Q3_OK;
}

// The packed sibling: sequences of seq_len[i] rows, all from position 0, end to end in qkv / out. The packed q/k-norm
// launch, the packed plane split where a sequence takes the bf16x3 kernel, one packed attention launch per kernel present.
extern "C" q3_status q3_attn_prefill_packed_ex(int device, const q3_attn_prefill_packed_ex_args* p) {
    if (!p || !p->seq_len || !p->qkv || !p->q_norm_w || !p->k_norm_w || !p->rope_cos || !p->rope_sin || !p->kcache || !p->vcache || !p->out)
        return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: null argument");
    if (p->path) p->path[0] = p->path[1] = 0;
    if (p->plane_tail) p->plane_tail[0] = p->plane_tail[1] = 0;
    const int n_seq = p->n_seq, nh = p->nh, nkv = p->nkv, layout = p->layout, max_seq = p->max_seq;
    if (p->kernel != -1 && p->kernel != AP_T && p->kernel != AP_X3) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: kernel -1, 2 or 3");
    if (n_seq < 1 || n_seq > 64 || nkv < 1 || nh < nkv || nh > 64 || nh % nkv || max_seq < 1 || max_seq > 8192)
        return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: bad shape");
    const int nrep = nh / nkv;
    if (nrep != 1 && nrep != 2 && nrep != 4) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: heads / kv heads 1, 2 or 4");
    int rows = 0;
    std::vector<int> trow((size_t)n_seq), kern((size_t)n_seq);
    for (int s = 0; s < n_seq; ++s) {
        const int L = p->seq_len[s];
        if (L < 1 || L > max_seq) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: seq_len[%d] = %d outside 1 .. max_seq (%d)", s, L, max_seq);
        rows += L; trow[(size_t)s] = s; kern[(size_t)s] = p->kernel >= 0 ? p->kernel : (L >= 256 ? AP_X3 : AP_T);
    }
    if (rows > 16384) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: %d rows (at most 16384)", rows);
    const int ld_qkv = p->ld_qkv, QD = nh * HEAD_DIM;
    if (ld_qkv < (nh + 2 * nkv) * HEAD_DIM || ld_qkv % 4 || p->ld_out < QD || p->ld_out % 4) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: bad pitch");
    if (layout < 0 || layout > 1) return set_err(layout == 2 ? Q3_UNSUPPORTED : Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: layout 0 or 1 (prefill never runs on bf16 pages)");
    const int n_pg = (max_seq + KV_PAGE_POS - 1) / KV_PAGE_POS;
    auto cache_row = [&](float* c, int s, int g, int pp) { return c + (((size_t)s * nkv + g) * max_seq + pp) * HEAD_DIM; };
    TestSlabs slabs;
    if (layout == 1) {
        if (p->n_layers < 1 || p->n_layers > 4 || p->layer < 0 || p->layer >= p->n_layers || p->n_slabs < 1 || p->n_slabs > 2)
            return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: n_layers 1..4, layer inside them, n_slabs 1..2");
        if (!p->page_slots || !p->stray) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: a paged layout needs page_slots and stray");
        slabs.shape(p->n_layers, nkv, 4);
        if (slabs.geo.v_delta() > 0x7fffffffu) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: K -> V distance beyond the kernels' 32-bit form");
        const int limit = KvPool::SLAB_SLOTS * p->n_slabs;
        std::vector<char> taken((size_t)limit, 0);
        for (int s = 0; s < n_seq; ++s)
            for (int i = 0; i < n_pg; ++i) {
                const int slot = p->page_slots[(size_t)s * n_pg + i];
                if (slot < 0 || slot >= limit) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: page_slots[%d][%d] = %d outside 0 .. %d", s, i, slot, limit - 1);
                if (taken[(size_t)slot]) return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: slot %d is named twice (every sequence starts at 0: no shared page)", slot);
                taken[(size_t)slot] = 1;
            }
    }
    PackHost ph;
    if (!pack_host_build(p->seq_len, trow.data(), kern.data(), n_seq, nh, nkv, &ph) || ph.rows != rows)
        return set_err(Q3_INVALID_ARG, "q3_attn_prefill_packed_ex: the pack's tables refused the shape");
    HIPC(hipSetDevice(device));
    DevPool pool;
    const size_t cn = (size_t)n_seq * nkv * max_seq * HEAD_DIM, rn = (size_t)max_seq * 64, on = (size_t)rows * p->ld_out;
    float *qkv, *qw, *kw, *rc, *rs, *kv = nullptr, *qbuf, *out; unsigned char* kvp = nullptr; int* tabs = nullptr;
    unsigned long long* table = nullptr;
    if (layout == 1) {
        for (int s = 0; s < p->n_slabs; ++s) {
            if (s == 1) HIPC(pool.alloc(&table, (size_t)n_seq * KV_MAX_PAGES));
            HIPC(slabs.add_slab(pool));
        }
        if (!table) HIPC(pool.alloc(&table, (size_t)n_seq * KV_MAX_PAGES));
    } else HIPC(pool.alloc(&kv, 2 * cn));
    HIPC(pool.alloc(&qkv, (size_t)rows * ld_qkv)); HIPC(pool.alloc(&qw, (size_t)HEAD_DIM)); HIPC(pool.alloc(&kw, (size_t)HEAD_DIM));
    HIPC(pool.alloc(&rc, rn)); HIPC(pool.alloc(&rs, rn));
    HIPC(pool.alloc(&qbuf, (size_t)rows * QD)); HIPC(pool.alloc(&out, on)); HIPC(pool.alloc(&tabs, ph.blob.size()));
    HIPC(q3_hipMemcpy(qkv, p->qkv, (size_t)rows * ld_qkv * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(qw, p->q_norm_w, HEAD_DIM * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(kw, p->k_norm_w, HEAD_DIM * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(rc, p->rope_cos, rn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(rs, p->rope_sin, rn * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(tabs, ph.blob.data(), ph.blob.size() * 4, hipMemcpyHostToDevice));
    auto each_row = [&](auto&& f) {
        for (int s = 0; s < n_seq; ++s) for (int g = 0; g < nkv; ++g) for (int pp = 0; pp < max_seq; ++pp) for (int v = 0; v < 2; ++v) {
            const int slot = p->page_slots[(size_t)s * n_pg + pp / KV_PAGE_POS];
            f(slot, slabs.row_elem(slot, p->layer, v, g, pp), cache_row(v ? p->vcache : p->kcache, s, g, pp));
        }
    };
    if (layout == 1) {
        slabs.fill_pattern();
        each_row([&](int slot, size_t elem, float* row) { slabs.put_row(slabs.img, slot, elem, row); });
        HIPC(slabs.upload());
        std::vector<unsigned long long> tab((size_t)n_seq * KV_MAX_PAGES);
        for (int s = 0; s < n_seq; ++s)
            for (int i = 0; i < KV_MAX_PAGES; ++i) tab[(size_t)s * KV_MAX_PAGES + i] = slabs.page(p->page_slots[(size_t)s * n_pg + (i < n_pg ? i : 0)]);
        HIPC(q3_hipMemcpy(table, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
        if (p->rot_used)
            for (int s = 0; s < n_seq; ++s) for (int i = 0; i < n_pg; ++i) for (int g = 0; g < nkv; ++g)
                p->rot_used[((size_t)s * n_pg + i) * nkv + g] = kv_rot(slabs.page(p->page_slots[(size_t)s * n_pg + i]), g);
    } else {
        HIPC(q3_hipMemcpy(kv, p->kcache, cn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(kv + cn, p->vcache, cn * 4, hipMemcpyHostToDevice));
    }
    HIPC(q3_hipMemcpy(out, p->out, on * 4, hipMemcpyHostToDevice));
    AttnArgs t{};
    t.qkv = qkv; t.ld_qkv = ld_qkv; t.q_norm_w = qw; t.k_norm_w = kw; t.eps = p->eps; t.rope_cos = rc; t.rope_sin = rs;
    t.pos_dev = nullptr; t.pos_static = 0; t.max_seq = max_seq; t.qbuf = qbuf; t.out = out; t.ld_out = p->ld_out;
    if (layout == 1) { t.kv_pages = table; t.kv_layer_off = (size_t)p->layer * slabs.geo.layer_stride(); t.kv_vdelta = slabs.geo.v_delta(); }
    else { t.kcache = kv; t.vcache = kv + cn; }
    t.B = rows; t.nh = nh; t.nkv = nkv; t.n_splits = 1; t.rows_per_seq = rows;
    const PackTab pt = ph.tab(tabs);
    const size_t kb_used = (size_t)ph.plane_tiles * KVP_TILE_BYTES, kb = kb_used + 2 * KVP_TILE_BYTES;
    if (ph.n_plane_items > 0) { HIPC(pool.alloc(&kvp, kb)); HIPC(fill_ff(kvp, kb)); }
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_qknorm_rope_kv_pack(t, pt, 0));
    if (kvp) { HIPC(launch_kv_planes_pack(t, pt, kvp, 0)); t.kvp = kvp; t.kvp_tiles = ph.plane_tiles; }
    HIPC(launch_attn_prefill_pack(t, pt, AP_T, 0));
    HIPC(launch_attn_prefill_pack(t, pt, AP_X3, 0));
    HIPC(q3_hipDeviceSynchronize());
    if (p->path) { p->path[0] = ph.per_xcd[0] > 0 ? 1 : 0; p->path[1] = ph.per_xcd[1] > 0 ? 1 : 0; }
    if (kvp && p->plane_tail) {
        std::vector<unsigned char> tail(2 * KVP_TILE_BYTES);
        HIPC(q3_hipMemcpy(tail.data(), kvp + kb_used, tail.size(), hipMemcpyDeviceToHost));
        long long still = 0;
        for (unsigned char c : tail) still += c == 0xff;
        p->plane_tail[0] = still; p->plane_tail[1] = (long long)tail.size();
    }
    HIPC(q3_hipMemcpy(p->out, out, on * 4, hipMemcpyDeviceToHost));
    if (layout == 1) {
        std::vector<std::vector<uint32_t>> got;
        HIPC(slabs.download(got));
        each_row([&](int slot, size_t elem, float* row) { slabs.get_row(got, slot, elem, row); slabs.copy_row(slabs.img, got, slot, elem); });
        slabs.strays(got, p->stray);
    } else {
        HIPC(q3_hipMemcpy(p->kcache, kv, cn * 4, hipMemcpyDeviceToHost)); HIPC(q3_hipMemcpy(p->vcache, kv + cn, cn * 4, hipMemcpyDeviceToHost));
        if (p->stray) { p->stray[0] = 0; p->stray[1] = -1; }
    }
    return Q3_OK;
}

// ---- the kernels that build the prompt rows, one launch at a time (tests/test_gpu_prompt_rows.py) ----
// Exactly one launch_* per call. A destination goes up whole, 64 guard elements on both sides, and comes back whole; whatever the
// kernel would read or write outside its arrays is refused here, before a device is touched.
extern "C" q3_status q3_prompt_rows_ex(int device, const q3_prompt_rows_ex_args* p) {
    constexpr int G = 64;
    if (!p) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: null argument");
    const int mode = p->mode, n = p->n, cols = p->cols;
    if (mode < 0 || mode > 4) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: mode 0..4");
    if (n < 1 || n > 65535) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: n 1..65535");
    if (mode != 4 && (cols < 1 || cols > 65536 || !p->out)) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: cols 1..65536 and a destination");
    auto table_ok = [](int rows) { return rows >= 1 && rows <= (1 << 20); };
    size_t payload = 0;
    if (mode == 0) {
        if (!p->table || !p->ids || !table_ok(p->n_table)) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: the gather needs table [n_table][cols] and ids");
        for (int r = 0; r < n; ++r) if (p->ids[r] >= (uint32_t)p->n_table) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: ids[%d] = %u outside the table (%d)", r, p->ids[r], p->n_table);
        payload = (size_t)n * cols;
    } else if (mode == 1) {
        if (!p->src || !p->text_row || !p->codec_id || !p->table || !table_ok(p->n_table) || !table_ok(p->n_rows))
            return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: the assembly needs rows [n_rows][cols], text_row, codec_id and codec_emb [n_table][cols]");
        for (int i = 0; i < n; ++i) {
            const int tr = p->text_row[i], cid = p->codec_id[i];
            if (tr >= p->n_rows) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: text_row[%d] = %d outside rows (%d)", i, tr, p->n_rows);
            if (cid >= p->n_table) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: codec_id[%d] = %d outside codec_emb (%d)", i, cid, p->n_table);
            if (cid == -2 && !p->xvec) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: codec_id[%d] = -2 without xvec", i);
            if (cid <= -3) {
                const long long fr = -3LL - cid;
                if (!p->ref_codes || !p->cp_embs || !table_ok(p->cp_vocab) || p->n_ref < 1 || fr >= p->n_ref)
                    return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: codec_id[%d] = %d names frame %lld beyond ref_codes (%d frames)", i, cid, fr, p->ref_codes ? p->n_ref : 0);
                const uint32_t* f = p->ref_codes + (size_t)fr * 16;
                if (f[0] >= (uint32_t)p->n_table) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: ref_codes[%lld][0] = %u outside codec_emb (%d)", fr, f[0], p->n_table);
                for (int g = 1; g < 16; ++g)
                    if (f[g] >= (uint32_t)p->cp_vocab) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: ref_codes[%lld][%d] = %u outside its table (%d)", fr, g, f[g], p->cp_vocab);
            }
        }
        payload = (size_t)n * cols;
    } else if (mode == 2) {
        if (!p->src || p->lds < cols || p->ldd < cols || p->lds > (1 << 20) || p->ldd > (1 << 20)) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: the copy needs src and cols <= lds, ldd");
        payload = (size_t)n * p->ldd;
    } else if (mode == 3) {
        if (!p->src || !p->dst_row || !table_ok(p->n_rows)) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: the scatter needs src, dst_row and rows [n_rows][cols]");
        std::vector<char> seen((size_t)p->n_rows, 0);
        for (int r = 0; r < n; ++r) {
            const int d = p->dst_row[r];
            if (d < 0) continue;
            if (d >= p->n_rows) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: dst_row[%d] = %d outside rows (%d)", r, d, p->n_rows);
            if (seen[(size_t)d]) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: dst_row names row %d twice", d);
            seen[(size_t)d] = 1;
        }
        payload = (size_t)p->n_rows * cols;
    } else {
        if (!p->ent || !p->trail_len || !p->text_ready || !p->limit || !table_ok(p->n_rows))
            return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: the publish needs ent and trail_len / text_ready / limit [n_rows]");
        std::vector<char> seen((size_t)p->n_rows, 0);
        for (int i = 0; i < n; ++i) {
            const int b = p->ent[4 * i];
            if (b < 0 || b >= p->n_rows) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: ent[%d] names row %d outside [0, %d)", i, b, p->n_rows);
            if (seen[(size_t)b]) return set_err(Q3_INVALID_ARG, "q3_prompt_rows_ex: ent names row %d twice", b);
            seen[(size_t)b] = 1;
        }
    }
    HIPC(hipSetDevice(device));
    DevPool pool;
    auto up = [&](const void* h, size_t bytes, void** d) -> q3_status {
        char* q; HIPC(pool.alloc(&q, bytes)); HIPC(q3_hipMemcpy(q, h, bytes, hipMemcpyHostToDevice)); *d = q;
        return Q3_OK;
    };
    void* d = nullptr;
    if (mode == 4) {
        const size_t bytes = ((size_t)p->n_rows + 2 * G) * 4;
        int *ent, *tl, *trd, *lim;
        Q3C(up(p->ent, (size_t)n * 16, &d)); ent = (int*)d;
        Q3C(up(p->trail_len, bytes, &d)); tl = (int*)d; Q3C(up(p->text_ready, bytes, &d)); trd = (int*)d; Q3C(up(p->limit, bytes, &d)); lim = (int*)d;
        HIPC(q3_hipDeviceSynchronize());
        HIPC(launch_publish_text(ent, n, tl + G, trd + G, lim + G, 0));
        HIPC(q3_hipDeviceSynchronize());
        HIPC(q3_hipMemcpy(p->trail_len, tl, bytes, hipMemcpyDeviceToHost)); HIPC(q3_hipMemcpy(p->text_ready, trd, bytes, hipMemcpyDeviceToHost));
        HIPC(q3_hipMemcpy(p->limit, lim, bytes, hipMemcpyDeviceToHost));
        return Q3_OK;
    }
    const size_t out_bytes = (payload + 2 * G) * 4;
    float* out;
    Q3C(up(p->out, out_bytes, &d)); out = (float*)d + G;
    hipError_t e = hipSuccess;
    if (mode == 0) {
        const uint16_t* table; const uint32_t* ids;
        Q3C(up(p->table, (size_t)p->n_table * cols * 2, &d)); table = (const uint16_t*)d;
        Q3C(up(p->ids, (size_t)n * 4, &d)); ids = (const uint32_t*)d;
        HIPC(q3_hipDeviceSynchronize());
        e = launch_gather_rows_bf16(table, ids, out, n, cols, 0);
    } else if (mode == 1) {
        const float *rows, *xvec = nullptr; const int *tr, *ci; const uint16_t *emb, *cp = nullptr; const uint32_t* ref = nullptr;
        const uint16_t* const* cp_tab = nullptr;
        Q3C(up(p->src, (size_t)p->n_rows * cols * 4, &d)); rows = (const float*)d;
        Q3C(up(p->text_row, (size_t)n * 4, &d)); tr = (const int*)d; Q3C(up(p->codec_id, (size_t)n * 4, &d)); ci = (const int*)d;
        Q3C(up(p->table, (size_t)p->n_table * cols * 2, &d)); emb = (const uint16_t*)d;
        if (p->xvec) { Q3C(up(p->xvec, (size_t)cols * 4, &d)); xvec = (const float*)d; }
        if (p->ref_codes && p->cp_embs && p->n_ref >= 1 && table_ok(p->cp_vocab)) {
            Q3C(up(p->ref_codes, (size_t)p->n_ref * 64, &d)); ref = (const uint32_t*)d;
            Q3C(up(p->cp_embs, (size_t)15 * p->cp_vocab * cols * 2, &d)); cp = (const uint16_t*)d;
            const uint16_t* tabs[15];
            for (int g = 0; g < 15; ++g) tabs[g] = cp + (size_t)g * p->cp_vocab * cols;
            Q3C(up(tabs, sizeof(tabs), &d)); cp_tab = (const uint16_t* const*)d;
        }
        HIPC(q3_hipDeviceSynchronize());
        e = launch_assemble_rows(rows, tr, emb, ci, xvec, out, n, cols, 0, ref, cp_tab);
    } else if (mode == 2) {
        const float* src;
        Q3C(up(p->src, (size_t)n * p->lds * 4, &d)); src = (const float*)d;
        HIPC(q3_hipDeviceSynchronize());
        e = launch_copy_rows(src, p->lds, out, p->ldd, n, cols, 0);
    } else {
        const float* src; const int* dr;
        Q3C(up(p->src, (size_t)n * cols * 4, &d)); src = (const float*)d;
        Q3C(up(p->dst_row, (size_t)n * 4, &d)); dr = (const int*)d;
        HIPC(q3_hipDeviceSynchronize());
        e = launch_scatter_rows(src, dr, out, n, cols, 0);
    }
    HIPC(e);
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(p->out, out - G, out_bytes, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// ---- the codec transformer's attention family and its small neighbours, one launch at a time (tests/test_gpu_codec_attn_ops.py) ----
extern "C" int q3_attn_c_path(int hd, int kernel) {
    if (hd != 64 || kernel < -1 || kernel > ATTN_C_MFMA) return -1;
    return kernel < 0 ? attn_c_pick() : kernel;
}

// One launch_attn_c / launch_attn_cs / launch_attn_cb / launch_mimi_attn call over host arrays. Everything a kernel would address
// is checked against the buffers first: a bad shape is a status, never a launch. o is uploaded whole and copied back whole; the
// caches go up as given (NaNs beyond a row's end included).
extern "C" q3_status q3_attn_c_ex(int device, const q3_attn_c_ex_args* p) {
    if (!p || !p->q || !p->o) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: null argument");
    const int mode = p->mode, nh = p->nh, hd = p->hd;
    if (mode < 0 || mode > 3) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: mode 0..3");
    if (hd != 64 || nh < 1 || nh > 64) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: bad shape (hd == 64, 1 <= nh <= 64)");
    const int QD = nh * hd;
    const bool whole = mode == 0 || mode == 3, blk = mode == 2;
    if (whole) {
        if (!p->k || !p->v) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: null argument");
        if (p->L < 1 || p->L > (1 << 16)) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: bad shape (L 1..65536)");
        if (mode == 0 && (p->kernel < -1 || p->kernel > ATTN_C_MFMA)) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: kernel -1..1");
        if (mode == 3 && p->window < 1) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: window >= 1");
    } else {
        if (!p->rows || !p->caches || (blk && (!p->tabs || !p->tab0 || !p->tab_n))) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: null argument");
        if (p->N < 1 || p->N > (1 << 16) || p->n_rows < 1 || p->n_rows > 1024 || p->layers < 1 || p->layers > 64 || p->layer < 0 || p->layer >= p->layers ||
            p->cap < 1 || p->cap > (1 << 16))
            return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: bad shape (N, cap 1..65536, n_rows 1..1024, layer inside layers 1..64)");
        if (blk && (p->cap % 32 != 0 || p->n_blocks < 1 || p->n_blocks > (1 << 16) || p->n_tabs < 1 || p->n_tabs > (1 << 20)))
            return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: bad shape (bf a multiple of 32, n_blocks 1..65536, n_tabs 1..2^20)");
        for (int r = 0; r < p->n_rows; ++r) {
            const int a0 = p->rows[3 * r], e = p->rows[3 * r + 1], qcol = p->rows[3 * r + 2];
            if (a0 < 0 || e <= a0) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: row %d: no new frames (a0 = %d, e = %d)", r, a0, e);
            if (qcol < 0 || qcol > p->N || e - a0 > p->N - qcol) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: row %d: columns %d .. %d outside [0, %d)", r, qcol, qcol + e - a0, p->N);
            if (!blk) {
                if (e > p->cap) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: row %d ends at %d, beyond its cache (%d)", r, e, p->cap);
                continue;
            }
            const int t0 = p->tab0[r], tn = p->tab_n[r], need = (e + p->cap - 1) / p->cap;
            if (t0 < 0 || tn < 0 || t0 > p->n_tabs || tn > p->n_tabs - t0) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: row %d: block list %d + %d outside the table (%d)", r, t0, tn, p->n_tabs);
            if (tn < need) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: row %d: %d blocks for %d frames of %d per block", r, tn, e, p->cap);
            for (int b = 0; b < tn; ++b)
                if (p->tabs[t0 + b] < 0 || p->tabs[t0 + b] >= p->n_blocks) return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: row %d: block %d outside the pool (%d)", r, p->tabs[t0 + b], p->n_blocks);
        }
    }
    HIPC(hipSetDevice(device));
    DevPool pool;
    const size_t cols = whole ? (size_t)p->L : (size_t)p->N, qn = (size_t)QD * cols;
    float *q, *o, *k = nullptr, *v = nullptr;
    HIPC(pool.alloc(&q, qn)); HIPC(pool.alloc(&o, qn));
    HIPC(q3_hipMemcpy(q, p->q, qn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(o, p->o, qn * 4, hipMemcpyHostToDevice));
    hipError_t e;
    if (whole) {
        HIPC(pool.alloc(&k, qn)); HIPC(pool.alloc(&v, qn));
        HIPC(q3_hipMemcpy(k, p->k, qn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(v, p->v, qn * 4, hipMemcpyHostToDevice));
        HIPC(q3_hipDeviceSynchronize());
        if (mode == 0) e = launch_attn_c(q, k, v, o, nh, hd, p->L, p->scale, p->kernel < 0 ? attn_c_pick() : p->kernel, 0);
        else e = launch_mimi_attn(q, k, v, o, nh, hd, p->L, p->window, p->scale, 0);
    } else {
        const size_t unit = (size_t)p->layers * 2 * QD * p->cap;              // one row's cache / one block
        const size_t cn = unit * (blk ? (size_t)p->n_blocks : (size_t)p->n_rows), layer_off = (size_t)p->layer * 2 * QD * p->cap;
        float* kv; HIPC(pool.alloc(&kv, cn)); HIPC(q3_hipMemcpy(kv, p->caches, cn * 4, hipMemcpyHostToDevice));
        int max_tiles = 0;
        for (int r = 0; r < p->n_rows; ++r) max_tiles = std::max(max_tiles, ((p->rows[3 * r + 1] - 1) >> 5) - (p->rows[3 * r] >> 5) + 1);
        if (blk) {
            std::vector<AttnCbRow> rows((size_t)p->n_rows); std::vector<const float*> tabs((size_t)p->n_tabs);
            for (int r = 0; r < p->n_rows; ++r) rows[(size_t)r] = AttnCbRow{p->tab0[r], p->rows[3 * r], p->rows[3 * r + 1], p->rows[3 * r + 2]};
            for (int i = 0; i < p->n_tabs; ++i) {          // entries no row owns may hold anything: they point at block 0
                const int b = p->tabs[i];
                tabs[(size_t)i] = kv + unit * (size_t)((b < 0 || b >= p->n_blocks) ? 0 : b);
            }
            AttnCbRow* rd; const float** td;
            HIPC(pool.alloc(&rd, rows.size())); HIPC(pool.alloc(&td, tabs.size()));
            HIPC(q3_hipMemcpy(rd, rows.data(), rows.size() * sizeof(AttnCbRow), hipMemcpyHostToDevice));
            HIPC(q3_hipMemcpy(td, tabs.data(), tabs.size() * sizeof(const float*), hipMemcpyHostToDevice));
            HIPC(q3_hipDeviceSynchronize());
            e = launch_attn_cb(q, o, rd, td, p->n_rows, max_tiles, layer_off, nh, hd, p->N, p->cap, p->scale, 0);
        } else {
            std::vector<AttnCsRow> rows((size_t)p->n_rows);
            for (int r = 0; r < p->n_rows; ++r) rows[(size_t)r] = AttnCsRow{kv + unit * (size_t)r, p->rows[3 * r], p->rows[3 * r + 1], p->rows[3 * r + 2]};
            AttnCsRow* rd;
            HIPC(pool.alloc(&rd, rows.size()));
            HIPC(q3_hipMemcpy(rd, rows.data(), rows.size() * sizeof(AttnCsRow), hipMemcpyHostToDevice));
            HIPC(q3_hipDeviceSynchronize());
            e = launch_attn_cs(q, o, rd, p->n_rows, max_tiles, layer_off, nh, hd, p->N, p->cap, p->scale, 0);
        }
    }
    if (e == hipErrorInvalidValue) {
        (void)hipGetLastError();
        return set_err(Q3_INVALID_ARG, "q3_attn_c_ex: the launcher refused mode=%d nh=%d hd=%d (%s)", mode, nh, hd, hipGetErrorString(e));
    }
    HIPC(e);
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(p->o, o, qn * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_rope_c_ex(int device, float* q_host, float* k_host, const float* cs_host, const float* sn_host, const int* pos_host, int nh,
                                  int hd, int L, int n_pos) {
    if (!q_host || !k_host || !cs_host || !sn_host) return set_err(Q3_INVALID_ARG, "q3_rope_c_ex: null argument");
    if (nh < 1 || nh > 64 || hd < 2 || hd > 256 || hd % 2 || L < 1 || L > (1 << 20) || n_pos < 1 || n_pos > (1 << 20))
        return set_err(Q3_INVALID_ARG, "q3_rope_c_ex: bad shape (nh 1..64, hd even 2..256, L, n_pos 1..2^20)");
    if (!pos_host && n_pos < L) return set_err(Q3_INVALID_ARG, "q3_rope_c_ex: %d positions for %d columns", n_pos, L);
    if (pos_host) for (int t = 0; t < L; ++t) if (pos_host[t] < 0 || pos_host[t] >= n_pos) return set_err(Q3_INVALID_ARG, "q3_rope_c_ex: pos[%d] = %d outside [0, %d)", t, pos_host[t], n_pos);
    HIPC(hipSetDevice(device));
    DevPool pool;
    const size_t n = (size_t)nh * hd * L, rn = (size_t)n_pos * (hd / 2);
    float *q, *k, *cs, *sn; int* pos = nullptr;
    HIPC(pool.alloc(&q, n)); HIPC(pool.alloc(&k, n)); HIPC(pool.alloc(&cs, rn)); HIPC(pool.alloc(&sn, rn));
    HIPC(q3_hipMemcpy(q, q_host, n * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(k, k_host, n * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(cs, cs_host, rn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(sn, sn_host, rn * 4, hipMemcpyHostToDevice));
    if (pos_host) { HIPC(pool.alloc(&pos, (size_t)L)); HIPC(q3_hipMemcpy(pos, pos_host, (size_t)L * 4, hipMemcpyHostToDevice)); }
    HIPC(q3_hipDeviceSynchronize());
    if (pos) HIPC(launch_rope_c_pos(q, k, cs, sn, pos, nh, hd, L, 0));
    else HIPC(launch_rope_c(q, k, cs, sn, nh, hd, L, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(q_host, q, n * 4, hipMemcpyDeviceToHost)); HIPC(q3_hipMemcpy(k_host, k, n * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// does [off, off + (C - 1) * pitch] lie inside a buffer of `elems`?
static bool col_inside(size_t base, long long off, int pitch, int C, size_t elems) {
    if (off < 0 || pitch < 0) return false;
    const size_t last = base + (size_t)off + (size_t)(C - 1) * (size_t)pitch;
    return base <= elems && (size_t)off <= elems && last < elems;
}

extern "C" q3_status q3_copy_cols_ex(int device, const float* src_host, size_t src_elems, float* dst_host, size_t dst_elems, int n, int C,
                                     const long long* s_off, const long long* d_off, const int* sp, const int* dp, size_t src_off, size_t dst_off) {
    if (!src_host || !dst_host || !s_off || !d_off || !sp || !dp) return set_err(Q3_INVALID_ARG, "q3_copy_cols_ex: null argument");
    const size_t lim = (size_t)1 << 28;
    if (n < 1 || n > (1 << 20) || C < 1 || C > (1 << 16) || src_elems < 1 || src_elems > lim || dst_elems < 1 || dst_elems > lim)
        return set_err(Q3_INVALID_ARG, "q3_copy_cols_ex: bad shape (n 1..2^20, C 1..65536, buffers 1..2^28 floats)");
    for (int j = 0; j < n; ++j) {
        if (s_off[j] >= 0 && !col_inside(src_off, s_off[j], sp[j], C, src_elems)) return set_err(Q3_INVALID_ARG, "q3_copy_cols_ex: column %d leaves the source", j);
        if (!col_inside(dst_off, d_off[j], dp[j], C, dst_elems)) return set_err(Q3_INVALID_ARG, "q3_copy_cols_ex: column %d leaves the destination", j);
    }
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *src, *dst; ColCopy* dd;
    HIPC(pool.alloc(&src, src_elems)); HIPC(pool.alloc(&dst, dst_elems)); HIPC(pool.alloc(&dd, (size_t)n));
    std::vector<ColCopy> d((size_t)n);
    for (int j = 0; j < n; ++j) d[(size_t)j] = ColCopy{s_off[j] < 0 ? nullptr : src + s_off[j], dst + d_off[j], sp[j], dp[j]};
    HIPC(q3_hipMemcpy(src, src_host, src_elems * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(dst, dst_host, dst_elems * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(dd, d.data(), d.size() * sizeof(ColCopy), hipMemcpyHostToDevice));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_copy_cols(dd, n, C, src_off, dst_off, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(dst_host, dst, dst_elems * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_copy_segs_ex(int device, const float* src_host, size_t src_elems, float* dst_host, size_t dst_elems, int n_segs,
                                     const unsigned long long* segs_host) {
    if (!src_host || !dst_host || !segs_host) return set_err(Q3_INVALID_ARG, "q3_copy_segs_ex: null argument");
    const size_t lim = (size_t)1 << 28;
    if (n_segs < 1 || n_segs > 65535 || src_elems < 1 || src_elems > lim || dst_elems < 1 || dst_elems > lim)
        return set_err(Q3_INVALID_ARG, "q3_copy_segs_ex: bad shape (1..65535 segments, buffers 1..2^28 floats)");
    std::vector<SegCopy> segs((size_t)n_segs); size_t max_n = 0;
    for (int i = 0; i < n_segs; ++i) {
        const unsigned long long s = segs_host[3 * i], d = segs_host[3 * i + 1], n = segs_host[3 * i + 2];
        if (s > src_elems || n > src_elems - s || d > dst_elems || n > dst_elems - d)
            return set_err(Q3_INVALID_ARG, "q3_copy_segs_ex: segment %d (%llu floats at %llu -> %llu) leaves its buffers", i, n, s, d);
        segs[(size_t)i] = SegCopy{s, d, n}; max_n = std::max(max_n, (size_t)n);
    }
    if (max_n == 0) return set_err(Q3_INVALID_ARG, "q3_copy_segs_ex: every segment is empty");
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *src, *dst; SegCopy* sd;
    HIPC(pool.alloc(&src, src_elems)); HIPC(pool.alloc(&dst, dst_elems)); HIPC(pool.alloc(&sd, segs.size()));
    HIPC(q3_hipMemcpy(src, src_host, src_elems * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(dst, dst_host, dst_elems * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(sd, segs.data(), segs.size() * sizeof(SegCopy), hipMemcpyHostToDevice));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_copy_segs(src, dst, sd, n_segs, max_n, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(dst_host, dst, dst_elems * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_gather_frames_ex(int device, const uint32_t* src_host, size_t src_elems, const long long* s_off, int n, uint32_t* dst_host,
                                         size_t dst_elems) {
    if (!src_host || !s_off || !dst_host) return set_err(Q3_INVALID_ARG, "q3_gather_frames_ex: null argument");
    const size_t lim = (size_t)1 << 28;
    if (n < 1 || n > (1 << 20) || src_elems < 16 || src_elems > lim || dst_elems < (size_t)n * 16 || dst_elems > lim)
        return set_err(Q3_INVALID_ARG, "q3_gather_frames_ex: bad shape (n 1..2^20, source >= 16, destination >= 16 n, both <= 2^28)");
    for (int j = 0; j < n; ++j)
        if (s_off[j] < 0 || (size_t)s_off[j] > src_elems - 16) return set_err(Q3_INVALID_ARG, "q3_gather_frames_ex: frame %d leaves the source", j);
    HIPC(hipSetDevice(device));
    DevPool pool;
    uint32_t *src, *dst; const uint32_t** pd;
    HIPC(pool.alloc(&src, src_elems)); HIPC(pool.alloc(&dst, dst_elems)); HIPC(pool.alloc(&pd, (size_t)n));
    std::vector<const uint32_t*> ptrs((size_t)n);
    for (int j = 0; j < n; ++j) ptrs[(size_t)j] = src + s_off[j];
    HIPC(q3_hipMemcpy(src, src_host, src_elems * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(dst, dst_host, dst_elems * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(pd, ptrs.data(), ptrs.size() * sizeof(const uint32_t*), hipMemcpyHostToDevice));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_gather_frames(pd, dst, n, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(dst_host, dst, dst_elems * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_rvq_embed_ex(int device, const uint32_t* frames_host, int n_frames, const float* first_cb_host, const float* rest_cbs_host,
                                     int cb_dim, int cb_size, float* first_out_host, float* rest_out_host, int out_front, int out_elems) {
    if (!frames_host || !first_cb_host || !rest_cbs_host || !first_out_host || !rest_out_host) return set_err(Q3_INVALID_ARG, "q3_rvq_embed_ex: null argument");
    if (n_frames < 1 || n_frames > (1 << 16) || cb_dim < 1 || cb_dim > 256 || cb_size < 1 || cb_size > (1 << 16))
        return set_err(Q3_INVALID_ARG, "q3_rvq_embed_ex: bad shape (n_frames 1..65536, cb_dim 1..256, cb_size 1..65536)");
    if (out_front < 0 || out_elems < 0 || (size_t)out_elems < (size_t)out_front + (size_t)cb_dim * n_frames)
        return set_err(Q3_INVALID_ARG, "q3_rvq_embed_ex: the outputs must hold out_front + cb_dim * n_frames floats");
    HIPC(hipSetDevice(device));
    DevPool pool;
    const size_t cbn = (size_t)cb_size * cb_dim;
    uint32_t* frames; float *fcb, *rcb, *fo, *ro; const float** tabs;
    HIPC(pool.alloc(&frames, (size_t)n_frames * 16)); HIPC(pool.alloc(&fcb, cbn)); HIPC(pool.alloc(&rcb, cbn * 15));
    HIPC(pool.alloc(&fo, (size_t)out_elems)); HIPC(pool.alloc(&ro, (size_t)out_elems)); HIPC(pool.alloc(&tabs, 15));
    const float* th[15];
    for (int i = 0; i < 15; ++i) th[i] = rcb + (size_t)i * cbn;
    HIPC(q3_hipMemcpy(frames, frames_host, (size_t)n_frames * 64, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(fcb, first_cb_host, cbn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(rcb, rest_cbs_host, cbn * 15 * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(fo, first_out_host, (size_t)out_elems * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(ro, rest_out_host, (size_t)out_elems * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(tabs, th, sizeof th, hipMemcpyHostToDevice));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_rvq_embed(frames, n_frames, fcb, tabs, fo + out_front, ro + out_front, cb_dim, cb_size, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(first_out_host, fo, (size_t)out_elems * 4, hipMemcpyDeviceToHost)); HIPC(q3_hipMemcpy(rest_out_host, ro, (size_t)out_elems * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_silu_mul_ex(int device, const float* g_host, const float* u_host, float* y_host, long long n, long long y_elems) {
    if (!g_host || !u_host || !y_host) return set_err(Q3_INVALID_ARG, "q3_silu_mul_ex: null argument");
    if (n < 1 || n > (1LL << 28) || y_elems < n || y_elems > (1LL << 28)) return set_err(Q3_INVALID_ARG, "q3_silu_mul_ex: bad shape (1 <= n <= y_elems <= 2^28)");
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *g, *u, *y;
    HIPC(pool.alloc(&g, (size_t)n)); HIPC(pool.alloc(&u, (size_t)n)); HIPC(pool.alloc(&y, (size_t)y_elems));
    HIPC(q3_hipMemcpy(g, g_host, (size_t)n * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(u, u_host, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(y, y_host, (size_t)y_elems * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_silu_mul(g, u, y, (int64_t)n, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(y_host, y, (size_t)y_elems * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// ---- the voice-clone encoders' own kernels, one launch at a time (tests/test_gpu_clone_ops.py) ----
// the shared frame of q3_spk_op_ex / q3_mimi_op_ex: a (and b) up, `out` up whole, one launch on out + out_front, `out` back whole
template <typename Launch>
static q3_status clone_op_run(const char* who, int device, const float* a_host, size_t a_n, const float* b_host, size_t b_n, float* out_host,
                              size_t out_front, size_t out_n, Launch launch) {
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *a, *b = nullptr, *out;
    HIPC(pool.alloc(&a, a_n)); HIPC(pool.alloc(&out, out_n));
    HIPC(q3_hipMemcpy(a, a_host, a_n * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(out, out_host, out_n * 4, hipMemcpyHostToDevice));
    if (b_host) { HIPC(pool.alloc(&b, b_n)); HIPC(q3_hipMemcpy(b, b_host, b_n * 4, hipMemcpyHostToDevice)); }
    HIPC(q3_hipDeviceSynchronize());
    const hipError_t e = launch(a, b, out + out_front);
    if (e == hipErrorInvalidValue) {
        (void)hipGetLastError();
        return set_err(Q3_INVALID_ARG, "%s: the launcher refused its arguments (%s)", who, hipGetErrorString(e));
    }
    HIPC(e);
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(out_host, out, out_n * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_spk_op_ex(int device, const q3_spk_op_ex_args* p) {
    if (!p || !p->a || !p->out) return set_err(Q3_INVALID_ARG, "q3_spk_op_ex: null argument");
    const int op = p->op, C = p->C, T = p->T;
    const long long lim = 1LL << 28;
    if (op < 0 || op > 5) return set_err(Q3_INVALID_ARG, "q3_spk_op_ex: op 0..5");
    if (C < 1 || C > 65535 || T < 1 || T > (1 << 20)) return set_err(Q3_INVALID_ARG, "q3_spk_op_ex: bad shape (C 1..65535, T 1..2^20)");
    if (p->a_elems < 1 || p->a_elems > lim || p->b_elems < 0 || p->b_elems > lim || p->out_elems < 1 || p->out_elems > lim || p->out_front < 0 ||
        p->out_front > p->out_elems || (p->b == nullptr) != (p->b_elems == 0))
        return set_err(Q3_INVALID_ARG, "q3_spk_op_ex: bad buffers (1..2^28 floats each, out_front inside out, b_elems 0 exactly when b is null)");
    const long long CT = (long long)C * T;
    long long need_a = CT, need_b = 0, need_out = 0;
    switch (op) {
    case 0: {
        const long long pr = (long long)p->Tp - T - p->pl;
        if (p->pl < 0 || p->pl > T - 1 || p->Tp > (1 << 20) || pr < 0 || pr > T - 1)
            return set_err(Q3_INVALID_ARG, "q3_spk_op_ex: pad of %d + %lld columns around T = %d (each side 0..T - 1, Tp <= 2^20)", p->pl, pr, T);
        need_b = p->b ? CT : 0; need_out = (long long)C * p->Tp;
        break;
    }
    case 1:
        if (p->ld < 1 || p->ld > (1 << 20) || p->off < 0 || T > p->ld - p->off)
            return set_err(Q3_INVALID_ARG, "q3_spk_op_ex: columns %d .. %d outside a row of %d", p->off, p->off + T, p->ld);
        need_a = (long long)C * p->ld; need_out = CT;
        break;
    case 2: need_out = C; break;
    case 3: need_b = C; need_out = CT; break;
    case 4: need_out = 3 * CT; break;
    default: need_b = CT; need_out = 2LL * C; break;
    }
    if ((op == 3 || op == 5) && !p->b) return set_err(Q3_INVALID_ARG, "q3_spk_op_ex: op %d needs b", op);
    if ((op == 1 || op == 2 || op == 4) && p->b) return set_err(Q3_INVALID_ARG, "q3_spk_op_ex: op %d takes no b", op);
    if (p->a_elems < need_a || p->b_elems < need_b || need_out > p->out_elems - p->out_front)
        return set_err(Q3_INVALID_ARG, "q3_spk_op_ex: op %d needs %lld / %lld / %lld floats in a / b / out behind out_front", op, need_a, need_b, need_out);
    return clone_op_run("q3_spk_op_ex", device, p->a, (size_t)p->a_elems, p->b, (size_t)p->b_elems, p->out, (size_t)p->out_front, (size_t)p->out_elems,
                        [&](const float* a, const float* b, float* out) -> hipError_t {
                            switch (op) {
                            case 0: return launch_spk_pad(a, b, out, C, T, p->pl, p->Tp, 0);
                            case 1: return launch_spk_cols(a, p->ld, p->off, out, C, T, 0);
                            case 2: return launch_spk_mean(a, out, C, T, 0);
                            case 3: return launch_spk_se_apply(a, b, out, C, T, 0);
                            case 4: return launch_spk_asp_in(a, out, C, T, 0);
                            default: return launch_spk_asp_pool(a, b, out, C, T, 0);
                            }
                        });
}

extern "C" q3_status q3_mimi_op_ex(int device, const q3_mimi_op_ex_args* p) {
    if (!p || !p->a || !p->out) return set_err(Q3_INVALID_ARG, "q3_mimi_op_ex: null argument");
    const int op = p->op, C = p->C, L = p->L, r = p->r, Lf = p->Lf;
    const long long lim = 1LL << 28;
    if (op < 0 || op > 2) return set_err(Q3_INVALID_ARG, "q3_mimi_op_ex: op 0..2");
    if (L < 1 || L > (1 << 24)) return set_err(Q3_INVALID_ARG, "q3_mimi_op_ex: bad shape (L 1..2^24)");
    if (op != 0 && (C < 1 || C > 65535)) return set_err(Q3_INVALID_ARG, "q3_mimi_op_ex: bad shape (C 1..65535)");
    if (p->a_elems < 1 || p->a_elems > lim || p->b_elems < 0 || p->b_elems > lim || p->out_elems < 1 || p->out_elems > lim || p->out_front < 0 ||
        p->out_front > p->out_elems || (p->b == nullptr) != (p->b_elems == 0))
        return set_err(Q3_INVALID_ARG, "q3_mimi_op_ex: bad buffers (1..2^28 floats each, out_front inside out, b_elems 0 exactly when b is null)");
    long long need_a = L, need_b = 0, need_out = L;
    if (op == 1) {
        if (r < 1 || r > 64 || (long long)C * r > 65535 || Lf < 1 || Lf > (1 << 24))
            return set_err(Q3_INVALID_ARG, "q3_mimi_op_ex: bad fold (r 1..64, C * r <= 65535, Lf 1..2^24)");
        if (!p->replicate && (long long)(Lf - 1) * r >= L)
            return set_err(Q3_INVALID_ARG, "q3_mimi_op_ex: plain fold of L = %d by r = %d has no column %d ((Lf - 1) * r < L)", L, r, Lf - 1);
        need_a = (long long)C * L; need_out = (long long)C * r * (Lf + (p->replicate ? 1 : 0));
    } else if (op == 2) {
        need_a = need_out = (long long)C * L; need_b = C;
    }
    if ((op == 2) != (p->b != nullptr)) return set_err(Q3_INVALID_ARG, "q3_mimi_op_ex: b (cluster_usage) goes with op 2 alone");
    if (p->a_elems < need_a || p->b_elems < need_b || need_out > p->out_elems - p->out_front)
        return set_err(Q3_INVALID_ARG, "q3_mimi_op_ex: op %d needs %lld / %lld / %lld floats in a / b / out behind out_front", op, need_a, need_b, need_out);
    return clone_op_run("q3_mimi_op_ex", device, p->a, (size_t)p->a_elems, p->b, (size_t)p->b_elems, p->out, (size_t)p->out_front, (size_t)p->out_elems,
                        [&](const float* a, const float* b, float* out) -> hipError_t {
                            if (op == 0) return launch_mimi_elu(a, out, (size_t)L, 0);
                            if (op == 1) return launch_mimi_fold(a, out, C, L, r, Lf, p->elu, p->replicate, 0);
                            return launch_mimi_codebook(a, b, out, C, L, 0);
                        });
}

extern "C" q3_status q3_mimi_rvq_ex(int device, const float* proj_host, int T, const float* books_host, int n_layers, int CB, int CD,
                                    uint32_t* codes_host, int n_q, int q0) {
    if (!proj_host || !books_host || !codes_host) return set_err(Q3_INVALID_ARG, "q3_mimi_rvq_ex: null argument");
    if (CD < 1 || CD > 256 || CB < 1 || CB > (1 << 16) || T < 1 || T > (1 << 16))
        return set_err(Q3_INVALID_ARG, "q3_mimi_rvq_ex: bad shape (CD 1..256, CB 1..65536, T 1..65536)");
    if (n_layers < 1 || q0 < 0 || n_q < 1 || n_q > 64 || n_layers > n_q - q0)
        return set_err(Q3_INVALID_ARG, "q3_mimi_rvq_ex: layers %d .. %d outside a frame of %d codes (n_layers >= 1, q0 >= 0, n_q 1..64)", q0, q0 + n_layers, n_q);
    const size_t pn = (size_t)CD * T, bn = (size_t)n_layers * CB * CD, cn = (size_t)T * n_q;
    // the winner indexes the table: a frame whose every distance is inf or NaN has none, so the values must keep the distances finite
    for (size_t i = 0; i < pn; ++i) if (!(fabsf(proj_host[i]) < 1e12f)) return set_err(Q3_INVALID_ARG, "q3_mimi_rvq_ex: proj[%zu] is not finite or beyond 1e12", i);
    for (size_t i = 0; i < bn; ++i) if (!(fabsf(books_host[i]) < 1e12f)) return set_err(Q3_INVALID_ARG, "q3_mimi_rvq_ex: books[%zu] is not finite or beyond 1e12", i);
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *proj, *books; uint32_t* codes;
    HIPC(pool.alloc(&proj, pn)); HIPC(pool.alloc(&books, bn)); HIPC(pool.alloc(&codes, cn));
    HIPC(q3_hipMemcpy(proj, proj_host, pn * 4, hipMemcpyHostToDevice)); HIPC(q3_hipMemcpy(books, books_host, bn * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(codes, codes_host, cn * 4, hipMemcpyHostToDevice));
    HIPC(q3_hipDeviceSynchronize());
    const hipError_t e = launch_mimi_rvq(proj, T, books, n_layers, CB, CD, codes, n_q, q0, 0);
    if (e == hipErrorInvalidValue) {
        (void)hipGetLastError();
        return set_err(Q3_INVALID_ARG, "q3_mimi_rvq_ex: the launcher refused its arguments (%s)", hipGetErrorString(e));
    }
    HIPC(e);
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(codes_host, codes, cn * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

#ifdef Q3_TRACE
// development builds only (not declared in include/q3tts.h): arm the per-node stamp buffer BEFORE the first
// q3_session_generate (the captured graph keeps the slice pointers), then read the stamps of the last replayed frame.
extern "C" q3_status q3_debug_trace_enable(q3_session* s, int max_nodes) {
    if (!s || max_nodes < 1) return set_err(Q3_INVALID_ARG, "q3_debug_trace_enable");
    const size_t bytes = (size_t)max_nodes * TRACE_NODE * 8;
    HIPC(hipMalloc((void**)&s->trace_buf, bytes));
    HIPC(hipMemset(s->trace_buf, 0, bytes));
    s->trace_cap = max_nodes;
    return Q3_OK;
}
extern "C" q3_status q3_debug_trace_read(q3_session* s, unsigned long long* stamps_host, int* meta_host, int cap_nodes, int* n_nodes) {
    if (!s || !s->trace_buf || !n_nodes) return set_err(Q3_INVALID_ARG, "q3_debug_trace_read");
    HIPC(sync_frames(s));
    const int n = (int)s->trace_meta.size();
    *n_nodes = n;
    if (stamps_host && meta_host) {
        if (cap_nodes < n) return set_err(Q3_INVALID_ARG, "trace buffer too small");
        HIPC(q3_hipMemcpy(stamps_host, s->trace_buf, (size_t)n * TRACE_NODE * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            const auto& t = s->trace_meta[i];
            const int v[7] = {t.kind, t.a, t.b, t.c, t.d, t.e, t.f};
            memcpy(meta_host + (size_t)i * 7, v, sizeof v);
        }
    }
    return Q3_OK;
}
#endif

extern "C" q3_status q3_session_submit_info(q3_session* s, int* path, int* nodes) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (path) *path = s->aql ? 1 + s->aql_mode : s->graph ? 1 : 0;
    if (nodes) *nodes = s->aql ? q3::aql_program_nodes(s->aql) : 0;
    return Q3_OK;
}

extern "C" q3_status q3_session_submit_fences(q3_session* s, int* acquire_free, int* release_free) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    q3::aql_program_fence_free(s->aql, acquire_free, release_free);
    return Q3_OK;
}

extern "C" q3_status q3_session_frame_bytes(q3_session* s, int kv_len, double* weight_bytes, double* kv_bytes) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    const q3_config& c = s->m->cfg;
    auto layer_params = [](int H, int I, int nh, int nkv) { return (double)H * (nh + 2 * nkv) * HEAD_DIM + (double)H * nh * HEAD_DIM + 3.0 * (double)H * I; };
    const double talker = c.n_layers * layer_params(c.hidden, c.inter, c.n_heads, c.n_kv_heads) + (double)c.codec_vocab * c.hidden;
    const double cp_pass = c.cp_layers * layer_params(c.cp_hidden, c.cp_inter, c.cp_heads, c.cp_kv_heads) + (double)c.cp_vocab * c.cp_hidden +
                           (c.hidden != c.cp_hidden ? (double)c.cp_hidden * c.hidden : 0.0);
    if (weight_bytes) *weight_bytes = 2.0 * (talker + 15.0 * cp_pass);          // bf16; SURVEY §8(d)
    if (kv_bytes) {
        const double kv_tok = 2.0 * c.n_kv_heads * HEAD_DIM * (s->kv_bf16 ? 2.0 : 4.0) * c.n_layers;   // f32 K/V (default) or a bf16 session's
        const double cp_tok = 2.0 * c.cp_kv_heads * HEAD_DIM * 4.0 * c.cp_layers;
        *kv_bytes = s->B * (kv_tok * kv_len + cp_tok * 135.0);
    }
    return Q3_OK;
}

// profiling read-out: accumulated GPU milliseconds / algorithmic bytes / launches of the bf16 GEMV family
extern "C" q3_status q3_session_profile_read(q3_session* s, double* ms, double* bytes, long* launches, int reset) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (ms) *ms = s->prof_linear.ms; if (bytes) *bytes = s->prof_linear.bytes; if (launches) *launches = s->prof_linear.launches;
    if (reset) s->prof_linear = ProfAcc();
    return Q3_OK;
}

// the distinct GEMV launches (and how often each ran) since profiling was enabled / last reset: rows of 8 ints
// {M, N, K, epilogue, fused input RMSNorm (0 / 1), reserved (0), tiling, count} — what q3_bench_linear can replay
extern "C" q3_status q3_session_profile_shapes(q3_session* s, int* rows, int cap_rows, int* n_rows, int reset) {
    if (!s || !n_rows) return set_err(Q3_INVALID_ARG, "null argument");
    *n_rows = (int)s->prof_shapes.size();
    if (rows) {
        if (cap_rows < *n_rows) return set_err(Q3_INVALID_ARG, "shape buffer too small (%d < %d rows)", cap_rows, *n_rows);
        for (int i = 0; i < *n_rows; ++i) {
            const ProfShape& q = s->prof_shapes[i];
            const int v[8] = {q.M, q.N, q.K, q.epi, q.rms, q.produce, q.tiled, q.count};
            memcpy(rows + (size_t)i * 8, v, sizeof v);
        }
    }
    if (reset) s->prof_shapes.clear();
    return Q3_OK;
}

// ------------------------------------------------------------------------------------------------
// micro-benchmark of one GEMV shape (kernel development aid, used by tools/bench_kernels.py):
// `iters` back-to-back launches cycling over `n_copies` distinct weight buffers (so the stream comes
// from HBM, not the 256 MiB Infinity Cache), captured in one hipGraph and timed with HIP events.
// epi: LinEpi; rms: fused input RMSNorm; tiled: 1 = 16-row MFMA tiles, 2 = 4-row tiles, 3 = 16-row tiles with split-K in two,
// 0 = first-generation VALU kernel, < 0 = the engine's choice for an unsplit launch.
// ------------------------------------------------------------------------------------------------
extern "C" q3_status q3_bench_linear(int device, int M, int N, int K, int epi, int rms, int tiled, int iters, int n_copies,
                                     double* avg_us) {
    if (M < 1 || M > Q3_MAX_BATCH || N < 16 || K < 32 || iters < 1 || n_copies < 1 || !avg_us || epi < EPI_NONE || epi > EPI_SWIGLU || rms < 0 || rms > 1)
        return set_err(Q3_INVALID_ARG, "q3_bench_linear: bad argument (epi 0..3, rms 0/1)");
    if (tiled < 0) tiled = (M <= 16 && N < 4096 && !short_k_wide(N, K) && (M <= 2 || (N <= 1024 && M <= 8))) ? 2 : 1;    // the engine's choice (pick_mode)
    const bool sk2 = tiled == 3;          // 3 = 16-row tiles, split-K in two (LinArgs::ksplit): y alternates between two buffers,
    if (sk2) tiled = 1;                   // each launch clearing the other one as its side job, as the frame loop's neighbours do
    HIPC(hipSetDevice(device));
    DevPool pool;
    const size_t welems = tiled == 2 ? tiled_elems(2, N, K) : tiled_elems(1, N, K);
    const int nmat = epi == EPI_SWIGLU ? 2 : 1;
    uint16_t* w; float *x, *y, *nw, *res;
    HIPC(pool.alloc(&w, welems * nmat * n_copies));
    HIPC(pool.alloc(&x, (size_t)Q3_MAX_BATCH * K)); HIPC(pool.alloc(&y, (size_t)2 * Q3_MAX_BATCH * N)); HIPC(pool.alloc(&nw, (size_t)K)); HIPC(pool.alloc(&res, (size_t)Q3_MAX_BATCH * N));
    HIPC(hipMemset(y, 0, (size_t)2 * Q3_MAX_BATCH * N * 4));
    {   // random-ish bf16 weights / f32 activations (never zeros: DVFS, guide §5.4 rule 25)
        std::vector<uint16_t> hw(welems);
        q3_synth_fill(1, "bench.w", Q3_DTYPE_BF16, 0.02f, 0.0f, (int64_t)welems, hw.data());
        for (int c = 0; c < nmat * n_copies; ++c) HIPC(q3_hipMemcpy(w + (size_t)c * welems, hw.data(), welems * 2, hipMemcpyHostToDevice));
        std::vector<float> hx((size_t)Q3_MAX_BATCH * K), hn((size_t)K, 1.0f);
        q3_synth_fill(2, "bench.x", Q3_DTYPE_F32, 1.0f, 0.0f, (int64_t)hx.size(), hx.data());
        HIPC(q3_hipMemcpy(x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
        HIPC(q3_hipMemcpy(nw, hn.data(), hn.size() * 4, hipMemcpyHostToDevice));
    }
    hipStream_t st; HIPC(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    float* ws = nullptr; size_t ws_bytes = 0;
    if (M > 16 && tiled == 1 && N % 128 == 0 && K % 128 == 0) { ws_bytes = gemm_wide_ws_bytes(M, N, K, epi); HIPC(pool.alloc(&ws, ws_bytes / 4)); }
    auto one = [&](int i) -> hipError_t {
        LinArgs a;
        a.ws = ws; a.ws_bytes = ws_bytes;
        const int c = i % n_copies;
        a.W = w + (size_t)c * nmat * welems; a.W2 = nmat == 2 ? a.W + welems : nullptr;
        a.N = N; a.K = K; a.Kpad = tiled == 2 ? up128(K) : up32(K); a.tiled = tiled; a.x = x; a.ldx = K; a.y = y; a.ldy = N; a.M = M; a.epi = epi;
        if (rms) { a.norm_w = nw; a.eps = 1e-6f; }
        if (epi == EPI_RESID) { a.resid = res; a.ldr = N; }
        if (sk2) { a.ksplit = 2; a.y = y + (size_t)(i & 1) * Q3_MAX_BATCH * N; a.zero = y + (size_t)((i + 1) & 1) * Q3_MAX_BATCH * N; a.zero_n = M * N; }
        return launch_linear(a, st);
    };
    for (int i = 0; i < 4; ++i) HIPC(one(i));
    HIPC(hipStreamSynchronize(st));
    hipGraph_t g; hipGraphExec_t ge;
    HIPC(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    hipError_t e = hipSuccess;
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = one(i);
    hipError_t e2 = hipStreamEndCapture(st, &g);
    if (e != hipSuccess || e2 != hipSuccess) return set_err(Q3_HIP_ERROR, "bench capture failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    HIPC(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    HIPC(hipGraphLaunch(ge, st)); HIPC(hipStreamSynchronize(st));     // warm
    hipEvent_t ev0, ev1; HIPC(hipEventCreate(&ev0)); HIPC(hipEventCreate(&ev1));
    double sum = 0.0;          // mean over 5 replays (not the best one)
    for (int rep = 0; rep < 5; ++rep) {
        HIPC(hipEventRecord(ev0, st));
        HIPC(hipGraphLaunch(ge, st));
        HIPC(hipEventRecord(ev1, st));
        HIPC(hipStreamSynchronize(st));
        float ms = 0; HIPC(hipEventElapsedTime(&ms, ev0, ev1));
        sum += ms;
    }
    *avg_us = sum / 5.0 * 1000.0 / iters;
    hipEventDestroy(ev0); hipEventDestroy(ev1); hipGraphExecDestroy(ge); hipGraphDestroy(g); hipStreamDestroy(st);
    return Q3_OK;
}

// Op-level test entry: both host buffers (guard bytes included: the caller's business) go to the device, ONE launch runs the
// segment list, both come back (an exchange changes the source too). Offsets are bytes into the two buffers; a segment that does
// not lie inside both is refused before anything runs.
extern "C" q3_status q3_row_move(int device, void* src_host, size_t src_bytes, void* dst_host, size_t dst_bytes, int n_segs, const size_t* src_off,
                                 const size_t* dst_off, const size_t* seg_bytes, const int* mode) {
    if (!src_host || !dst_host || !src_off || !dst_off || !seg_bytes || !mode) return set_err(Q3_INVALID_ARG, "q3_row_move: null argument");
    if (n_segs < 1 || n_segs > 65535) return set_err(Q3_INVALID_ARG, "q3_row_move: %d segments outside 1..65535", n_segs);
    if (src_bytes == 0 || dst_bytes == 0) return set_err(Q3_INVALID_ARG, "q3_row_move: empty buffer");
    std::vector<RowSeg> segs((size_t)n_segs); size_t max_bytes = 0;
    for (int i = 0; i < n_segs; ++i) {
        if (mode[i] != ROW_MOVE_COPY && mode[i] != ROW_MOVE_EXCHANGE) return set_err(Q3_INVALID_ARG, "q3_row_move: segment %d: mode %d is neither copy (0) nor exchange (1)", i, mode[i]);
        if (src_off[i] > src_bytes || seg_bytes[i] > src_bytes - src_off[i] || dst_off[i] > dst_bytes || seg_bytes[i] > dst_bytes - dst_off[i])
            return set_err(Q3_INVALID_ARG, "q3_row_move: segment %d (%zu bytes at %zu -> %zu) leaves its buffers (%zu, %zu bytes)", i, seg_bytes[i], src_off[i], dst_off[i], src_bytes, dst_bytes);
        max_bytes = std::max(max_bytes, seg_bytes[i]);
    }
    HIPC(hipSetDevice(device));
    DevPool pool;
    char *sd = nullptr, *dd = nullptr; RowSeg* segs_dev = nullptr;
    HIPC(pool.alloc(&sd, src_bytes)); HIPC(pool.alloc(&dd, dst_bytes)); HIPC(pool.alloc(&segs_dev, (size_t)n_segs));
    for (int i = 0; i < n_segs; ++i) segs[(size_t)i] = RowSeg{sd + src_off[i], dd + dst_off[i], (unsigned long long)seg_bytes[i], mode[i], 0};
    HIPC(q3_hipMemcpy(sd, src_host, src_bytes, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(dd, dst_host, dst_bytes, hipMemcpyHostToDevice));
    HIPC(q3_hipMemcpy(segs_dev, segs.data(), segs.size() * sizeof(RowSeg), hipMemcpyHostToDevice));
    HIPC(launch_row_move(segs_dev, n_segs, max_bytes, nullptr));
    HIPC(q3_null_stream_sync());
    HIPC(q3_hipMemcpy(src_host, sd, src_bytes, hipMemcpyDeviceToHost));
    HIPC(q3_hipMemcpy(dst_host, dd, dst_bytes, hipMemcpyDeviceToHost));
    return Q3_OK;
}

// ---- the frame's sampler and seam kernels in their session forms (tests/test_gpu_sampler_op.py, tests/test_gpu_frame_seam.py) ----
// Every entry checks its arguments before the first device call, uploads every buffer a kernel may write WITH the caller's guard
// elements (`guard` in front of and behind it), runs ONE launch and copies those buffers back whole.
namespace {
template <typename T> hipError_t upload(DevPool& pool, T** dev, const T* host, size_t n) {
    hipError_t e = pool.alloc(dev, n);
    if (e != hipSuccess) return e;
    return q3_hipMemcpy(*dev, host, n * sizeof(T), hipMemcpyHostToDevice);
}
static_assert(sizeof(q3_sample_rec) == sizeof(SampleRow), "q3_sample_rec is SampleRow");
}  // namespace

extern "C" q3_status q3_sample_row(const q3_options* o, q3_sample_rec* out) {
    if (!o || !out) return set_err(Q3_INVALID_ARG, "q3_sample_row: null argument");
    const SampleRow r = sample_row(*o);
    memcpy(out, &r, sizeof r);
    return Q3_OK;
}

extern "C" q3_status q3_prompt_shape(const q3_request* r, int n_text, q3_prompt_shape_rec* out, int* text_row, int* codec_id, int cap_positions) {
    if (!r || !out) return set_err(Q3_INVALID_ARG, "q3_prompt_shape: null argument");
    if (n_text < 0 || r->n_instruct < 0 || r->n_ref < 0 || r->n_ref_text < 0) return set_err(Q3_INVALID_ARG, "q3_prompt_shape: negative length");
    if ((long long)n_text + r->n_instruct + r->n_ref + r->n_ref_text > (1 << 28)) return set_err(Q3_INVALID_ARG, "q3_prompt_shape: lengths beyond 2^28");
    *out = prompt_shape(*r, n_text);
    if (!text_row && !codec_id) return Q3_OK;
    if (!text_row || !codec_id) return set_err(Q3_INVALID_ARG, "q3_prompt_shape: one table without the other");
    if (cap_positions < out->prefill_len) return set_err(Q3_INVALID_ARG, "q3_prompt_shape: tables of %d positions, the prompt has %d", cap_positions, out->prefill_len);
    prompt_positions(*out, *r, 0, text_row, codec_id);
    return Q3_OK;
}

extern "C" q3_status q3_sample_ex(int device, const q3_sample_ex_args* p) {
    if (!p || !p->logits || !p->u || !p->tok) return set_err(Q3_INVALID_ARG, "q3_sample_ex: null argument");
    const int B = p->B, V = p->vocab, G = p->guard;
    if (V < 2 || V > 4096) return set_err(Q3_INVALID_ARG, "q3_sample_ex: vocab %d outside 2..4096", V);
    if (B < 1 || B > 1024 || G < 0 || G > 4096 || p->ld < V || p->ld > (1 << 16) || p->u_stride < 1 || p->u_elems < 1)
        return set_err(Q3_INVALID_ARG, "q3_sample_ex: bad shape (B 1..1024, guard 0..4096, vocab <= ld <= 65536, u_stride >= 1, u_elems >= 1)");
    if (p->advance && (!p->frame_idx || !p->pos)) return set_err(Q3_INVALID_ARG, "q3_sample_ex: advance needs frame_idx and pos");
    if (p->logits_hist && (p->hist_cap < 0 || p->hist_cap > 4096 || (long long)p->hist_stride_b < (long long)p->hist_cap * V))
        return set_err(Q3_INVALID_ARG, "q3_sample_ex: logits_hist needs 0 <= hist_cap <= 4096 and hist_stride_b >= hist_cap * vocab");
    for (int b = 0; b < B; ++b) {
        const long long d = p->draw_idx ? p->draw_idx[b] : 0, at = (long long)b * p->u_stride + d;
        if (d < 0 || at >= p->u_elems) return set_err(Q3_INVALID_ARG, "q3_sample_ex: row %d draws u[%lld] of %d", b, at, p->u_elems);
        const int tc = p->token_count ? p->token_count[G + b] : p->token_count_static;
        if (p->logits_hist && tc < 0) return set_err(Q3_INVALID_ARG, "q3_sample_ex: row %d: token_count %d indexes logits_hist", b, tc);
    }
    HIPC(hipSetDevice(device));
    DevPool pool;
    const size_t nB = (size_t)B + 2 * (size_t)G, n_seen = (size_t)B * V + 2 * (size_t)G, n_hist = (size_t)B * (size_t)p->hist_stride_b + 2 * (size_t)G;
    float *lg, *u, *hist = nullptr; uint8_t* seen = nullptr; uint32_t* tok; int *tc = nullptr, *fi = nullptr, *pos = nullptr, *didx = nullptr, *lim = nullptr, *rdy = nullptr;
    SampleRow* rows = nullptr;
    HIPC(upload(pool, &lg, p->logits, (size_t)B * p->ld)); HIPC(upload(pool, &u, p->u, (size_t)p->u_elems)); HIPC(upload(pool, &tok, p->tok, nB));
    if (p->seen) HIPC(upload(pool, &seen, p->seen, n_seen));
    if (p->draw_idx) HIPC(upload(pool, &didx, const_cast<int*>(p->draw_idx), (size_t)B));
    if (p->rows) HIPC(upload(pool, &rows, reinterpret_cast<SampleRow*>(const_cast<q3_sample_rec*>(p->rows)), (size_t)B));
    if (p->token_count) HIPC(upload(pool, &tc, p->token_count, nB));
    if (p->frame_idx) HIPC(upload(pool, &fi, p->frame_idx, nB));
    if (p->pos) HIPC(upload(pool, &pos, p->pos, nB));
    if (p->limit) HIPC(upload(pool, &lim, const_cast<int*>(p->limit), (size_t)B));
    if (p->text_ready) HIPC(upload(pool, &rdy, const_cast<int*>(p->text_ready), (size_t)B));
    if (p->logits_hist) HIPC(upload(pool, &hist, p->logits_hist, n_hist));
    SampleArgs a; memset(&a, 0, sizeof a);
    a.logits = lg; a.ld = p->ld; a.seen = seen ? seen + G : nullptr; a.u = u; a.u_stride = p->u_stride; a.draw_idx = didx; a.tok = tok + G;
    a.token_count = tc ? tc + G : nullptr; a.token_count_static = p->token_count_static;
    a.frame_idx = fi ? fi + G : nullptr; a.pos = pos ? pos + G : nullptr; a.advance = p->advance; a.rows = rows; a.limit = lim; a.text_ready = rdy;
    a.logits_hist = hist ? hist + G : nullptr; a.hist_stride_b = p->hist_stride_b; a.hist_cap = p->hist_cap; a.vocab = V; a.B = B;
    const q3_sample_rec& s = p->scalar;
    a.inv_temp = s.inv_temp; a.apply_temp = s.apply_temp; a.greedy = s.greedy; a.top_k = s.top_k; a.top_p = s.top_p; a.use_top_p = s.use_top_p;
    a.rep_pen = s.rep_pen; a.rep_inv = s.rep_inv; a.use_rep = s.use_rep; a.eos_id = s.eos_id; a.min_new_tokens = s.min_new_tokens;
    a.codec_eos = p->codec_eos; a.use_suppress = p->use_suppress;
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_sample(a, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(p->tok, tok, nB * 4, hipMemcpyDeviceToHost));
    if (seen) HIPC(q3_hipMemcpy(p->seen, seen, n_seen, hipMemcpyDeviceToHost));
    if (tc) HIPC(q3_hipMemcpy(p->token_count, tc, nB * 4, hipMemcpyDeviceToHost));
    if (fi) HIPC(q3_hipMemcpy(p->frame_idx, fi, nB * 4, hipMemcpyDeviceToHost));
    if (pos) HIPC(q3_hipMemcpy(p->pos, pos, nB * 4, hipMemcpyDeviceToHost));
    if (hist) HIPC(q3_hipMemcpy(p->logits_hist, hist, n_hist * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_frame_embed_ex(int device, const q3_frame_embed_ex_args* p) {
    if (!p || !p->codec_emb || !p->cp_embs || !p->tok || !p->cp_logits_last || !p->codes || !p->frame_idx || !p->text_rows || !p->trail_base ||
        !p->trail_len || !p->pad_row || !p->out)
        return set_err(Q3_INVALID_ARG, "q3_frame_embed_ex: null argument");
    const int B = p->B, H = p->H, V = p->cp_vocab, MF = p->max_frames, G = p->guard;
    if (B < 1 || B > 1024 || H < 1 || H > 8192 || V < 1 || V > 65536 || MF < 1 || MF > 4096 || p->n_sem < 1 || p->n_sem > 65536 || p->n_text_rows < 1 ||
        p->n_text_rows > (1 << 20) || G < 0 || G > 4096)
        return set_err(Q3_INVALID_ARG, "q3_frame_embed_ex: bad shape (B 1..1024, H 1..8192, cp_vocab, n_sem 1..65536, max_frames 1..4096, guard 0..4096)");
    for (int b = 0; b < B; ++b) {
        const int f = p->frame_idx[b];
        if (f < 0 || f > MF) return set_err(Q3_INVALID_ARG, "q3_frame_embed_ex: row %d: frame_idx %d outside [0, %d]", b, f, MF);
        if (p->tok[b] >= (uint32_t)p->n_sem) return set_err(Q3_INVALID_ARG, "q3_frame_embed_ex: row %d: token %u outside the table", b, p->tok[b]);
        const uint32_t* slot = p->codes + G + ((size_t)b * MF + (f < MF ? f : MF - 1)) * 16;
        for (int g = 1; g < 15; ++g)
            if (slot[g] >= (uint32_t)V) return set_err(Q3_INVALID_ARG, "q3_frame_embed_ex: row %d: code %d = %u outside the table", b, g, slot[g]);
        const long long row = f < p->trail_len[b] ? (long long)p->trail_base[b] + f : (long long)p->pad_row[b];
        if (row < 0 || row >= p->n_text_rows) return set_err(Q3_INVALID_ARG, "q3_frame_embed_ex: row %d: text row %lld of %d", b, row, p->n_text_rows);
    }
    HIPC(hipSetDevice(device));
    DevPool pool;
    const size_t n_codes = (size_t)B * MF * 16 + 2 * (size_t)G, n_out = (size_t)B * H + 2 * (size_t)G, tab = (size_t)V * H;
    uint16_t *sem, *embs; uint32_t *tok, *codes; float *lg, *text, *out; int *fi, *tb, *tl, *pr, *rdy = nullptr;
    HIPC(upload(pool, &sem, const_cast<uint16_t*>(p->codec_emb), (size_t)p->n_sem * H)); HIPC(upload(pool, &embs, const_cast<uint16_t*>(p->cp_embs), 15 * tab));
    HIPC(upload(pool, &tok, const_cast<uint32_t*>(p->tok), (size_t)B)); HIPC(upload(pool, &lg, const_cast<float*>(p->cp_logits_last), (size_t)B * V));
    HIPC(upload(pool, &codes, p->codes, n_codes)); HIPC(upload(pool, &fi, const_cast<int*>(p->frame_idx), (size_t)B));
    HIPC(upload(pool, &text, const_cast<float*>(p->text_rows), (size_t)p->n_text_rows * H));
    HIPC(upload(pool, &tb, const_cast<int*>(p->trail_base), (size_t)B)); HIPC(upload(pool, &tl, const_cast<int*>(p->trail_len), (size_t)B));
    HIPC(upload(pool, &pr, const_cast<int*>(p->pad_row), (size_t)B)); HIPC(upload(pool, &out, p->out, n_out));
    if (p->text_ready) HIPC(upload(pool, &rdy, const_cast<int*>(p->text_ready), (size_t)B));
    FrameEmbedArgs f{};
    f.codec_emb = sem; for (int g = 0; g < 15; ++g) f.cp_embs[g] = embs + (size_t)g * tab;
    f.tok = tok; f.cp_logits_last = lg; f.cp_vocab = V; f.codes = codes + G; f.frame_idx = fi; f.max_frames = MF;
    f.text_rows = text; f.trail_base = tb; f.trail_len = tl; f.pad_row = pr; f.out = out + G; f.H = H; f.B = B; f.n_acoustic = 15; f.text_ready = rdy;
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_frame_embed(f, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(p->codes, codes, n_codes * 4, hipMemcpyDeviceToHost));
    HIPC(q3_hipMemcpy(p->out, out, n_out * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_cp_gather_ex(int device, const q3_cp_gather_ex_args* p) {
    if (!p || !p->out) return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: null argument");
    const int B = p->B, H = p->H, V = p->cp_vocab, MF = p->max_frames, G = p->guard, pass = p->pass;
    if (pass < 0 || pass > 15 || B < 1 || B > 1024 || H < 1 || H > 8192 || G < 0 || G > 4096)
        return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: bad shape (pass 0..15, B 1..1024, H 1..8192, guard 0..4096)");
    const bool proj = pass >= 1 && p->proj_tab, qkv = pass >= 1 && p->qkv_tab;
    const int n_rows = pass == 1 ? p->n_sem : V, width = proj ? p->proj_dim : H;
    if (pass == 0 && !p->last_hidden) return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: pass 0 needs last_hidden");
    if (pass >= 1 && (n_rows < 1 || n_rows > 65536)) return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: table of %d rows", n_rows);
    if (pass == 1 && (!p->tok || (!proj && !p->codec_emb))) return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: pass 1 needs tok and a table");
    if (pass >= 2 && (!p->cp_logits || !p->codes || !p->frame_idx || (!proj && !p->cp_emb) || MF < 1 || MF > 4096))
        return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: pass >= 2 needs cp_logits, codes, frame_idx, a table and max_frames 1..4096");
    if (width < 1 || width > 8192 || p->ld_out < width) return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: ld_out %d below the row (%d)", p->ld_out, width);
    if (qkv && (!p->qkv_out || p->qkv_dim < 4 || p->qkv_dim > 16384 || p->qkv_dim % 4 || p->ld_qkv_out < p->qkv_dim || p->ld_qkv_out % 4 || G % 4))
        return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: qkv_tab needs qkv_out, qkv_dim a multiple of 4 (4..16384), ld_qkv_out >= qkv_dim, ld_qkv_out and guard multiples of 4");
    for (int b = 0; b < B; ++b) {
        if (pass == 1 && p->tok[b] >= (uint32_t)n_rows) return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: row %d: token %u outside the table", b, p->tok[b]);
        if (pass >= 2 && p->frame_idx[b] < 0) return set_err(Q3_INVALID_ARG, "q3_cp_gather_ex: row %d: frame_idx %d", b, p->frame_idx[b]);
    }
    HIPC(hipSetDevice(device));
    DevPool pool;
    const size_t n_out = (size_t)B * p->ld_out + 2 * (size_t)G, n_qkv = (size_t)B * p->ld_qkv_out + 2 * (size_t)G, n_codes = (size_t)B * MF * 16 + 2 * (size_t)G;
    float *out, *qo = nullptr, *lh = nullptr, *lg = nullptr, *pt = nullptr, *qt = nullptr; uint16_t* emb = nullptr; uint32_t *tok = nullptr, *codes = nullptr; int* fi = nullptr;
    HIPC(upload(pool, &out, p->out, n_out));
    if (pass == 0) HIPC(upload(pool, &lh, const_cast<float*>(p->last_hidden), (size_t)B * H));
    if (pass == 1) HIPC(upload(pool, &tok, const_cast<uint32_t*>(p->tok), (size_t)B));
    if (pass >= 1 && !proj) HIPC(upload(pool, &emb, const_cast<uint16_t*>(pass == 1 ? p->codec_emb : p->cp_emb), (size_t)n_rows * H));
    if (proj) HIPC(upload(pool, &pt, const_cast<float*>(p->proj_tab), (size_t)n_rows * p->proj_dim));
    if (qkv) { HIPC(upload(pool, &qt, const_cast<float*>(p->qkv_tab), (size_t)n_rows * p->qkv_dim)); HIPC(upload(pool, &qo, p->qkv_out, n_qkv)); }
    if (pass >= 2) {
        HIPC(upload(pool, &lg, const_cast<float*>(p->cp_logits), (size_t)B * V)); HIPC(upload(pool, &codes, p->codes, n_codes));
        HIPC(upload(pool, &fi, const_cast<int*>(p->frame_idx), (size_t)B));
    }
    CpGatherArgs a{};
    a.pass = pass; a.last_hidden = lh; a.H = H; a.codec_emb = pass == 1 ? emb : nullptr; a.tok = tok; a.cp_emb = pass >= 2 ? emb : nullptr; a.cp_logits = lg;
    a.cp_vocab = V; a.codes = codes ? codes + G : nullptr; a.frame_idx = fi; a.max_frames = MF; a.out = out + G; a.ld_out = p->ld_out;
    a.proj_tab = pt; a.proj_dim = proj ? p->proj_dim : 0; a.qkv_tab = qt; a.qkv_dim = qkv ? p->qkv_dim : 0; a.qkv_out = qo ? qo + G : nullptr;
    a.ld_qkv_out = p->ld_qkv_out; a.B = B;
    HIPC(q3_hipDeviceSynchronize());
    HIPC(launch_cp_gather(a, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(p->out, out, n_out * 4, hipMemcpyDeviceToHost));
    if (qo) HIPC(q3_hipMemcpy(p->qkv_out, qo, n_qkv * 4, hipMemcpyDeviceToHost));
    if (codes) HIPC(q3_hipMemcpy(p->codes, codes, n_codes * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}

extern "C" q3_status q3_rmsnorm_ex(int device, const float* x_host, long long x_elems, long long x_off, int ldx, const float* w_host, float* y_host,
                                   long long y_elems, long long y_front, int ldy, int rows, int cols, float eps, const int* frame_idx,
                                   const int* text_ready) {
    if (!x_host || !w_host || !y_host) return set_err(Q3_INVALID_ARG, "q3_rmsnorm_ex: null argument");
    if ((frame_idx == nullptr) != (text_ready == nullptr)) return set_err(Q3_INVALID_ARG, "q3_rmsnorm_ex: frame_idx and text_ready come together");
    const long long lim = 1LL << 28;
    if (rows < 1 || rows > 4096 || cols < 1 || cols > (1 << 16) || ldx < 1 || ldy < cols || x_off < 0 || y_front < 0 || x_elems < 1 || x_elems > lim ||
        y_elems < 1 || y_elems > lim || x_off + (long long)(rows - 1) * ldx + cols > x_elems || y_front + (long long)(rows - 1) * ldy + cols > y_elems)
        return set_err(Q3_INVALID_ARG, "q3_rmsnorm_ex: bad shape (rows 1..4096, cols 1..65536, ldx >= 1, ldy >= cols, every row inside its buffer)");
    HIPC(hipSetDevice(device));
    DevPool pool;
    float *x, *w, *y; int *fi = nullptr, *rdy = nullptr;
    HIPC(upload(pool, &x, const_cast<float*>(x_host), (size_t)x_elems)); HIPC(upload(pool, &w, const_cast<float*>(w_host), (size_t)cols));
    HIPC(upload(pool, &y, y_host, (size_t)y_elems));
    if (frame_idx) { HIPC(upload(pool, &fi, const_cast<int*>(frame_idx), (size_t)rows)); HIPC(upload(pool, &rdy, const_cast<int*>(text_ready), (size_t)rows)); }
    HIPC(q3_hipDeviceSynchronize());
    if (fi) HIPC(launch_rmsnorm_hold(x + x_off, ldx, w, y + y_front, ldy, rows, cols, eps, fi, rdy, 0));
    else HIPC(launch_rmsnorm(x + x_off, ldx, w, y + y_front, ldy, rows, cols, eps, 0));
    HIPC(q3_hipDeviceSynchronize());
    HIPC(q3_hipMemcpy(y_host, y, (size_t)y_elems * 4, hipMemcpyDeviceToHost));
    return Q3_OK;
}
