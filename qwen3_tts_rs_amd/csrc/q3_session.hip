// q3_session.hip — sessions: KV paging, talker / code-predictor step, frame capture and submission, prefill, generate, streaming, run / decode / get
// (one of the units of the engine: q3_engine.h says which holds what)
#include "q3_engine.h"
#include "q3_prefix_cache.h"

// Everything this session has in flight has landed: the frames on the library's own AQL queue (q3_aql.cpp; not ordered with any
// HIP stream) and whatever rides the session's stream. Every host-side wait of the engine goes through here.
hipError_t sync_frames(q3_session* s) {
    if (s->aql) {
        std::string why;
        if (!q3::aql_wait(s->aql, &why)) { s->aql_failed = true; set_err(Q3_HIP_ERROR, "AQL frame submission: %s", why.c_str()); return hipErrorUnknown; }
    }
    return hipStreamSynchronize(s->stream);
}

static hipError_t run_linear(q3_session* s, const LinArgs& a_in) {
    LinArgs a = a_in;
    a.ws = s->wide_ws; a.ws_bytes = s->wide_ws_bytes;
#ifdef Q3_TRACE
    a.trace = s->trace_next(0, a.M, a.N, a.K, a.epi, a.norm_w ? 1 : 0, a.tiled);
#endif
    if (!s->profile) return launch_linear(a, s->stream);
    // profiling: bracket the launch with event records (inside graph capture these become event-record
    // nodes, so the timestamps are taken on the GPU timeline without host launch latency in between)
    hipEvent_t e0, e1;
    if (s->prof_pool_next + 2 <= s->prof_pool.size()) { e0 = s->prof_pool[s->prof_pool_next++]; e1 = s->prof_pool[s->prof_pool_next++]; }
    else {
        hipError_t e = hipEventCreate(&e0); if (e != hipSuccess) return e;
        e = hipEventCreate(&e1); if (e != hipSuccess) return e;
        s->prof_pool.push_back(e0); s->prof_pool.push_back(e1); s->prof_pool_next = s->prof_pool.size();
    }
    hipError_t e = hipEventRecord(e0, s->stream); if (e != hipSuccess) return e;
    e = launch_linear(a, s->stream);
    hipError_t e2 = hipEventRecord(e1, s->stream);
    s->prof_events.push_back({e0, e1});
    s->prof_event_bytes.push_back((double)a.N * a.K * 2.0 * (a.epi == EPI_SWIGLU ? 2.0 : 1.0));
    {   // launch inventory (q3_session_profile_shapes): M, N, K, epilogue, fused input norm, reserved, tiling
        ProfShape ps{a.M, a.N, a.K, a.epi, a.norm_w ? 1 : 0, 0, a.ksplit == 2 ? 3 : a.tiled, 1};
        bool found = false;
        for (auto& q : s->prof_shapes)
            if (q.M == ps.M && q.N == ps.N && q.K == ps.K && q.epi == ps.epi && q.rms == ps.rms && q.produce == ps.produce && q.tiled == ps.tiled) { q.count += 1; found = true; break; }
        if (!found) s->prof_shapes.push_back(ps);
    }
    return e != hipSuccess ? e : e2;
}

// Paged KV bookkeeping (KvPool): row b gets the pages for positions [0, n_pos) it does not hold yet; the new table entries
// are queued on the session's stream ahead of the kernels that read them (hipMemcpyAsync stages pageable sources before it
// returns; kv_rows[b] never reallocates: reserved to KV_MAX_PAGES at creation).
q3_status kv_reserve_row(q3_session* s, int b, int n_pos) {
    if (!s->paged) return Q3_OK;
    if (n_pos > KV_MAX_PAGES * KV_PAGE_POS) return set_err(Q3_KV_OVERFLOW, "%d positions exceed a row's page table (%d)", n_pos, KV_MAX_PAGES * KV_PAGE_POS);
    std::vector<float*>& row = s->kv_rows[(size_t)b];
    const int need = (n_pos + KV_PAGE_POS - 1) / KV_PAGE_POS, have = (int)row.size();
    if (need <= have) return Q3_OK;
    KvPool& pool = s->kv_in_bf16 ? s->m->kv_pool16 : s->m->kv_pool;
    if (kv_take(s->m, pool, need - have, row) != hipSuccess)      // (reclaims pages only the prefix cache holds before it gives up)
    {
        s->kv_overflow_row = b;
        return set_err(Q3_KV_OVERFLOW, "KV page pool exhausted: row %d needs %d more %s page(s) of %d positions (budget: %ld of %ld half-pages in use)",
                       b, need - have, s->kv_in_bf16 ? "bf16" : "f32", KV_PAGE_POS, s->m->kv_budget.used, s->m->kv_budget.limit);
    }
    static_assert(sizeof(float*) == sizeof(unsigned long long), "page table entries are 64-bit pointers");
    HIPC(hipMemcpyAsync(s->kv_table + (size_t)b * KV_MAX_PAGES + have, row.data() + have, (size_t)(need - have) * 8, hipMemcpyHostToDevice, s->stream));
    return Q3_OK;
}
// pages for what the next `frames` frames of every row can touch: frame f of a row writes position prefill_len + f, a row
// that reached its limit keeps rewriting position prefill_len + limit (k_sample freezes its counters)
q3_status kv_reserve_frames(q3_session* s, int frames) {
    if (!s->paged) return Q3_OK;
    s->kv_overflow_row = -1;
    for (int b = 0; b < s->B; ++b) {
        const SeqInfo& q = s->seq[(size_t)b];
        if (q.idle) continue;
        int upto = (q.opened ? q.committed : s->frames_run - q.start_run) + frames;      // (a held row rewrites its current position)
        if (upto > q.limit) upto = q.limit;
        if (upto < 0) upto = 0;
        Q3C(kv_reserve_row(s, b, q.prefill_len + upto + 1));
    }
    return Q3_OK;
}
void kv_release_row(q3_session* s, int b) {        // the caller has drained every stream that may still touch the row
    if (s->paged && !s->kv_rows[(size_t)b].empty()) (s->kv_in_bf16 ? s->m->kv_pool16 : s->m->kv_pool).give(s->kv_rows[(size_t)b]);
}

// bf16 sessions: every row's f32 pages -> as many pages of the bf16 pool (k_kv_pages_to_bf16), the table rewritten, the f32
// pages returned (a page the prefix cache also holds stays the cache's: KvPool::give). The caller has drained the stream; this
// drains it again before the f32 pages go back.
static q3_status kv_convert_to_bf16(q3_session* s) {
    if (!s->paged) return set_err(Q3_UNSUPPORTED, "bf16 K/V needs the paged cache");
    const q3_config& c = s->m->cfg;
    std::vector<unsigned long long> src, dst; std::vector<std::vector<float*>> fresh((size_t)s->B);
    q3_status st = Q3_OK;
    for (int b = 0; b < s->B && st == Q3_OK; ++b) {
        const int n = (int)s->kv_rows[(size_t)b].size();
        if (kv_take(s->m, s->m->kv_pool16, n, fresh[(size_t)b]) != hipSuccess) { st = set_err(Q3_KV_OVERFLOW, "KV page pool (bf16) exhausted: row %d needs %d page(s)", b, n); break; }
        for (int i = 0; i < n; ++i) { src.push_back((unsigned long long)s->kv_rows[(size_t)b][(size_t)i]); dst.push_back((unsigned long long)fresh[(size_t)b][(size_t)i]); }
    }
    if (st != Q3_OK) { for (auto& f : fresh) if (!f.empty()) s->m->kv_pool16.give(f); return st; }
    const int n = (int)src.size();
    hipError_t e = hipMemcpyAsync(s->kv_conv, src.data(), (size_t)n * 8, hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s->kv_conv + (size_t)s->B * KV_MAX_PAGES, dst.data(), (size_t)n * 8, hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) e = launch_kv_pages_to_bf16(s->kv_conv, s->kv_conv + (size_t)s->B * KV_MAX_PAGES, n, c.n_layers, c.n_kv_heads, s->m->kv_pool.layer_stride(), s->m->kv_pool.v_delta(), s->stream);
    if (e == hipSuccess) e = sync_frames(s);
    if (e != hipSuccess) { for (auto& f : fresh) if (!f.empty()) s->m->kv_pool16.give(f); return set_err(Q3_HIP_ERROR, "K/V conversion to bf16: %s", hipGetErrorString(e)); }
    for (int b = 0; b < s->B; ++b) {
        s->m->kv_pool.give(s->kv_rows[(size_t)b]);
        s->kv_rows[(size_t)b].assign(fresh[(size_t)b].begin(), fresh[(size_t)b].end());
        if (!s->kv_rows[(size_t)b].empty())
            HIPC(hipMemcpyAsync(s->kv_table + (size_t)b * KV_MAX_PAGES, s->kv_rows[(size_t)b].data(), s->kv_rows[(size_t)b].size() * 8, hipMemcpyHostToDevice, s->stream));
    }
    HIPC(sync_frames(s));
    s->kv_in_bf16 = true;
    return Q3_OK;
}

// one DecoderLayer (transformer.rs:442-467) for the single new token of every sequence
q3_status lm_layer(q3_session* s, const LmDims& d, const LayerW& w, LmBuf& b, float* kc, float* vc, int max_seq,
                   const int* pos_dev, int pos_static, int n_splits, int rows_per_seq, bool skip_qkv,
                   const CpGatherArgs* fold,         // fold: this layer's attention does the pass's gather
                   int paged_layer) {                // >= 0: the talker's paged cache, this layer's index (kc / vc / max_seq unused)
    const q3_model* m = s->m;
    // B = number of activation ROWS of this step: one per sequence, or rows_per_seq consecutive positions per
    // sequence (chunked prefill, the code predictor's 2-token first pass)
    const int QD = d.nh * HEAD_DIM, KD = d.nkv * HEAD_DIM, B = s->B * rows_per_seq;
    LinArgs a;
    a.N = QD + 2 * KD; a.K = d.H; set_w(a, w.qkv, B, a.N, a.K); a.x = b.X; a.ldx = d.H; a.norm_w = w.in_ln; a.eps = d.eps;
    a.y = b.QKV; a.ldy = QD + 2 * KD; a.M = B; a.epi = EPI_NONE;
    // Wide sessions: the q|k|v GEMM hands its K-slice sums straight to the attention kernel, which adds them on the 3 x 128
    // values it needs (AttnArgs::qkv_part) — the slice-sum launch in between (93 per frame at 1.7B, 5.2 us + gap each) is gone.
    // Only for the one-launch decode attention (static one-row steps); Q3_WIDE_NO_QKV_FUSE=1: off (A/B aid)
    static const bool qkv_fuse = getenv("Q3_WIDE_NO_QKV_FUSE") == nullptr;
    WidePartial wp{nullptr, nullptr, 0};
    if (!skip_qkv) {       // skip: the caller already filled b.QKV (code predictor layer 0, table rows)
        bool fused = false;
        if (qkv_fuse && B >= gemm_wide_min_rows() && rows_per_seq == 1 && !s->legacy_attn && !s->profile && !s->debug && s->wide_ws) {
            LinArgs a2 = a; a2.ws = s->wide_ws; a2.ws_bytes = s->wide_ws_bytes;
            const hipError_t e = launch_gemm_wide_partial(a2, s->stream, &wp);
            if (e == hipSuccess && wp.S <= 8) fused = true;
            else if (e != hipSuccess && e != hipErrorNotSupported) HIPC(e);
            else if (e == hipSuccess) { wp = WidePartial{nullptr, nullptr, 0}; }       // more than eight slices: let the slice-sum launch redo it
        }
        if (!fused) { wp = WidePartial{nullptr, nullptr, 0}; HIPC(run_linear(s, a)); }
    }
    AttnArgs t{};
    t.qkv = b.QKV; t.ld_qkv = QD + 2 * KD; t.q_norm_w = w.q_norm; t.k_norm_w = w.k_norm; t.eps = d.eps;
    t.rope_cos = m->rope_cos; t.rope_sin = m->rope_sin; t.pos_dev = pos_dev; t.pos_static = pos_static;
    t.kcache = kc; t.vcache = vc; t.max_seq = max_seq; t.qbuf = b.Q; t.part = b.PART; t.out = b.ATT; t.ld_out = QD;
    t.B = B; t.nh = d.nh; t.nkv = d.nkv; t.n_splits = n_splits; t.rows_per_seq = rows_per_seq;
    if (paged_layer >= 0) {
        t.kv_pages = s->kv_table; t.kv_layer_off = (size_t)paged_layer * s->m->kv_pool.layer_stride();
        t.kv_vdelta = s->m->kv_pool.v_delta();
        t.kv_row_pages = (max_seq + KV_PAGE_POS - 1) / KV_PAGE_POS;
        t.kv_bf16 = s->kv_in_bf16 ? 1 : 0;
    }
    if (wp.part) { t.qkv_part = wp.part; t.qkv_ssq = wp.ssq; t.qkv_S = wp.S; t.qkv_K = d.H; t.qkv_eps = d.eps; }
    // Split-K projections (LinArgs::ksplit, k_gemv_sk2): o-proj and down-proj with N <= 2048 and K >= 2048 at 3 .. 16 rows (wide
    // sessions: blocks of 16 rows, see below)
    // run as two K halves that meet in the output through order-independent atomic adds. The output buffer must hold zeros:
    // SUM is cleared by this layer's attention launch (its last reader was the previous down-proj), X by the gate/up
    // launch (its last reader is this layer's o-proj, as the residual).
    const bool first2 = !s->legacy_attn && rows_per_seq == 2 && !pos_dev && pos_static == 0 && paged_layer < 0;
    const bool attn3 = !first2 && (s->legacy_attn || rows_per_seq > 1);
    // Wide sessions (B > 16, round 3): the same kernel over blocks of 16 rows (grid plane z) — one launch instead of the
    // split-K GEMM + slice-sum pair for exactly the narrow outputs where the second launch hurt most (B = 64, code
    // predictor o / down: 9.4 + 4.9 us -> one launch). Q3_WIDE_NO_SK2=1: off (A/B aid)
    static const bool wide_sk2 = getenv("Q3_WIDE_NO_SK2") == nullptr;
    const bool sk_rows = s->ksplit && B >= 3 && (B <= 16 || (wide_sk2 && B <= Q3_MAX_BATCH && rows_per_seq == 1)) && d.H <= 2048 && d.H % 4 == 0;
    // (round 6: also behind the code predictor's 2-token first pass — 16 rows at B = 8 — whose o-projection ran on k_gemv_lds with
    // 64 workgroups: 5.8 us against 3.6 as two K halves; Q3_FIRST2_NO_SK=1: the old kernel, A/B aid)
    static const bool first2_sk = getenv("Q3_FIRST2_NO_SK") == nullptr;
    const bool o_sk = sk_rows && (!first2 || first2_sk) && !attn3 && w.o.t1 && QD >= 2048 && up32(QD) / 32 >= 16;
    // (beyond 32 rows the 25 MB talker down-proj is re-read by every 16-row block — 32.0 us at B = 64 against 16.5 + 4.8 for
    // the GEMM pair — while the smaller matrices win: code predictor o 14.6 -> 6.8, down 15.7 -> 9.2, talker o 14.4 -> 11.7 us)
    const bool dn_big = B > 32 && (size_t)d.I * d.H * 2 > ((size_t)12 << 20);
    const bool dn_sk = sk_rows && !dn_big && w.down.t1 && w.gate.t1 && d.I >= 2048 && up32(d.I) / 32 >= 16;
    if (t.kv_bf16 && (first2 || attn3)) return set_err(Q3_UNSUPPORTED, "multi-row talker steps are not available once a session's K/V is bf16");
    if (first2) {
        if (fold) {                                 // pass-1 gather folded: row 2b+1 = table row tok[b]
            t.g_tok = fold->tok; t.g_qkv_tab = fold->qkv_tab; t.g_proj_tab = fold->proj_tab; t.g_proj_dim = fold->proj_dim;
            t.g_x = fold->out; t.g_ldx = fold->ld_out;
        }
        if (o_sk) { t.zero = b.SUM; t.zero_n = B * d.H; }
        HIPC(launch_attn_first2(t, s->stream));    // the code predictor's 2-token first pass
    } else if (attn3) {     // rows of one sequence depend on each other's K/V: three launches
        HIPC(launch_qknorm_rope_kv(t, s->stream));
        HIPC(launch_attn_decode(t, s->stream));
        HIPC(launch_attn_merge(t, s->stream));
    } else {
        if (fold) {
            t.g_logits = fold->cp_logits; t.g_vocab = fold->cp_vocab; t.g_qkv_tab = fold->qkv_tab;
            t.g_proj_tab = fold->proj_tab; t.g_proj_dim = fold->proj_dim; t.g_x = fold->out; t.g_ldx = fold->ld_out;
            t.g_codes = fold->codes; t.g_frame_idx = fold->frame_idx; t.g_max_frames = fold->max_frames; t.g_code_slot = fold->pass - 1;
        }
        if (o_sk) { t.zero = b.SUM; t.zero_n = B * d.H; }
        if (s->cp_attn && attn_cp_ok(t)) {      // <= 16 positions, static position: the code predictor
#ifdef Q3_TRACE
            t.trace = s->trace_next(1, t.B, t.nh, 1, t.pos_static, t.g_logits ? 1 : 0);
#endif
            HIPC(launch_attn_cp(t, s->stream));
        } else {
#ifdef Q3_TRACE
            t.trace = s->trace_next(2, t.B, t.nh, n_splits, t.pos_static, t.g_logits ? 1 : 0);
#endif
            HIPC(launch_attn_fused(t, s->stream));
#ifdef Q3_TRACE
            if (n_splits > 1) t.trace = s->trace_next(3, t.B, t.nh, n_splits, t.pos_static);
#endif
            if (n_splits > 1) HIPC(launch_attn_merge(t, s->stream));
        }
    }
    auto force16 = [&](LinArgs& l, const TW& tw) { l.tiled = 1; l.W = tw.t1; l.Kpad = kpad_for(1, l.K); l.ksplit = 2; };
    LinArgs o;
    o.N = d.H; o.K = QD; set_w(o, w.o, B, o.N, o.K); o.x = b.ATT; o.ldx = QD; o.resid = b.X; o.ldr = d.H; o.y = b.SUM; o.ldy = d.H; o.M = B; o.epi = EPI_RESID;
    if (o_sk) force16(o, w.o);
    HIPC(run_linear(s, o));
    LinArgs g;
    g.N = d.I; g.K = d.H; set_w2(g, w.gate, w.up, B, g.N, g.K); g.x = b.SUM; g.ldx = d.H; g.norm_w = w.post_ln; g.eps = d.eps;
    g.y = b.ACT; g.ldy = d.I; g.M = B; g.epi = EPI_SWIGLU;
    if (dn_sk) { g.zero = b.X; g.zero_n = B * d.H; }
    HIPC(run_linear(s, g));
    LinArgs dn;
    dn.N = d.H; dn.K = d.I; set_w(dn, w.down, B, dn.N, dn.K); dn.x = b.ACT; dn.ldx = d.I; dn.resid = b.SUM; dn.ldr = d.H; dn.y = b.X; dn.ldy = d.H; dn.M = B; dn.epi = EPI_RESID;
    if (dn_sk) force16(dn, w.down);
    HIPC(run_linear(s, dn));
    return Q3_OK;
}

static bool d_nh_ok(const q3_config& c) {     // GEMM prefill needs N % 64 == 0 for every projection and a 1- or 2-way GQA ratio
    const int qkv = (c.n_heads + 2 * c.n_kv_heads) * HEAD_DIM, rep = c.n_heads / (c.n_kv_heads ? c.n_kv_heads : 1);
    return qkv % 64 == 0 && c.hidden % 64 == 0 && c.inter % 64 == 0 && (rep == 1 || rep == 2);
}
LmDims talker_dims(const q3_config& c) { return LmDims{c.hidden, c.inter, c.n_heads, c.n_kv_heads, c.n_layers, c.rms_eps}; }
LmDims cp_dims(const q3_config& c) { return LmDims{c.cp_hidden, c.cp_inter, c.cp_heads, c.cp_kv_heads, c.cp_layers, c.rms_eps}; }

// talker layers on the contents of tb.X at position pos (device array or static); with_head: final
// norm → LASTH and codec_head → LOGITS (talker.rs:716-736)
q3_status talker_step(q3_session* s, const int* pos_dev, int pos_static, bool with_head, int rows_per_seq, const int* text_ready) {
    const q3_model* m = s->m; const q3_config& c = m->cfg;
    const LmDims d = talker_dims(c);
    for (int i = 0; i < c.n_layers; ++i)
        Q3C(lm_layer(s, d, m->tl[i], s->tb, s->paged ? nullptr : s->kcache + (size_t)i * s->kv_layer_stride,
                     s->paged ? nullptr : s->vcache + (size_t)i * s->kv_layer_stride,
                     s->max_seq, pos_dev, pos_static, s->n_splits, rows_per_seq, false, nullptr, s->paged ? i : -1));
    if (with_head) {
        // final norm of each sequence's LAST row of the step (a frame with open text rows: held rows keep their LASTH)
        if (text_ready)
            HIPC(launch_rmsnorm_hold(s->tb.X + (size_t)(rows_per_seq - 1) * c.hidden, rows_per_seq * c.hidden, m->norm, s->LASTH, c.hidden, s->B,
                                     c.hidden, c.rms_eps, s->frame_idx, text_ready, s->stream));
        else
        HIPC(launch_rmsnorm(s->tb.X + (size_t)(rows_per_seq - 1) * c.hidden, rows_per_seq * c.hidden, m->norm, s->LASTH, c.hidden, s->B,
                            c.hidden, c.rms_eps, s->stream));
        LinArgs h;
        h.N = c.codec_vocab; h.K = c.hidden; set_w(h, m->codec_head, s->B, h.N, h.K); h.x = s->LASTH; h.ldx = c.hidden; h.y = s->LOGITS; h.ldy = c.codec_vocab;
        h.M = s->B; h.epi = EPI_NONE;
        HIPC(run_linear(s, h));
    }
    return Q3_OK;
}

// generate_acoustic_codes (code_predictor.rs:320-416) as 16 single-token passes: pass 0 = talker
// hidden (pos 0), pass 1 = semantic embedding (pos 1) → lm_head[0]; pass p = embedding of code p-2
// (pos p) → lm_head[p-1]. (The reference runs passes 0 and 1 as one 2-token causal prefill; for
// causal attention that is the same computation.) Codes 0..13 are recorded by the next pass's
// gather, code 14 by frame_embed / the caller.
static q3_status cp_run(q3_session* s) {
    const q3_model* m = s->m; const q3_config& c = m->cfg;
    const LmDims d = cp_dims(c);
    const int H = c.hidden, CH = c.cp_hidden, V = c.cp_vocab, B = s->B;
    const int n_pass = c.n_groups;   // 16
    // First pass as the reference does it (code_predictor.rs:337-367): the talker hidden state and the semantic
    // embedding go through the layers TOGETHER as a 2-token causal prefill (rows 2b, 2b+1), when 2B rows fit.
    const bool two = !s->no_chunk && 2 * B <= 16;
    for (int p = two ? 1 : 0; p < n_pass; ++p) {
        const int rows = (two && p == 1) ? 2 : 1;
        CpGatherArgs g{};
        g.pass = p; g.last_hidden = s->LASTH; g.H = H; g.codec_emb = m->codec_emb; g.tok = s->tok;
        g.cp_emb = p >= 2 ? m->cp_emb[p - 2] : nullptr;
        g.cp_logits = p >= 2 ? s->CP_LOGITS + (size_t)(p - 2) * B * V : nullptr;
        g.cp_vocab = V; g.codes = s->codes; g.frame_idx = s->frame_idx; g.max_frames = s->max_frames; g.B = B;
        float* dst = m->mtp_w.t1 ? s->CP_IN : s->cb.X; const int ld = m->mtp_w.t1 ? H : CH;
        // 1.7B with pre-projected tables: only the talker hidden state (pass 0) still goes through the 2048 -> 1024
        // projection at run time; every embedding row arrives already projected (14 GEMV launches less per frame)
        const bool tabs = m->mtp_w.t1 && m->proj_tabs && s->proj_tables;
        auto project = [&](int M, int ldy, const float* x_in = nullptr) -> q3_status {
            LinArgs a;
            a.N = CH; a.K = H; set_w(a, m->mtp_w, M, CH, H); a.x = x_in ? x_in : s->CP_IN; a.ldx = H; a.bias = m->mtp_b; a.y = s->cb.X; a.ldy = ldy;
            a.M = M; a.epi = EPI_NONE;
            HIPC(run_linear(s, a));
            return Q3_OK;
        };
        // layer-0 q|k|v of a table row comes from the table too (both model sizes): the layer-0 qkv GEMV then only runs
        // for the rows that carry the talker hidden state
        const bool qt = m->qkv0_tabs && s->qkv_tables && (tabs || !m->mtp_w.t1);
        const int QKVD = (d.nh + 2 * d.nkv) * HEAD_DIM;
        bool skip0 = false, fold0 = false;
        auto qkv_rows0 = [&](int ldx, int ldy) -> q3_status {      // run-time layer-0 qkv of the B pass-0 rows
            LinArgs a;
            a.N = QKVD; a.K = CH; set_w(a, m->cl[0].qkv, B, QKVD, CH); a.x = s->cb.X; a.ldx = ldx; a.norm_w = m->cl[0].in_ln; a.eps = d.eps;
            a.y = s->cb.QKV; a.ldy = ldy; a.M = B; a.epi = EPI_NONE;
            HIPC(run_linear(s, a));
            return Q3_OK;
        };
        if (tabs) {
            if (rows == 2) {
                // B rows of talker hidden: projected straight from LASTH (the copy to CP_IN was a launch of its own)
                static const bool no_fold2 = getenv("Q3_CP_NO_FOLD") != nullptr;
                if (no_fold2) { g.pass = 0; g.out = s->CP_IN; g.ld_out = H; HIPC(launch_cp_gather(g, s->stream)); }
                Q3C(project(B, 2 * CH, no_fold2 ? s->CP_IN : s->LASTH));           // -> cb.X rows 2b
                g.pass = 1; g.out = s->cb.X + CH; g.ld_out = 2 * CH; g.proj_tab = m->sem_proj; g.proj_dim = CH;   // rows 2b+1
                if (qt) { g.qkv_tab = m->sem_qkv0; g.qkv_dim = QKVD; g.qkv_out = s->cb.QKV + QKVD; g.ld_qkv_out = 2 * QKVD; }
                // the semantic row (table row tok[b]) is read by the 2-token attention itself
                fold0 = qt && !s->legacy_attn && !no_fold2 && CH % 4 == 0;
                if (!fold0) HIPC(launch_cp_gather(g, s->stream));
                if (qt) { Q3C(qkv_rows0(2 * CH, 2 * QKVD)); skip0 = true; }
            } else if (p == 0) {
                g.out = s->CP_IN; g.ld_out = H;
                HIPC(launch_cp_gather(g, s->stream));
                Q3C(project(B, CH));
            } else {
                g.out = s->cb.X; g.ld_out = CH; g.proj_tab = p == 1 ? m->sem_proj : m->cp_proj[p - 2]; g.proj_dim = CH;
                if (qt) { g.qkv_tab = p == 1 ? m->sem_qkv0 : m->cp_qkv0[p - 2]; g.qkv_dim = QKVD; g.qkv_out = s->cb.QKV; g.ld_qkv_out = QKVD; skip0 = true; }
                // passes >= 2 with both tables: no launch of its own — the layer-0 attention re-derives the argmax and
                // reads the table rows itself (14 launches less per frame; Q3_CP_NO_FOLD=1: the separate launch, A/B aid)
                static const bool no_fold = getenv("Q3_CP_NO_FOLD") != nullptr;
                fold0 = qt && p >= 2 && !s->legacy_attn && !no_fold && CH % 4 == 0;
                if (!fold0) HIPC(launch_cp_gather(g, s->stream));
            }
        } else {
        if (rows == 2) {
            // row 2b = talker hidden (pass-0 source), row 2b+1 = semantic embedding (pass-1 source)
            g.pass = 0; g.out = dst; g.ld_out = 2 * ld;
            HIPC(launch_cp_gather(g, s->stream));
            g.pass = 1; g.out = dst + ld;
            if (qt) { g.qkv_tab = m->sem_qkv0; g.qkv_dim = QKVD; g.qkv_out = s->cb.QKV + QKVD; g.ld_qkv_out = 2 * QKVD; }
            HIPC(launch_cp_gather(g, s->stream));
            if (qt) { Q3C(qkv_rows0(2 * CH, 2 * QKVD)); skip0 = true; }
        } else {
            g.out = dst; g.ld_out = ld;
            if (qt && p >= 1) { g.qkv_tab = p == 1 ? m->sem_qkv0 : m->cp_qkv0[p - 2]; g.qkv_dim = QKVD; g.qkv_out = s->cb.QKV; g.ld_qkv_out = QKVD; skip0 = true; }
            HIPC(launch_cp_gather(g, s->stream));
        }
        if (m->mtp_w.t1) Q3C(project(B * rows, CH));
        }
        for (int i = 0; i < c.cp_layers; ++i)
            Q3C(lm_layer(s, d, m->cl[i], s->cb, s->ckcache + (size_t)i * s->ckv_layer_stride, s->cvcache + (size_t)i * s->ckv_layer_stride,
                         n_pass + 1, nullptr, rows == 2 ? 0 : p, 1, rows, i == 0 && skip0, (i == 0 && fold0) ? &g : nullptr));
        if (p >= 1) {
            LinArgs h;
            h.N = V; h.K = CH; set_w(h, m->cp_head[p - 1], B, V, CH); h.x = s->cb.X + (size_t)(rows - 1) * CH; h.ldx = rows * CH;
            h.norm_w = m->cp_norm; h.eps = c.rms_eps;
            h.y = s->CP_LOGITS + (size_t)(p - 1) * B * V; h.ldy = V; h.M = B; h.epi = EPI_NONE;
            HIPC(run_linear(s, h));
        }
    }
    return Q3_OK;
}

// sampling options of one request -> the sampler's per-row record (sampling.rs:140-319 branch conditions)
SampleRow sample_row(const q3_options& o) {
    SampleRow r{};
    r.apply_temp = (o.temperature != 1.0 && o.temperature > 0.0) ? 1 : 0;
    r.inv_temp = (float)(1.0 / o.temperature);
    r.greedy = o.temperature < 0.01 ? 1 : 0;
    r.top_k = o.top_k; r.use_top_p = (o.top_p < 1.0 && o.top_p > 0.0) ? 1 : 0; r.top_p = (float)o.top_p;
    r.use_rep = (o.repetition_penalty != 1.0 && !(fabs(o.repetition_penalty - 1.0) < 1e-9)) ? 1 : 0;
    r.rep_pen = (float)o.repetition_penalty; r.rep_inv = 1.0f / (float)o.repetition_penalty;
    r.eos_id = o.eos_token_id; r.min_new_tokens = o.min_new_tokens;
    return r;
}

static void fill_sample_args(q3_session* s, SampleArgs& a) {
    const q3_config& c = s->m->cfg;
    memset(&a, 0, sizeof a);
    a.logits = s->LOGITS; a.ld = c.codec_vocab; a.seen = s->seen; a.u = s->U; a.u_stride = s->max_frames + 2; a.limit = s->limit;
    a.draw_idx = s->token_count; a.tok = s->tok; a.token_count = s->token_count; a.frame_idx = s->frame_idx; a.pos = s->pos;
    a.vocab = c.codec_vocab; a.B = s->B;
    const SampleRow r = sample_row(s->opts);          // scalar fields = the first request's (every row reads its own through a.rows)
    a.apply_temp = r.apply_temp; a.inv_temp = r.inv_temp; a.greedy = r.greedy; a.top_k = r.top_k; a.use_top_p = r.use_top_p; a.top_p = r.top_p;
    a.use_rep = r.use_rep; a.rep_pen = r.rep_pen; a.rep_inv = r.rep_inv; a.eos_id = r.eos_id; a.min_new_tokens = r.min_new_tokens;
    a.rows = s->sample_rows;
    a.codec_eos = CODEC_EOS; a.use_suppress = 1;
    if (s->debug && s->logits_hist) { a.logits_hist = s->logits_hist; a.hist_stride_b = (s->max_frames + 1) * c.codec_vocab; a.hist_cap = s->max_frames + 1; }
}

// one frame of generate_codes (lib.rs:580-652)
static q3_status frame_launch(q3_session* s) {
    const q3_model* m = s->m; const q3_config& c = m->cfg;
#ifdef Q3_TRACE
    s->trace_node = 0; s->trace_meta.clear();        // every frame (and the capture) re-uses the same slices
#endif
    Q3C(cp_run(s));
    FrameEmbedArgs f{};
    f.codec_emb = m->codec_emb; f.tok = s->tok;
    for (int g = 0; g < 15; ++g) f.cp_embs[g] = g < (int)m->cp_emb.size() ? m->cp_emb[(size_t)g] : nullptr;
    f.cp_logits_last = s->CP_LOGITS + (size_t)14 * s->B * c.cp_vocab; f.cp_vocab = c.cp_vocab;
    f.codes = s->codes; f.frame_idx = s->frame_idx; f.max_frames = s->max_frames;
    f.text_rows = s->rows; f.trail_base = s->trail_base; f.trail_len = s->trail_len; f.pad_row = s->pad_row;
    f.out = s->tb.X; f.H = c.hidden; f.B = s->B; f.n_acoustic = c.n_groups - 1;
    f.text_ready = s->text_ready;            // null unless a row was opened
    HIPC(launch_frame_embed(f, s->stream));
    if (s->debug && s->cp_logits_hist) {
        // capture is host-indexed: only valid outside graph replay (debug sessions never use graphs)
        HIPC(hipMemcpyAsync(s->cp_logits_hist + (size_t)s->frames_run * 15 * s->B * c.cp_vocab, s->CP_LOGITS,
                            (size_t)15 * s->B * c.cp_vocab * 4, hipMemcpyDeviceToDevice, s->stream));
    }
    Q3C(talker_step(s, s->pos, 0, true, 1, s->text_ready));
    SampleArgs a; fill_sample_args(s, a); a.advance = 1; a.text_ready = s->text_ready;
    HIPC(launch_sample(a, s->stream));
    return Q3_OK;
}


// ---- prompt layout (DESIGN "Prompt layout"): the one description of how a request becomes a prompt ----
// the ICL length cap in frames over a text of n_text tokens (lib.rs:913-929)
int icl_frame_cap(int n_text) { return std::max(75, 6 * n_text); }
// Projected text rows of a request: [instruct…, im_start, assistant, newline, tts_pad, tts_bos, (ICL: ref_text…,) text…, tts_eos].
// Prefill positions (talker.rs:451-491 CustomVoice / 511-564 voice clone / 585-627 VoiceDesign): instruct, role x 3, the codec
// overlay over tts_pad… tts_bos, then the first text token — or, ICL, the block of n_ref + 1 positions that pairs
// [ref_text, text, tts_eos] (tts_pad once that runs out) with codec_bos and the reference frames (the streaming overlay,
// talker.rs:646-710). What the prefill does not consume is the trailing text (lib.rs:508-519; ICL: talker.rs:692-708).
PromptShape prompt_shape(const q3_request& r, int n_text) {
    PromptShape p{};
    const bool vd = r.mode == Q3_MODE_VOICE_DESIGN;
    p.icl = r.mode == Q3_MODE_VOICE_CLONE && r.n_ref > 0 && r.ref_codes && r.ref_text_ids;
    p.n_ins = vd ? r.n_instruct : 0;
    p.n_ref_text = p.icl ? r.n_ref_text : 0;
    p.n_icl = p.icl ? r.n_ref + 1 : 0;                  // streaming overlay: icl_len = n_codec
    p.overlay = vd ? 5 : 6;                             // think, think_bos, language, think_eos, (speaker | x-vector,) pad; codec_bos follows
    p.prefill_len = p.n_ins + 3 + p.overlay + ((n_text > 0 && !p.icl) ? 1 : 0) + p.n_icl;
    p.n_rows = p.n_ins + 5 + p.n_ref_text + n_text + 1;
    const int n_all = p.n_ref_text + n_text;            // ICL: [ref_text, text], + tts_eos once closed
    p.n_trail = p.icl ? std::max(n_all - p.n_icl, 0) : std::max(n_text - 1, 0);
    p.trailing_len = p.icl ? std::max(n_all + 1 - p.n_icl, 1) : p.n_trail + 1;
    p.limit = p.icl ? std::min(r.opts.max_length, icl_frame_cap(n_text)) : r.opts.max_length;
    p.open_need = p.icl ? std::max(p.n_icl - p.n_ref_text, 1) : 1;      // tts_eos must fall after the ICL block
    p.prefix_pages = vd ? r.n_instruct / KV_PAGE_POS : 0;      // the instruct positions, in whole pages (q3_prefix_cache.h)
    p.r_role = p.n_ins; p.r_pad = p.r_role + 3; p.r_bos = p.r_pad + 1; p.r_text = p.r_bos + 1; p.r_eos = p.r_text + n_all;
    if (p.icl) p.trail_base = n_all + 1 > p.n_icl ? p.r_text + p.n_icl : p.r_pad;
    else p.trail_base = n_text > 1 ? p.r_text + 1 : p.r_eos;
    return p;
}
void prompt_positions(const PromptShape& sh, const q3_request& r, int row_base, int* tr, int* ci) {
    const int codec[7] = {CODEC_THINK, CODEC_THINK_BOS, (int)r.language_id, CODEC_THINK_EOS,
                          r.mode == Q3_MODE_VOICE_CLONE ? -2 : (int)r.speaker_id, CODEC_PAD, CODEC_BOS};
    int p = 0;
    for (int i = 0; i < sh.n_ins + 3; ++i) { tr[p] = row_base + i; ci[p] = -1; ++p; }      // instruct, role: text alone
    for (int i = 0; i < sh.overlay; ++i) {
        tr[p] = row_base + (i == sh.overlay - 1 ? sh.r_bos : sh.r_pad);
        ci[p] = codec[i < 4 || sh.overlay == 6 ? i : i + 1];      // VoiceDesign has no speaker position
        ++p;
    }
    if (p + sh.n_icl < sh.prefill_len) { tr[p] = row_base + sh.r_text; ci[p] = CODEC_BOS; ++p; }      // the first text token (not ICL)
    const int n_text_all = sh.r_eos + 1 - sh.r_text;      // [ref_text, text, tts_eos]
    for (int i = 0; i < sh.n_icl; ++i) {      // ICL block: text (or tts_pad) row + codec_bos / Σ16 reference-frame embeddings
        tr[p] = row_base + (i < n_text_all ? sh.r_text + i : sh.r_pad);
        ci[p] = i == 0 ? CODEC_BOS : -3 - (i - 1);
        ++p;
    }
}
// worst-case cost of a row against the model's KV budget (KvBudget units): every page prompt + limit + 1 positions can reach; a
// bf16 row holds f32 pages for its prompt and, while they are converted, bf16 pages beside them
long row_worst_units(int prefill_len, int limit, bool bf16) {
    const long full = (prefill_len + limit + 1 + KV_PAGE_POS - 1) / KV_PAGE_POS, pre = (prefill_len + 1 + KV_PAGE_POS - 1) / KV_PAGE_POS;
    return bf16 ? std::max(3 * pre, full) : 2 * full;
}
// a request that only occupies a row: a one-token CustomVoice prompt with a one-frame limit, built from fixed, known-valid values
// (ten prefill positions). Rows of the batcher's session before a ticket enters them; rows of a ragged first batch before prefill.
q3_request idle_request(int chunk_frames) {
    static const uint32_t one_tok[1] = {0};
    q3_request d{};
    d.mode = Q3_MODE_CUSTOM_VOICE; d.text_ids = one_tok; d.n_text = 1;
    d.speaker_id = 0; d.language_id = 0;                                       // codec token 0: valid in every vocabulary
    d.opts.temperature = 0.9; d.opts.top_p = 0.9; d.opts.repetition_penalty = 1.05; d.opts.top_k = 50;      // SynthesisOptions::default (lib.rs:1786-1836)
    d.opts.eos_token_id = -1; d.opts.min_new_tokens = 2; d.opts.max_length = 1; d.opts.has_seed = 1; d.opts.seed = 0;
    d.opts.chunk_frames = chunk_frames;
    return d;
}
// Sessions take rows of ANY mix of prompt kinds and lengths (round 5; BASELINE config[3] on a Base checkpoint mixes x-vector and
// ICL prompts, lib.rs:718-784, 802-870, 897-1046 are per-call in the reference). Rows of one prefill length are prefilled
// together by the session itself (the fast path: one batched prefill). A RAGGED batch is opened on idle rows sized for the
// longest prompt / largest limit; q3_session_prefill then prefills the rows in groups of equal prefill length — each group a
// batched side prefill — and moves every row in the way a continuous-batching swap does (transplant_row), so every row carries
// the bits of its own run and decode proceeds in one captured frame graph over all rows.
static q3_status session_create_any(q3_model* m, const q3_request* reqs, int batch, int frame_budget, int prompt_budget, q3_session** out) {
    if (!m || !reqs || !out) return set_err(Q3_INVALID_ARG, "q3_session_create: null argument");
    if (batch < 1 || batch > Q3_MAX_BATCH) return set_err(Q3_UNSUPPORTED, "batch %d unsupported (1..%d sequences per session)", batch, Q3_MAX_BATCH);
    bool ragged = false; int S0 = 0, Smax = 0, Lmax = 0, rows_max = 0;
    for (int b = 0; b < batch; ++b) {
        const q3_request& r = reqs[b];
        if (r.n_text < 0 || r.n_instruct < 0 || r.n_ref < 0 || r.n_ref_text < 0) return set_err(Q3_INVALID_ARG, "bad token id arrays");
        const PromptShape sh = prompt_shape(r);
        if (b == 0) S0 = sh.prefill_len;
        ragged = ragged || sh.prefill_len != S0;
        Smax = std::max(Smax, sh.prefill_len); Lmax = std::max(Lmax, sh.limit);
        rows_max = std::max(rows_max, sh.n_rows);
        if (r.opts.chunk_frames != reqs[0].opts.chunk_frames) return set_err(Q3_UNSUPPORTED, "all requests of a batch must share chunk_frames (the streaming chunk is a property of the session)");
    }
    if (!ragged) return session_create(m, reqs, batch, frame_budget, prompt_budget, out);
    if (Lmax < 1) return set_err(Q3_INVALID_ARG, "max_length must be >= 1");
    const int fb = std::max(frame_budget, Lmax);
    int pb = std::max(std::max(prompt_budget, Smax), 16);
    if (rows_max > pb + 1024) pb = rows_max - 1024;          // a row's text-row slot is prompt_budget + 1024 rows
    std::vector<q3_request> idle((size_t)batch, idle_request(reqs[0].opts.chunk_frames));
    q3_session* s = nullptr;
    Q3C(session_create(m, idle.data(), batch, fb, pb, &s));
    s->ragged.resize((size_t)batch);
    for (int b = 0; b < batch; ++b) s->ragged[(size_t)b].own(reqs[b], m->cfg.hidden);
    *out = s;
    return Q3_OK;
}
extern "C" q3_status q3_session_create(q3_model* m, const q3_request* reqs, int batch, q3_session** out) {
    return session_create_any(m, reqs, batch, 0, 0, out);
}
extern "C" q3_status q3_session_create_reserved(q3_model* m, const q3_request* reqs, int batch, int frame_budget, int prompt_budget, q3_session** out) {
    if (frame_budget < 0 || prompt_budget < 0) return set_err(Q3_INVALID_ARG, "q3_session_create_reserved: negative budget");
    return session_create_any(m, reqs, batch, frame_budget, prompt_budget, out);
}
q3_status session_create(q3_model* m, const q3_request* reqs, int batch, int frame_budget, int prompt_budget, q3_session** out,
                                hipStream_t borrow) {
    if (!m || !reqs || !out) return set_err(Q3_INVALID_ARG, "q3_session_create: null argument");
    if (!m->finalized) return set_err(Q3_INVALID_ARG, "model not finalized");
    if (batch < 1 || batch > Q3_MAX_BATCH) return set_err(Q3_UNSUPPORTED, "batch %d unsupported (1..%d sequences per session)", batch, Q3_MAX_BATCH);
    HIPC(hipSetDevice(m->device));
    const q3_config& c = m->cfg;
    std::unique_ptr<q3_session> s(new q3_session());
    s->m = m; s->B = batch; s->opts = reqs[0].opts;
    { static std::atomic<uint64_t> next_uid{1}; s->uid = next_uid.fetch_add(1); }
    m->refs.fetch_add(1);
    if (s->opts.max_length < 1) return set_err(Q3_INVALID_ARG, "max_length must be >= 1");
    s->seq.resize(batch); s->out.resize((size_t)batch);
    int rows = 0;
    for (int b = 0; b < batch; ++b) {
        const q3_request& r = reqs[b];
        if (r.opts.chunk_frames != s->opts.chunk_frames) return set_err(Q3_UNSUPPORTED, "all requests of a batch must share chunk_frames (the streaming chunk is a property of the session)");
        if (!(r.opts.temperature >= 0.0) || r.opts.repetition_penalty <= 0.0) return set_err(Q3_INVALID_ARG, "bad sampling options");
        if (r.mode < 0 || r.mode > 2) return set_err(Q3_INVALID_ARG, "bad mode %d", r.mode);
        if (r.n_text < 0 || r.n_instruct < 0 || (r.n_text > 0 && !r.text_ids) || (r.n_instruct > 0 && !r.instruct_ids))
            return set_err(Q3_INVALID_ARG, "bad token id arrays");
        if (r.mode == Q3_MODE_VOICE_CLONE && !r.xvector) return set_err(Q3_INVALID_ARG, "voice clone needs an x-vector");
        SeqInfo& q = s->seq[b];
        q.req = r; q.max_length_req = r.opts.max_length;
        q.text.assign(r.text_ids, r.text_ids + r.n_text);
        for (uint32_t id : q.text) if (id >= (uint32_t)c.text_vocab) return set_err(Q3_INVALID_ARG, "text id %u out of range", id);
        if (r.mode == Q3_MODE_VOICE_DESIGN) q.instruct.assign(r.instruct_ids, r.instruct_ids + r.n_instruct);
        for (uint32_t id : q.instruct) if (id >= (uint32_t)c.text_vocab) return set_err(Q3_INVALID_ARG, "instruct id %u out of range", id);
        if (r.language_id >= (uint32_t)c.codec_vocab || (r.mode == Q3_MODE_CUSTOM_VOICE && r.speaker_id >= (uint32_t)c.codec_vocab))
            return set_err(Q3_INVALID_ARG, "speaker/language id out of range");
        if (r.xvector) q.xvec.assign(r.xvector, r.xvector + c.hidden);
        const PromptShape sh = prompt_shape(r);      // (arithmetic alone; a negative n_ref_text is refused below, before the shape sizes anything)
        q.icl = sh.icl;
        if (r.mode == Q3_MODE_VOICE_CLONE && r.n_ref > 0 && r.ref_codes) {
            // reference frames are prepended at decode whenever the prompt carries them — also without a reference
            // transcript, when the prefill stays x-vector-only (lib.rs:1022: `if let Some(ref_codes) = &prompt.ref_codes`)
            q.ref_codes.assign(r.ref_codes, r.ref_codes + (size_t)r.n_ref * 16);
            for (int f = 0; f < r.n_ref; ++f) {
                if (q.ref_codes[(size_t)f * 16] >= (uint32_t)c.codec_vocab) return set_err(Q3_INVALID_ARG, "reference semantic code out of range");
                for (int g = 1; g < 16; ++g) if (q.ref_codes[(size_t)f * 16 + g] >= (uint32_t)c.cp_vocab) return set_err(Q3_INVALID_ARG, "reference acoustic code out of range");
            }
        }
        if (q.icl) {
            if (r.n_ref_text < 0) return set_err(Q3_INVALID_ARG, "bad reference text");
            q.ref_text.assign(r.ref_text_ids, r.ref_text_ids + r.n_ref_text);
            for (uint32_t id : q.ref_text) if (id >= (uint32_t)c.text_vocab) return set_err(Q3_INVALID_ARG, "reference text id %u out of range", id);
            // lib.rs:913-929 (must be identical for every sequence of the batch, checked below through s->opts)
            q.req.opts.repetition_penalty = r.opts.repetition_penalty < 1.5 ? 1.5 : r.opts.repetition_penalty;
            q.req.opts.max_length = sh.limit;
            if (b == 0) s->opts = q.req.opts;
        }
        q.prefill_len = sh.prefill_len; q.trailing_len = sh.trailing_len;
        q.row_base = rows; q.n_rows = sh.n_rows;
        rows += q.n_rows;
        if (q.prefill_len != s->seq[0].prefill_len)
            return set_err(Q3_UNSUPPORTED, "all sequences of a batch must have the same prefill length (%d vs %d)", q.prefill_len, s->seq[0].prefill_len);
    }
    s->prefill_len = s->seq[0].prefill_len;
    s->n_rows_total = rows;
    s->max_frames = frame_budget > 1 ? frame_budget : 1;          // room for rows that arrive later with a larger limit (continuous batching)
    for (auto& q : s->seq) {
        if (q.req.opts.max_length < 1) return set_err(Q3_INVALID_ARG, "max_length must be at least 1");
        q.limit = q.req.opts.max_length; q.start_run = 0;
        if (q.limit > s->max_frames) s->max_frames = q.limit;
        if (q.n_rows > s->row_cap) s->row_cap = q.n_rows;
    }
    s->opts.max_length = s->max_frames;
    if (s->row_cap < 1024) s->row_cap = 1024;      // replacement slots hold any text up to ~1000 tokens (8 MB per row at H = 2048), longer if the batch had one
    if (prompt_budget > 0 && s->row_cap < prompt_budget + 1024) s->row_cap = prompt_budget + 1024;      // ... or the caller announced longer prompts (instruct / reference text rows are projected rows too)
    s->repl_base = rows;
    // KV sized for what the path needs (prefill + frames), not the reference's max_new_tokens+256 (lib.rs:450)
    s->max_seq = (prompt_budget > s->prefill_len ? prompt_budget : s->prefill_len) + s->max_frames + 1;   // prompt_budget: later rows with longer prompts
    if (s->max_seq > m->rope_len) return set_err(Q3_KV_OVERFLOW, "sequence length %d exceeds the RoPE table (%d)", s->max_seq, m->rope_len);
    {
        static const int ns_env = [] { const char* e = getenv("Q3_ATTN_SPLITS"); return e ? atoi(e) : 0; }();   // tuning aid
        // ~2 attention workgroups per CU over a 640-frame utterance. With the three-deep unconditional K/V requests of
        // k_attn_fused (round 2) a workgroup walks its keys without a round trip per key and fewer, longer key ranges
        // win: B = 8: 3.908 / 3.724 / 3.651 / 3.609 / 3.635 / 3.812 ms/frame at 1 / 2 / 4 / 8 / 16 / 32 splits (before:
        // 4.40 / 3.99 / 3.77 / 3.67 / 3.68); B = 1 stays at 16 (2.794 vs 2.800 at 8)
        int ns = ns_env > 0 ? ns_env : (batch <= 2 ? 1024 : 512) / (batch * c.n_kv_heads);     // (B <= 2: up to the long-context cap below)
        // long contexts (a 4k-position prompt: 38 MB of f32 K/V per layer) want more than 16 workgroups per KV head to
        // stream them (B = 1 at 4.1k positions: 3.90 -> 3.55 ms/frame); short sessions keep the cheaper 16-way merge
        const int cap = ns_env > 0 ? MAX_SPLITS : (s->max_seq > 2048 ? MAX_SPLITS : 16);
        if (ns < 1) ns = 1; if (ns > cap) ns = cap; s->n_splits = ns;
    }
    {   // the frame loop is a chain of ~600 short dependent kernels per frame: give its queue the highest priority so
        // that its workgroups are dispatched ahead of the vocoder segments running beside it (q3_session_run)
        if (borrow) { s->stream = borrow; s->owns_stream = false; }      // q3_session_replace: no second queue for a one-row prefill
        else {
            {
                std::lock_guard<std::mutex> g(m->stream_mu);
                if (!m->idle_streams.empty()) { s->stream = m->idle_streams.back(); m->idle_streams.pop_back(); }
            }
            if (!s->stream) {
                int least = 0, greatest = 0;
                HIPC(hipDeviceGetStreamPriorityRange(&least, &greatest));
                HIPC(hipStreamCreateWithPriority(&s->stream, hipStreamNonBlocking, greatest));
            }
        }
    }
    const int B = batch, H = c.hidden, CH = c.cp_hidden;
    s->pool.lazy = true;
    auto alloc_lm = [&](LmBuf& b, const LmDims& d, int nsplit) -> hipError_t {
        const int QD = d.nh * HEAD_DIM, KD = d.nkv * HEAD_DIM;
        const size_t R = batch > 16 ? (size_t)up16(batch) : 16;     // rows: up to 16 for multi-row steps (B <= 16), else one row per sequence
        hipError_t e;
        if ((e = s->pool.alloc(&b.X, R * d.H)) != hipSuccess) return e;
        if ((e = s->pool.alloc(&b.SUM, R * d.H)) != hipSuccess) return e;
        if ((e = s->pool.alloc(&b.QKV, R * (QD + 2 * KD))) != hipSuccess) return e;
        if ((e = s->pool.alloc(&b.Q, R * QD)) != hipSuccess) return e;
        if ((e = s->pool.alloc(&b.ATT, R * QD)) != hipSuccess) return e;
        if ((e = s->pool.alloc(&b.ACT, R * d.I)) != hipSuccess) return e;
        return s->pool.alloc(&b.PART, R * d.nh * nsplit * PART_STRIDE);
    };
    HIPC(alloc_lm(s->tb, talker_dims(c), s->n_splits));
    HIPC(alloc_lm(s->cb, cp_dims(c), 1));
    if (B > 16) {     // wide sessions: workspace of the split-K GEMM, sized for the largest projection of either network
        size_t need = 0;
        auto upd = [&](int N, int K, int epi) { if (N % 128 == 0 && K % 128 == 0) { const size_t b = gemm_wide_ws_bytes(B, N, K, epi); if (b > need) need = b; } };
        const int QDt = c.n_heads * HEAD_DIM, KDt = c.n_kv_heads * HEAD_DIM, QDc = c.cp_heads * HEAD_DIM, KDc = c.cp_kv_heads * HEAD_DIM;
        upd(QDt + 2 * KDt, H, EPI_NONE); upd(H, QDt, EPI_RESID); upd(c.inter, H, EPI_SWIGLU); upd(H, c.inter, EPI_RESID); upd(c.codec_vocab, H, EPI_NONE);
        upd(QDc + 2 * KDc, c.cp_hidden, EPI_NONE); upd(c.cp_hidden, QDc, EPI_RESID); upd(c.cp_inter, c.cp_hidden, EPI_SWIGLU); upd(c.cp_hidden, c.cp_inter, EPI_RESID);
        upd(c.cp_vocab, c.cp_hidden, EPI_NONE); upd(c.cp_hidden, H, EPI_NONE);
        if (need) { HIPC(s->pool.alloc(&s->wide_ws, need / 4)); s->wide_ws_bytes = need; }
    }
    HIPC(s->pool.alloc(&s->LASTH, (size_t)B * H));
    HIPC(s->pool.alloc(&s->LOGITS, (size_t)B * c.codec_vocab));
    HIPC(s->pool.alloc(&s->CP_IN, (size_t)(B > 16 ? up16(B) : 16) * H));
    HIPC(s->pool.alloc(&s->CP_LOGITS, (size_t)15 * B * c.cp_vocab));
    s->kv_layer_stride = (size_t)B * c.n_kv_heads * s->max_seq * HEAD_DIM;
    {   // talker KV: pages from the model's pool as the rows grow (default), or one extent per row sized for the worst case
        const char* e = getenv("Q3_KV_CONTIGUOUS");          // read per session: the paged-vs-contiguous test flips it
        s->paged = !(e && atoi(e) != 0);
        if (s->paged) {
            if (s->max_seq > KV_MAX_PAGES * KV_PAGE_POS) return set_err(Q3_KV_OVERFLOW, "sequence length %d exceeds a row's page table (%d)", s->max_seq, KV_MAX_PAGES * KV_PAGE_POS);
            HIPC(s->pool.alloc(&s->kv_table, (size_t)B * KV_MAX_PAGES));
            HIPC(s->pool.alloc(&s->kv_conv, (size_t)2 * B * KV_MAX_PAGES));
            HIPC(s->pool.alloc(&s->park_desc, PARK_DESC_BYTES));      // q3_session_park_row / _resume_row: nothing is allocated at a frame boundary
            s->shelf = std::make_shared<ParkShelf>();
            s->kv_rows.resize((size_t)B);
            for (auto& r : s->kv_rows) r.reserve(KV_MAX_PAGES);
        } else {
            HIPC(s->pool.alloc(&s->kcache, s->kv_layer_stride * c.n_layers));
            HIPC(s->pool.alloc(&s->vcache, s->kv_layer_stride * c.n_layers));
        }
    }
    s->ckv_layer_stride = (size_t)B * c.cp_kv_heads * (c.n_groups + 1) * HEAD_DIM;
    // K and V of the code predictor in ONE block: k_attn_cp takes their distance as a 32-bit float count, and two blocks of the
    // size-class cache can lie further apart than that (the launch then silently fell back to k_attn_fused: 70 nodes per
    // frame 1.1 us slower each — seen in a profiling run of round 4)
    HIPC(s->pool.alloc(&s->ckcache, 2 * s->ckv_layer_stride * c.cp_layers + 64));
    s->cvcache = s->ckcache + s->ckv_layer_stride * c.cp_layers + 64;
    HIPC(s->pool.alloc(&s->rows, ((size_t)rows + (size_t)B * s->row_cap) * H));      // + one replacement slot per row (q3_session_replace)
    HIPC(s->pool.alloc(&s->limit, B));
    HIPC(s->pool.alloc(&s->sample_rows, B));
    {
        std::vector<int> lim(B); std::vector<SampleRow> sr(B);
        for (int b = 0; b < B; ++b) { lim[b] = s->seq[b].limit; sr[b] = sample_row(s->seq[b].req.opts); }
        HIPC(q3_hipMemcpy(s->limit, lim.data(), B * 4, hipMemcpyHostToDevice));
        HIPC(q3_hipMemcpy(s->sample_rows, sr.data(), B * sizeof(SampleRow), hipMemcpyHostToDevice));
    }
    HIPC(s->pool.alloc(&s->embeds, (size_t)B * s->prefill_len * H));
    HIPC(s->pool.alloc(&s->xvec, (size_t)B * H));
    HIPC(s->pool.alloc(&s->ids_dev, (size_t)rows)); HIPC(s->pool.alloc(&s->tr_dev, (size_t)B * s->prefill_len)); HIPC(s->pool.alloc(&s->ci_dev, (size_t)B * s->prefill_len));
    HIPC(s->pool.alloc(&s->proj_e, (size_t)rows * c.text_dim)); HIPC(s->pool.alloc(&s->proj_h, (size_t)rows * c.text_dim));
    HIPC(s->pool.alloc(&s->trail_base, B)); HIPC(s->pool.alloc(&s->trail_len, B)); HIPC(s->pool.alloc(&s->pad_row, B));
    HIPC(s->pool.alloc(&s->tok, B)); HIPC(s->pool.alloc(&s->seen, (size_t)B * c.codec_vocab));
    HIPC(s->pool.alloc(&s->frame_idx, B)); HIPC(s->pool.alloc(&s->pos, B)); HIPC(s->pool.alloc(&s->token_count, B));
    HIPC(s->pool.alloc(&s->U, (size_t)B * (s->max_frames + 2)));      // one draw per sampled token (max_frames + 1) + a spare for a frozen row
    HIPC(s->pool.alloc(&s->codes, (size_t)B * s->max_frames * 16));
    // RNG: one PCG stream per sequence, one draw per sampled token
    std::vector<float> U((size_t)B * (s->max_frames + 2), 0.0f);
    for (int b = 0; b < B; ++b) {
        uint64_t st;
        const q3_options& o = reqs[b].opts;
        uint64_t seed = o.seed;
        if (!o.has_seed) seed = (uint64_t)std::chrono::high_resolution_clock::now().time_since_epoch().count() + 0x9E37ULL * b;
        q3_rng_seed(seed, &st);
        for (int i = 0; i <= s->max_frames; ++i) U[(size_t)b * (s->max_frames + 2) + i] = q3_rng_next(&st);
    }
    HIPC(q3_hipMemcpy(s->U, U.data(), U.size() * 4, hipMemcpyHostToDevice));
    HIPC(s->pool.settle());                 // every zero-fill has landed before a kernel on the session's own stream can run
    s->pool.lazy = false;
    *out = s.release();
    return Q3_OK;
}

// Every exit path (q3_session_free, a failed q3_session_create) goes through here: streams are drained BEFORE the pool's
// blocks return to the device cache (member destructors run after this body), so no later session is handed memory a
// queued kernel still writes.
q3_session::~q3_session() {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (dec_stream) (void)hipStreamSynchronize(dec_stream);
    for (auto st : par_streams) (void)hipStreamSynchronize(st);
    if (aql) q3::aql_program_destroy(aql);               // waits for its outstanding replays
    for (int b = 0; b < (int)kv_rows.size(); ++b) kv_release_row(this, b);      // every stream that touched them is idle
    if (shelf) {         // records that outlive the session give their blocks to the device-memory cache themselves
        std::lock_guard<std::mutex> g(shelf->mu);
        shelf->alive = false;
        for (auto& blk : shelf->blocks) dev_free(blk.first);
        shelf->blocks.clear();
    }
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    if (graph) (void)hipGraphDestroy(graph);
    for (auto& ev : prof_pool) (void)hipEventDestroy(ev);
    for (auto st : par_streams) (void)hipStreamDestroy(st);
    if (ostage) q3_pcm_stage_free(ostage);
    if (cstream) q3_codec_stream_free(cstream);          // (drops its own reference to the model: ours is still held)
    cws.release(); seg_ws.release();
    for (auto& w : par_ws) w.release();
    if (dec_ev) (void)hipEventDestroy(dec_ev);
    if (dec_stream) (void)hipStreamDestroy(dec_stream);
    if (stream && owns_stream) {                   // synchronised above: idle, handed to the next session of this model
        std::lock_guard<std::mutex> g(m->stream_mu);
        if (m->idle_streams.size() < 16) { m->idle_streams.push_back(stream); stream = nullptr; }
    }
    if (stream && owns_stream) (void)hipStreamDestroy(stream);
    pool.release_all();                                          // the model's device must still be current for these
    if (m->refs.fetch_sub(1) == 1) model_destroy(m);          // the model handle was given up before its last session
}

extern "C" void q3_session_free(q3_session* s) { delete s; }

// K/V dtype of the talker cache (before q3_session_prefill): Q3_DTYPE_F32 (default: the parity contract is the reference's CPU
// F32 path) or Q3_DTYPE_BF16 — the reference GPU path's cache dtype (kv_cache.rs:234-310): half the K/V bytes per frame, results
// no longer bit-comparable with the F32 oracle. Needs the paged cache.
extern "C" q3_status q3_session_set_kv_dtype(q3_session* s, int dtype) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (s->prefilled) return set_err(Q3_INVALID_ARG, "q3_session_set_kv_dtype must be called before prefill");
    if (dtype != Q3_DTYPE_F32 && dtype != Q3_DTYPE_BF16) return set_err(Q3_INVALID_ARG, "q3_session_set_kv_dtype: unknown dtype %d", dtype);
    if (dtype == Q3_DTYPE_BF16 && !s->paged) return set_err(Q3_UNSUPPORTED, "bf16 K/V needs the paged cache (Q3_KV_CONTIGUOUS is set)");
    s->kv_bf16 = dtype == Q3_DTYPE_BF16;
    return Q3_OK;
}

extern "C" q3_status q3_session_set_debug(q3_session* s, int capture) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (s->prefilled) return set_err(Q3_INVALID_ARG, "set_debug must be called before prefill");
    if (capture && s->text_ready) return set_err(Q3_UNSUPPORTED, "set_debug: the session has open text rows");
    s->debug = capture != 0;
    if (s->debug && !s->logits_hist) {
        const q3_config& c = s->m->cfg;
        HIPC(hipSetDevice(s->m->device));
        HIPC(s->pool.alloc(&s->logits_hist, (size_t)s->B * (s->max_frames + 1) * c.codec_vocab));
        HIPC(s->pool.alloc(&s->cp_logits_hist, (size_t)s->max_frames * 15 * s->B * c.cp_vocab));
    }
    return Q3_OK;
}
extern "C" q3_status q3_session_set_profile(q3_session* s, int enable) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (enable && s->text_ready) return set_err(Q3_UNSUPPORTED, "set_profile: the session has open text rows");
    s->profile = enable != 0;
    return Q3_OK;
}
extern "C" q3_status q3_session_stream(q3_session* s, void** stream) {
    if (!s || !stream) return set_err(Q3_INVALID_ARG, "null argument");
    *stream = (void*)s->stream;
    return Q3_OK;
}
extern "C" q3_status q3_session_prefill_len(q3_session* s, int b, int* prefill_len, int* trailing_len) {
    if (!s || b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "bad sequence index");
    if (!s->ragged.empty()) {                    // a ragged batch before its prefill: the rows are still idle placeholders
        if (prefill_len) *prefill_len = prompt_shape(s->ragged[(size_t)b].r).prefill_len;
        if (trailing_len) *trailing_len = -1;
        return Q3_OK;
    }
    if (prefill_len) *prefill_len = s->seq[b].prefill_len;
    if (trailing_len) *trailing_len = s->seq[b].trailing_len;
    return Q3_OK;
}

// text projection (talker.rs:316-320) of `n` gathered rows: fc2(silu(fc1(e)+b1))+b2, 8 rows a time
static q3_status text_project(q3_session* s, const uint32_t* ids_dev, int n, float* out_rows) {
    const q3_model* m = s->m; const q3_config& c = m->cfg;
    const int TD = c.text_dim, H = c.hidden;
    if (n > s->n_rows_total) return set_err(Q3_INVALID_ARG, "text_project: %d rows exceed the session's %d", n, s->n_rows_total);
    float *e = s->proj_e, *h = s->proj_h;      // session scratch: everything below is queued on s->stream, nothing waits
    q3_status st = Q3_OK;
    hipError_t er = launch_gather_rows_bf16(m->text_emb, ids_dev, e, n, TD, s->stream);
    if (er == hipSuccess && n >= 48 && TD % 64 == 0 && H % 64 == 0 && !s->no_chunk) {
        // TextProjection (talker.rs:316-320) over all n token rows as two GEMMs instead of n/8 GEMV passes
        GemmArgs g1; g1.W = m->fc1w.t1; g1.x = e; g1.ldx = TD; g1.bias = m->fc1b; g1.y = h; g1.ldy = TD;
        g1.M = n; g1.N = TD; g1.K = TD; g1.Kpad = (TD + 31) / 32 * 32; g1.epi = EPI_SILU;
        er = launch_lm_gemm(g1, s->stream);
        if (er == hipSuccess) {
            GemmArgs g2; g2.W = m->fc2w.t1; g2.x = h; g2.ldx = TD; g2.bias = m->fc2b; g2.y = out_rows; g2.ldy = H;
            g2.M = n; g2.N = H; g2.K = TD; g2.Kpad = (TD + 31) / 32 * 32; g2.epi = EPI_NONE;
            er = launch_lm_gemm(g2, s->stream);
        }
    } else
    for (int r0 = 0; r0 < n && er == hipSuccess; r0 += 8) {
        const int M = (n - r0) < 8 ? (n - r0) : 8;
        LinArgs a;
        a.N = TD; a.K = TD; set_w(a, m->fc1w, M, TD, TD); a.x = e + (size_t)r0 * TD; a.ldx = TD; a.bias = m->fc1b; a.y = h + (size_t)r0 * TD; a.ldy = TD; a.M = M; a.epi = EPI_SILU;
        er = launch_linear(a, s->stream);
        if (er != hipSuccess) break;
        LinArgs b2;
        b2.N = H; b2.K = TD; set_w(b2, m->fc2w, M, H, TD); b2.x = h + (size_t)r0 * TD; b2.ldx = TD; b2.bias = m->fc2b; b2.y = out_rows + (size_t)r0 * H; b2.ldy = H; b2.M = M; b2.epi = EPI_NONE;
        er = launch_linear(b2, s->stream);
    }
    if (er != hipSuccess) st = set_err(Q3_HIP_ERROR, "text projection: %s", hipGetErrorString(er));
    return st;
}

// ---- open text rows (q3_session_open_text / q3_session_append_text) ----
// An opened row's trailing text rows live in its replacement slot (rows repl_base + b * row_cap ..), contiguous as k_frame_embed
// indexes them; frame f of the row may commit only once trailing row f is there (text_ready[b] > f), else the row is HELD.
static int slot_row0(const q3_session* s, int b) { return s->repl_base + b * s->row_cap; }
// trailing text rows of an opened row so far, without tts_eos: its text minus what the prefill consumes
static int open_n_trail(const SeqInfo& q) { return prompt_shape(q.request(), (int)q.text_all.size()).n_trail; }
// ... and their ids: the tail of [ref_text (ICL rows alone hold one), text]
static void open_trailing_ids(const SeqInfo& q, std::vector<uint32_t>& out) {
    std::vector<uint32_t> all(q.ref_text);
    all.insert(all.end(), q.text_all.begin(), q.text_all.end());
    out.assign(all.end() - open_n_trail(q), all.end());
}
// host view of an opened row's text: trailing rows present, what the frame reads (+ tts_eos once closed), frames allowed
static void open_counts(SeqInfo& q) {
    q.n_trail = open_n_trail(q);
    q.trailing_len = q.n_trail + (q.text_closed ? 1 : 0);
    q.ready = q.text_closed ? 0x7fffffff : q.n_trail;
    // the ICL length cap over the whole text, resolved at close against the request's own max_length
    if (q.icl && q.text_closed) q.limit = std::min(q.max_length_req, icl_frame_cap((int)q.text_all.size()));
}
// Appended text rows take ONE projection path whatever a call carries: 8-row GEMV groups, the unused rows of the last group
// padded in scratch. (text_project picks two GEMMs from 48 rows on, and at 1.7B the two sum in different orders: a token's bits
// would depend on what it was projected with.) Rows [dst, dst + n) of row b's slot; queued on the session stream.
// One group: 8 ids on the device -> app_out[8][H]. q3_session_append_text and the batcher's flush (session_append_many) both come
// through here, so a token's row has the same bits whichever of the two received it.
static hipError_t project_group(q3_session* s, const uint32_t* ids_dev) {
    const q3_model* m = s->m; const q3_config& c = m->cfg;
    const int TD = c.text_dim, H = c.hidden;
    hipError_t er = launch_gather_rows_bf16(m->text_emb, ids_dev, s->app_e, 8, TD, s->stream);
    if (er != hipSuccess) return er;
    LinArgs a;
    a.N = TD; a.K = TD; set_w(a, m->fc1w, 8, TD, TD); a.x = s->app_e; a.ldx = TD; a.bias = m->fc1b; a.y = s->app_h; a.ldy = TD; a.M = 8; a.epi = EPI_SILU;
    er = launch_linear(a, s->stream);
    if (er != hipSuccess) return er;
    LinArgs b2;
    b2.N = H; b2.K = TD; set_w(b2, m->fc2w, 8, H, TD); b2.x = s->app_h; b2.ldx = TD; b2.bias = m->fc2b; b2.y = s->app_out; b2.ldy = H; b2.M = 8; b2.epi = EPI_NONE;
    return launch_linear(b2, s->stream);
}
static q3_status project_appended(q3_session* s, int b, const std::vector<uint32_t>& ids, int dst) {
    const int H = s->m->cfg.hidden, n = (int)ids.size(), row0 = slot_row0(s, b);
    if (n <= 0) return Q3_OK;
    std::vector<uint32_t> padded((size_t)(n + 7) / 8 * 8);       // lives until the synchronisation below
    for (size_t i = 0; i < padded.size(); ++i) padded[i] = ids[i < (size_t)n ? i : (size_t)n - 1];
    hipError_t er = hipSuccess;
    for (int r0 = 0; r0 < n && er == hipSuccess; r0 += 8) {
        const int k = (n - r0) < 8 ? (n - r0) : 8;
        er = hipMemcpyAsync(s->app_ids, padded.data() + r0, 8 * 4, hipMemcpyHostToDevice, s->stream);
        if (er == hipSuccess) er = project_group(s, s->app_ids);
        if (er == hipSuccess)
            er = hipMemcpyAsync(s->rows + (size_t)(row0 + dst + r0) * H, s->app_out, (size_t)k * H * 4, hipMemcpyDeviceToDevice, s->stream);
    }
    const hipError_t es = sync_frames(s);
    if (er == hipSuccess) er = es;
    if (er != hipSuccess) return set_err(Q3_HIP_ERROR, "appended text projection: %s", hipGetErrorString(er));
    return Q3_OK;
}
// what the frame reads of an opened row — trail_len, text_ready, limit — published on the session stream, landed on return
static q3_status publish_text(q3_session* s, int b) {
    const SeqInfo& q = s->seq[(size_t)b];
    const int v[3] = {q.trailing_len, q.ready, q.limit};
    HIPC(hipMemcpyAsync(s->trail_len + b, &v[0], 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->text_ready + b, &v[1], 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->limit + b, &v[2], 4, hipMemcpyHostToDevice, s->stream));
    HIPC(sync_frames(s));
    return Q3_OK;
}
static bool any_open_text(const q3_session* s) { for (const auto& q : s->seq) if (q.opened && !q.text_closed) return true; return false; }

// text_ready (every row closed) and the scratch of the appended rows' projection path, once per session
static q3_status alloc_text_state(q3_session* s) {
    if (s->text_ready) return Q3_OK;
    const q3_config& c = s->m->cfg;
    HIPC(s->pool.alloc(&s->text_ready, (size_t)s->B));
    HIPC(s->pool.alloc(&s->app_ids, 8)); HIPC(s->pool.alloc(&s->app_e, (size_t)8 * c.text_dim));
    HIPC(s->pool.alloc(&s->app_h, (size_t)8 * c.text_dim)); HIPC(s->pool.alloc(&s->app_out, (size_t)8 * c.hidden));
    const std::vector<int> closed((size_t)s->B, 0x7fffffff);
    HIPC(q3_hipMemcpy(s->text_ready, closed.data(), (size_t)s->B * 4, hipMemcpyHostToDevice));
    return Q3_OK;
}

extern "C" q3_status q3_session_open_text(q3_session* s, int b) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "q3_session_open_text: bad sequence index %d", b);
    if (s->prefilled) return set_err(Q3_INVALID_ARG, "q3_session_open_text: rows are opened before q3_session_prefill");
    if (!s->ragged.empty()) return set_err(Q3_UNSUPPORTED, "q3_session_open_text: not in a ragged first batch (rows of different prefill lengths)");
    if (s->debug || s->profile) return set_err(Q3_UNSUPPORTED, "q3_session_open_text: not on debug / profiling sessions");
    SeqInfo& q = s->seq[(size_t)b];
    if (q.opened) return Q3_OK;
    if (q.text.empty()) return set_err(Q3_INVALID_ARG, "q3_session_open_text: row %d has no text token (an open row needs one at creation: the prefill consumes it)", b);
    if (q.icl) {
        const int need = prompt_shape(q.request()).open_need;
        if ((int)q.text.size() < need)
            return set_err(Q3_INVALID_ARG, "q3_session_open_text: ICL row %d needs at least %d target text tokens at creation (%d given), so that tts_eos falls after the ICL block", b, need, (int)q.text.size());
        if (q.max_length_req > s->max_frames)
            return set_err(Q3_UNSUPPORTED, "q3_session_open_text: ICL row %d asks for max_length %d beyond the session's frame budget %d (its length cap is resolved when the text closes; q3_session_create_reserved)", b, q.max_length_req, s->max_frames);
    }
    HIPC(hipSetDevice(s->m->device));
    Q3C(alloc_text_state(s));
    q.opened = true; q.text_closed = false; q.text_all = q.text; q.committed = 0;
    if (q.icl) q.limit = q.max_length_req;          // until the text closes (open_counts)
    open_counts(q);
    if (q.n_trail + 1 > s->row_cap) { q.opened = false; q.text_closed = true; return set_err(Q3_UNSUPPORTED, "q3_session_open_text: %d trailing text rows exceed the row's slot (%d)", q.n_trail + 1, s->row_cap); }
    HIPC(q3_hipMemcpy(s->limit + b, &q.limit, 4, hipMemcpyHostToDevice));
    return Q3_OK;
}

static q3_status refresh_codes(q3_session* s);
extern "C" q3_status q3_session_append_text(q3_session* s, int b, const uint32_t* ids, int n, int last) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "q3_session_append_text: bad sequence index %d", b);
    if (n < 0 || (n > 0 && !ids)) return set_err(Q3_INVALID_ARG, "q3_session_append_text: bad token id array");
    SeqInfo& q = s->seq[(size_t)b];
    if (!q.opened) return set_err(Q3_INVALID_ARG, "q3_session_append_text: row %d is not open (q3_session_open_text, before the prefill)", b);
    if (q.text_closed) return set_err(Q3_INVALID_ARG, "q3_session_append_text: row %d's text is already closed", b);
    const q3_config& c = s->m->cfg;
    for (int i = 0; i < n; ++i) if (ids[i] >= (uint32_t)c.text_vocab) return set_err(Q3_INVALID_ARG, "text id %u out of range", ids[i]);
    if (q.n_trail + n + 1 > s->row_cap) return set_err(Q3_UNSUPPORTED, "q3_session_append_text: %d trailing text rows exceed the row's slot (%d)", q.n_trail + n + 1, s->row_cap);
    if (!s->prefilled) {                 // the prefill projects whatever has arrived by then
        q.text_all.insert(q.text_all.end(), ids, ids + n);
        if (last) q.text_closed = true;
        open_counts(q);
        return Q3_OK;
    }
    HIPC(hipSetDevice(s->m->device));
    HIPC(sync_frames(s));                // no frame in flight while the row's text changes (q3_session_replace does the same)
    Q3C(refresh_codes(s));
    if (q.done) { q.text_all.insert(q.text_all.end(), ids, ids + n); if (last) q.text_closed = true; return Q3_OK; }   // ended (EOS / max_length): accepted, ignored
    std::vector<uint32_t> rows(ids, ids + n);
    if (last) rows.push_back(TTS_EOS);
    const int dst = q.n_trail;
    Q3C(project_appended(s, b, rows, dst));      // rows beyond trail_len: no frame reads them before publish_text
    q.text_all.insert(q.text_all.end(), ids, ids + n);
    if (last) q.text_closed = true;
    open_counts(q);
    Q3C(publish_text(s, b));
    s->codes_host_valid = false;
    return Q3_OK;
}

extern "C" q3_status q3_session_text_state(q3_session* s, int b, int* n_text, int* frames_committed, int* frames_runnable, int* closed,
                                           int* frames_replayed) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "q3_session_text_state: bad sequence index %d", b);
    const SeqInfo& q = s->seq[(size_t)b];
    int committed = 0, runnable = 0;
    if (s->prefilled) {
        HIPC(hipSetDevice(s->m->device));
        Q3C(refresh_codes(s));
        committed = q.opened ? q.committed : std::min(std::max(s->frames_run - q.start_run, 0), q.limit);
        runnable = q.done ? 0 : (q.opened ? std::min(q.ready, q.limit) : q.limit) - committed;
        if (runnable < 0) runnable = 0;
    } else {
        runnable = q.opened ? std::min(q.ready, q.limit) : q.limit;
    }
    if (n_text) *n_text = (int)(q.opened ? q.text_all.size() : q.text.size());
    if (frames_committed) *frames_committed = committed;
    if (frames_runnable) *frames_runnable = runnable;
    if (closed) *closed = q.text_closed ? 1 : 0;
    if (frames_replayed) *frames_replayed = s->frames_run;
    return Q3_OK;
}

// run_prefill_layers (talker.rs:823-841) for long prompts: chunks of up to 128 positions per sequence go through every
// layer as GEMMs over the decode path's tiled weight image + a query-blocked causal attention (q3_kernels_prefill.hip).
// Leaves the KV cache filled for positions [0, S) and LASTH / LOGITS of the last position, like the chunked decode-step
// schedule it replaces for S >= 48.
// positions per sequence per GEMM pass (prefill_gemm below)
static int prefill_gemm_chunk(int B) {
    static const int rows_env = [] { const char* e = getenv("Q3_PREFILL_ROWS"); return e ? atoi(e) : 4224; }();
    const int C = rows_env / B;
    return C < 128 ? 128 : (C / 128) * 128;
}
// P0 > 0: positions [0, P0) are already in the rows' pages (linked from the prefix cache) and are not computed again. The passes
// keep the cuts of the run from 0 — the same chunks, and inside the chunk P0 lies in the same query blocks (prefix_usable_pages rounds P0
// to a block boundary of that chunk) — so every position from P0 on sees the arithmetic of the uncached run.
// A packed pass (pk): the prompts of pk->side — one-row side sessions of `s`, staged, each from position 0 and
// of its own length — lie end to end in ONE activation matrix and go through the layers together: the GEMMs see one M (their
// bits are batch-invariant), the attention-side launches find sequences through the pack's tables, and each row's head writes
// its side session's LASTH / LOGITS with the launches of its one-row prefill. S_all, S and P0 are unused then.
struct PrefillPack { std::vector<q3_session*> side; PackHost host; };
static bool prefill_x3_on() { const char* x3e = getenv("Q3_PREFILL_ATTN_X3"); return !(x3e && atoi(x3e) == 0); }
static q3_status prefill_gemm(q3_session* s, int S_all, int S, bool with_head, int P0 = 0, const PrefillPack* pk = nullptr) {      // positions [P0, S) of the S_all-position prompts
    const q3_model* m = s->m; const q3_config& c = m->cfg;
    const LmDims d = talker_dims(c);
    const int B = pk ? 1 : s->B, H = d.H, QD = d.nh * HEAD_DIM, KD = d.nkv * HEAD_DIM, I = d.I;
    if (pk) { S_all = S = pk->host.rows; P0 = 0; }      // one chunk of all the pack's rows
    // positions per sequence per pass: up to 4224 activation rows per launch (a whole 4k-position prompt in one pass:
    // 33 M-tiles x N/128 workgroups per GEMM, 520 attention workgroups; 2048-row passes: 113 ms instead of 99 for the
    // 4105-position prefill of the 1.7B model), at least one 128-row tile per sequence
    const int C = pk ? S : prefill_gemm_chunk(B);
    const int max_rows = B * (S < C ? S : C);
    struct SyncedPool : DevPool { hipStream_t st; explicit SyncedPool(hipStream_t s_) : st(s_) {} ~SyncedPool() { (void)hipStreamSynchronize(st); } };
    SyncedPool tmp(s->stream);       // on EVERY return path the stream is drained before the blocks go back to the cache
    float *X, *QKV, *Qb, *ATT, *SUM, *ACT, *DEN;
    HIPC(tmp.alloc(&X, (size_t)max_rows * H)); HIPC(tmp.alloc(&QKV, (size_t)max_rows * (QD + 2 * KD)));
    HIPC(tmp.alloc(&Qb, (size_t)max_rows * QD)); HIPC(tmp.alloc(&ATT, (size_t)max_rows * QD));
    HIPC(tmp.alloc(&SUM, (size_t)max_rows * H)); HIPC(tmp.alloc(&ACT, (size_t)max_rows * I)); HIPC(tmp.alloc(&DEN, (size_t)max_rows));
    auto kp = [](int K) { return (K + 31) / 32 * 32; };
    // every GEMM input is split once into its three exact bf16 terms (launch_split_rows) instead of once per workgroup
    // column inside the GEMM; Q3_GEMM_NO_PLANES=1 keeps the in-kernel split (A/B aid)
    // long prompts: every query block's key range is halved over two workgroups and merged (k_attn_prefill_t)
    static const bool no_split = getenv("Q3_PREFILL_ATTN_NOSPLIT") != nullptr;
    static const bool gen2_attn = getenv("Q3_PREFILL_ATTN_GEN2") != nullptr || getenv("Q3_PREFILL_ATTN_VALU") != nullptr;
    const bool kv_split = !pk && !no_split && !gen2_attn && S >= 1024;
    float* PART = nullptr;
    if (kv_split) HIPC(tmp.alloc(&PART, (size_t)max_rows * d.nh * 2 * PART_STRIDE));
    // bf16-matrix-core attention (k_attn_prefill_x3) over per-layer bf16x3 planes of the cached K/V; Q3_PREFILL_ATTN_X3=0
    // keeps the f32-MFMA generation (A/B aid, read per call)
    const bool attn_x3 = pk ? pk->host.n_plane_items > 0 : !gen2_attn && prefill_x3_on() && S >= 256;
    unsigned char* KVP = nullptr;
    const int kvp_tiles = pk ? pk->host.plane_tiles : (S + 31) / 32;      // (a pack: all its sequences' tiles, kv heads included)
    if (attn_x3) HIPC(tmp.alloc(&KVP, (size_t)(pk ? 1 : B * d.nkv) * kvp_tiles * KVP_TILE_BYTES));
    // a pack's tables and the page-table rows of its side sessions, one block each
    int* PKT = nullptr; unsigned long long* PKP = nullptr; PackTab ptab{};
    if (pk) {
        if (!s->paged || gen2_attn) return set_err(Q3_INVALID_ARG, "packed prefill: needs paged K/V and the default attention kernels");
        HIPC(tmp.alloc(&PKT, pk->host.blob.size())); HIPC(tmp.alloc(&PKP, pk->side.size() * KV_MAX_PAGES));
        HIPC(hipMemcpyAsync(PKT, pk->host.blob.data(), pk->host.blob.size() * 4, hipMemcpyHostToDevice, s->stream));
        for (size_t j = 0; j < pk->side.size(); ++j)      // (the side sessions run on this stream: their table uploads are in order before this copy)
            HIPC(hipMemcpyAsync(PKP + j * KV_MAX_PAGES, pk->side[j]->kv_table, (size_t)KV_MAX_PAGES * 8, hipMemcpyDeviceToDevice, s->stream));
        ptab = pk->host.tab(PKT);
    }
    static const bool no_planes = getenv("Q3_GEMM_NO_PLANES") != nullptr;
    const bool planes = !no_planes && H % 8 == 0 && QD % 8 == 0 && I % 8 == 0;
    const int kmax = std::max(kp(H), std::max(kp(QD), kp(I)));
    const size_t plane_elems = (size_t)((max_rows + 127) / 128 * 128) * kmax;      // whole 128-row tiles (GemmArgs::xp)
    uint16_t* XP = nullptr;
    if (planes) HIPC(tmp.alloc(&XP, plane_elems * 3));
    auto split = [&](GemmArgs& g) -> hipError_t {
        if (!planes) return hipSuccess;
        g.xp = XP; g.xp_plane = plane_elems;
        return launch_split_rows(g.x, g.ldx, g.norm_w, XP, plane_elems, g.M, g.K, g.Kpad, s->stream);
    };
    // split-K workspace of the third GEMM geometry: small row counts only (that is where a GEMM's grid underfills the chip)
    float* SKW = nullptr; size_t skw_bytes = 0;
    if (planes && max_rows <= 1024) { skw_bytes = (size_t)8 * max_rows * (QD + 2 * KD > 2 * I / 4 ? QD + 2 * KD : 2 * I / 4) * sizeof(float); HIPC(tmp.alloc(&SKW, skw_bytes / sizeof(float))); }
    int ch = 0;
    for (int c0 = 0; c0 < S; c0 += C) {
        const int c1 = (S - c0) < C ? S : c0 + C;                // the chunk [c0, c1) of the run from 0
        if (c1 <= P0) continue;
        const int t0 = c0 > P0 ? c0 : P0;
        ch = c1 - t0;
        const int rows = B * ch;
        if (pk) {
            const PackSeq* ps = reinterpret_cast<const PackSeq*>(pk->host.blob.data() + pk->host.off_seq);
            for (size_t j = 0; j < pk->side.size(); ++j)
                HIPC(launch_copy_rows(pk->side[j]->embeds, H, X + (size_t)ps[j].row0 * H, H, ps[j].len, H, s->stream));
        } else
        for (int b = 0; b < B; ++b)
            HIPC(launch_copy_rows(s->embeds + ((size_t)b * S_all + t0) * H, H, X + (size_t)b * ch * H, H, ch, H, s->stream));
        for (int i = 0; i < d.layers; ++i) {
            const LayerW& w = m->tl[i];
            HIPC(launch_row_den(X, H, DEN, rows, H, d.eps, s->stream));
            GemmArgs g; g.W = w.qkv.t1; g.x = X; g.ldx = H; g.norm_w = w.in_ln; g.den = DEN; g.y = QKV; g.ldy = QD + 2 * KD;
            g.M = rows; g.N = QD + 2 * KD; g.K = H; g.Kpad = kp(H); g.epi = EPI_NONE;
            g.splitk_ws = SKW; g.splitk_ws_bytes = skw_bytes;
            HIPC(split(g)); HIPC(launch_lm_gemm(g, s->stream));
            AttnArgs t{};
            t.qkv = QKV; t.ld_qkv = QD + 2 * KD; t.q_norm_w = w.q_norm; t.k_norm_w = w.k_norm; t.eps = d.eps;
            t.rope_cos = m->rope_cos; t.rope_sin = m->rope_sin; t.pos_dev = nullptr; t.pos_static = t0;
            if (s->paged) {
                t.kv_pages = pk ? PKP : s->kv_table; t.kv_layer_off = (size_t)i * m->kv_pool.layer_stride(); t.kv_vdelta = m->kv_pool.v_delta();
            } else { t.kcache = s->kcache + (size_t)i * s->kv_layer_stride; t.vcache = s->vcache + (size_t)i * s->kv_layer_stride; }
            t.max_seq = s->max_seq; t.qbuf = Qb; t.part = nullptr; t.out = ATT; t.ld_out = QD;
            t.B = rows; t.nh = d.nh; t.nkv = d.nkv; t.n_splits = 1; t.rows_per_seq = ch;
            if (pk) {      // one launch each of norm + RoPE + append and of the plane split, at most one per attention kernel
                HIPC(launch_qknorm_rope_kv_pack(t, ptab, s->stream));
                if (attn_x3) { HIPC(launch_kv_planes_pack(t, ptab, KVP, s->stream)); t.kvp = KVP; t.kvp_tiles = kvp_tiles; }
                HIPC(launch_attn_prefill_pack(t, ptab, AP_T, s->stream));
                HIPC(launch_attn_prefill_pack(t, ptab, AP_X3, s->stream));
            } else {
            HIPC(launch_qknorm_rope_kv(t, s->stream));
            if (attn_x3) {
                HIPC(launch_kv_planes(t, B * d.nkv, t0 + ch, kvp_tiles, KVP, s->stream));
                t.kvp = KVP; t.kvp_tiles = kvp_tiles;
            }
            if (kv_split) { t.part = PART; t.n_splits = 2; }
            HIPC(launch_attn_prefill(t, s->stream));
            if (kv_split) HIPC(launch_attn_merge(t, s->stream));
            }
            GemmArgs o; o.W = w.o.t1; o.x = ATT; o.ldx = QD; o.resid = X; o.ldr = H; o.y = SUM; o.ldy = H;
            o.M = rows; o.N = H; o.K = QD; o.Kpad = kp(QD); o.epi = EPI_RESID;
            o.splitk_ws = SKW; o.splitk_ws_bytes = skw_bytes;
            HIPC(split(o)); HIPC(launch_lm_gemm(o, s->stream));
            HIPC(launch_row_den(SUM, H, DEN, rows, H, d.eps, s->stream));
            GemmArgs gu; gu.W = w.gate.t1; gu.W2 = w.up.t1; gu.x = SUM; gu.ldx = H; gu.norm_w = w.post_ln; gu.den = DEN; gu.y = ACT; gu.ldy = I;
            gu.M = rows; gu.N = I; gu.K = H; gu.Kpad = kp(H); gu.epi = EPI_SWIGLU;
            gu.splitk_ws = SKW; gu.splitk_ws_bytes = skw_bytes;
            HIPC(split(gu)); HIPC(launch_lm_gemm(gu, s->stream));
            GemmArgs dn; dn.W = w.down.t1; dn.x = ACT; dn.ldx = I; dn.resid = SUM; dn.ldr = H; dn.y = X; dn.ldy = H;
            dn.M = rows; dn.N = H; dn.K = I; dn.Kpad = kp(I); dn.epi = EPI_RESID;
            dn.splitk_ws = SKW; dn.splitk_ws_bytes = skw_bytes;
            HIPC(split(dn)); HIPC(launch_lm_gemm(dn, s->stream));
        }
    }
    if (!with_head) { HIPC(sync_frames(s)); return Q3_OK; }      // the caller runs the remaining positions
    if (pk) {      // each row's head as its one-row prefill launches it, into its side session
        const PackSeq* ps = reinterpret_cast<const PackSeq*>(pk->host.blob.data() + pk->host.off_seq);
        for (size_t j = 0; j < pk->side.size(); ++j) {
            q3_session* sd = pk->side[j];
            HIPC(launch_rmsnorm(X + (size_t)(ps[j].row0 + ps[j].len - 1) * H, ps[j].len * H, m->norm, sd->LASTH, H, 1, H, c.rms_eps, s->stream));
            LinArgs h;
            h.N = c.codec_vocab; h.K = H; set_w(h, m->codec_head, 1, h.N, h.K); h.x = sd->LASTH; h.ldx = H; h.y = sd->LOGITS; h.ldy = c.codec_vocab;
            h.M = 1; h.epi = EPI_NONE;
            HIPC(run_linear(sd, h));
        }
        HIPC(sync_frames(s));
        return Q3_OK;
    }
    // head on each sequence's last position (row b*ch + ch-1 of the last chunk): final norm -> LASTH, codec_head -> LOGITS
    HIPC(launch_rmsnorm(X + (size_t)(ch - 1) * H, ch * H, m->norm, s->LASTH, H, B, H, c.rms_eps, s->stream));
    LinArgs h;
    h.N = c.codec_vocab; h.K = H; set_w(h, m->codec_head, B, h.N, h.K); h.x = s->LASTH; h.ldx = H; h.y = s->LOGITS; h.ldy = c.codec_vocab;
    h.M = B; h.epi = EPI_NONE;
    HIPC(run_linear(s, h));
    HIPC(sync_frames(s));      // tmp buffers are freed on return
    return Q3_OK;
}

// Which kernels prefill an S-position prompt: the GEMM passes over [0, Sg) (or none), the decode-step schedule over the rest.
// The GEMM path works in 128-position tiles and its grids are sized to fill the chip in whole rounds (4096
// positions: 256 / 512 / 1536 workgroups of 256 CUs' worth); a few positions past the last full tile would cost every
// GEMM another round (4105 positions, one sequence: +9 ... +50 % per GEMM). Up to Q3_PREFILL_TAIL (default 32)
// trailing positions of a >= 1024-position prompt therefore go through the decode-step schedule instead (about
// 1 ms per 16 rows at 4k context), which appends to the same KV cache. The rule looks at the PROMPT only — never at the
// batch — so which kernels compute a given position does not depend on how many sequences are prefilled together
// (a batch pays ceil(B * r / 16) passes for it; positions below the cut always take the GEMM, whose bits are
// batch-invariant; the decode-step kernels pick their tiling by the row count of a pass, like any decode step).
static bool prefill_cut_of(const q3_model* m, int S, int* Sg) {
    static const int gemm_min = [] { const char* e = getenv("Q3_PREFILL_GEMM_MIN"); return e ? atoi(e) : 48; }();   // 0 disables the GEMM path
    static const int tail_max = [] { const char* e = getenv("Q3_PREFILL_TAIL"); return e ? atoi(e) : 32; }();
    *Sg = 0;
    if (gemm_min <= 0 || S < gemm_min || !d_nh_ok(m->cfg)) return false;
    const int r = S % 128;
    *Sg = (S >= 1024 && r > 0 && r <= tail_max) ? S - r : S;
    return true;
}
static bool prefill_cut(const q3_session* s, int S, int* Sg) {
    *Sg = 0;
    return !s->no_chunk && !s->debug && prefill_cut_of(s->m, S, Sg);
}
static int prefill_step_chunk(const q3_session* s) { return s->no_chunk ? 1 : (16 / s->B > 0 ? 16 / s->B : 1); }

// ---- prefix cache (q3_prefix_cache.h): what a session asks of it ----
// Eligible (PromptShape::prefix_pages): the instruct positions of a VoiceDesign row, in whole pages — the only prompt positions
// whose input is a pure function of the cache key. Never for debug / profile / no_chunk sessions or contiguous K/V.
static bool prefix_session_ok(const q3_session* s) { return prefix_on(s->m) && s->paged && !s->debug && !s->profile && !s->no_chunk; }
static int prefix_eligible_pages(const SeqInfo& q) { return prompt_shape(q.request()).prefix_pages; }
// The regime of this session's prefill: everything besides the token ids that decides the BITS of a cached position.
//   GEMM path: which attention kernel the prompt length selects (below 256 positions / bf16x3 / bf16x3 with key halves). With
//   key halves a query block's half boundary comes from the block's last position. At GQA ratio 2 a block is 128 rows = one
//   page, chunks start at multiples of 128, and every eligible page is a whole block: its last position is the page's, whatever
//   the prompt length or the chunk length — prompts of different lengths share pages. At ratio 1 a block is 256 rows: the block
//   a cached page lies in can end with the prompt or the chunk, and chunks of an odd number of pages shift the blocks, so Sg
//   and, when there is more than one chunk, the chunk length are part of the regime there.
//   Decode-step path (no GEMM geometry for the model): session width, key splits and prompt length.
static PrefixRegime prefix_regime_of(const q3_model* m, int B, int S, int n_splits) {
    PrefixRegime rg; int Sg = 0;
    if (prefill_cut_of(m, S, &Sg)) {
        const int C = prefill_gemm_chunk(B);
        const char* x3e = getenv("Q3_PREFILL_ATTN_X3");
        rg.v[0] = 1; rg.v[1] = Sg >= 1024 ? 2 : (Sg >= 256 ? 1 : 0);
        const bool wide_blk = 256 / (m->cfg.n_heads / m->cfg.n_kv_heads) > KV_PAGE_POS;      // blocks of more than one page
        rg.v[2] = (rg.v[1] == 2 && wide_blk) ? Sg : 0; rg.v[3] = (rg.v[1] == 2 && wide_blk && Sg > C) ? C : 0;
        rg.v[4] = (x3e && atoi(x3e) == 0) ? 1 : 0;
    } else { rg.v[0] = 2; rg.v[1] = B; rg.v[2] = n_splits; rg.v[3] = S; }
    return rg;
}
static PrefixRegime prefix_regime(const q3_session* s) { return prefix_regime_of(s->m, s->B, s->prefill_len, s->n_splits); }
// How many of `pages` cached pages a row may link so that the rest of the prompt is computed with the cuts of the uncached run.
//   GEMM path: the passes start at a block boundary of the chunk the first uncached position lies in (blocks are 256 / ratio
//   rows with the bf16x3 attention, 128 / ratio below 256 positions; chunks start at multiples of the chunk length). When every
//   GEMM position is cached no pass runs and nothing is rounded.
//   Decode-step path: the passes of 16 / B positions start at a multiple of that.
static int prefix_usable_pages_of(const q3_model* m, int B, int S, int pages) {
    int Sg = 0; const int P = pages * KV_PAGE_POS;
    if (prefill_cut_of(m, S, &Sg)) {
        if (P >= Sg) return Sg / KV_PAGE_POS;
        const int C = prefill_gemm_chunk(B), nrep = m->cfg.n_heads / m->cfg.n_kv_heads;
        const int blk = (Sg >= 256 ? 256 : 128) / nrep, c0 = (P / C) * C;
        const int P1 = c0 + ((P - c0) / blk) * blk;
        return P1 / KV_PAGE_POS;      // (blk < 128 never occurs: the GEMM path takes ratios 1 and 2 only)
    }
    const int ch = 16 / B > 0 ? 16 / B : 1;      // prefill_step_chunk of a session the cache serves (never no_chunk)
    int g = ch, r = KV_PAGE_POS; while (r) { const int t = g % r; g = r; r = t; }      // gcd(chunk, 128)
    const int step = KV_PAGE_POS / g * ch;
    return (P / step) * step / KV_PAGE_POS;
}
static int prefix_usable_pages(const q3_session* s, int pages) { return prefix_usable_pages_of(s->m, s->B, s->prefill_len, pages); }

static q3_status prefill_ragged(q3_session* s);
// Looks every row up and links what the session can use. Returns the number of positions the session's rows skip (the same for
// every row: rows of one batched prefill run through the same passes), or -1 when the rows hit differently and the session
// should prefill them in groups instead (prefill_ragged: each group a side session of its own width).
static int prefix_link(q3_session* s, q3_status* st) {
    *st = Q3_OK;
    const int B = s->B; q3_model* m = s->m;
    const PrefixRegime rg = prefix_regime(s);
    int kmin = 0x7fffffff, kmax = 0; bool opened = false;      // in pages the session can USE (chains of 9 and 8 pages both use 8 at ratio 1)
    for (int b = 0; b < B; ++b) {
        const SeqInfo& q = s->seq[(size_t)b];
        const int el = prefix_eligible_pages(q);
        const int k = (el > 0 && s->kv_rows[(size_t)b].empty()) ? prefix_usable_pages(s, prefix_peek(m, rg, q.instruct.data(), el)) : 0;
        kmin = std::min(kmin, k); kmax = std::max(kmax, k); opened = opened || q.opened;
    }
    if (kmin != kmax && !opened && !s->prefix_common) return -1;
    // (rows with open text, and the groups prefill_ragged has already formed, stay together: every row links what the row with
    // the shortest chain can — the bits of this session shape with the cache off)
    const int pages = kmin;
    bool short_of = false;
    for (int b = 0; b < B; ++b) {
        const SeqInfo& q = s->seq[(size_t)b];
        if (prefix_eligible_pages(q) < 1) continue;
        const int got = prefix_acquire(m, rg, q.instruct.data(), pages, s->kv_rows[(size_t)b]);      // (counts the lookup, also of a miss)
        short_of = short_of || got < pages;
    }
    if (pages < 1) return 0;
    if (short_of) {      // a block went between the two looks (another thread's eviction): this prefill runs from 0
        for (int b = 0; b < B; ++b) if (!s->kv_rows[(size_t)b].empty()) m->kv_pool.give(s->kv_rows[(size_t)b]);
        return 0;
    }
    for (int b = 0; b < B; ++b) {
        std::vector<float*>& row = s->kv_rows[(size_t)b];
        const hipError_t e = hipMemcpyAsync(s->kv_table + (size_t)b * KV_MAX_PAGES, row.data(), row.size() * 8, hipMemcpyHostToDevice, s->stream);
        if (e != hipSuccess) { *st = set_err(Q3_HIP_ERROR, "prefix cache: page table: %s", hipGetErrorString(e)); return 0; }
        s->seq[(size_t)b].reused = pages * KV_PAGE_POS;
    }
    return pages * KV_PAGE_POS;
}
// the rows of a one-length session as a ragged batch (prefix_link said -1): requests rebuilt from the rows' own copies
static void prefix_regroup(q3_session* s) {
    s->regrouped = true;      // transplant_row also brings each row's prompt embeddings (Q3_GET_PREFILL_EMBEDS stays valid)
    s->ragged.resize((size_t)s->B);
    for (int b = 0; b < s->B; ++b) s->ragged[(size_t)b].own(s->seq[(size_t)b].request(), s->m->cfg.hidden);
}

// q3_session_prefill in its three parts — stage the inputs, run the layers, finish — so that a packed pass (prefill_ragged) can run
// the middle part once for several one-row side sessions. What the staged uploads read lives in PrefillStaged until the finish.
struct PrefillStaged {
    std::vector<uint32_t> ids; std::vector<int> text_row, codec_id, trail_base, trail_len, pad_row, ready_v, limit_v; std::vector<float> xv;
    int P0 = 0; bool cached = false, regroup = false;      // regroup: the rows hit the prefix cache differently (prefix_link said -1)
};
static q3_status prefill_stage(q3_session* s, PrefillStaged& g);
static q3_status prefill_layers(q3_session* s, int P0);
static q3_status prefill_finish(q3_session* s, const PrefillStaged& g);

// Which rows of a ragged first batch share a packed pass: pure host arithmetic. A row packs when the GEMM path may
// run (gemm_ok), 48 <= length < 1024 (prefill_cut_of then gives Sg == S, and there are no key halves), it plans no prefix hit
// and is not barred by ok_row; packs form in row order and close when the next row would pass the budget; a pack of
// one row (a row longer than the budget always ends as one) is no pack. pass[b] = the row's pass or -1 (today's equal-length groups), row0[b] = its first activation row in the pass.
static int pack_plan(const int32_t* len, const int32_t* hit, const char* ok_row, int n, int budget, bool gemm_ok, int32_t* pass, int32_t* row0) {
    int n_pass = 0, first = -1, count = 0, total = 0;
    auto close = [&] {
        if (count >= 2) ++n_pass;
        else if (count == 1) { pass[first] = -1; row0[first] = 0; }
        count = 0; total = 0;
    };
    for (int b = 0; b < n; ++b) {
        pass[b] = -1; row0[b] = 0;
        if (!gemm_ok || len[b] < 48 || len[b] >= 1024 || (hit && hit[b] != 0) || (ok_row && !ok_row[b])) continue;
        if (count > 0 && total + len[b] > budget) close();
        if (count == 0) first = b;
        pass[b] = n_pass; row0[b] = total; total += len[b]; ++count;
    }
    close();
    return n_pass;
}
extern "C" q3_status q3_prefill_pack_plan(const int32_t* lengths, const int32_t* hit_pages, int32_t n, int32_t row_budget, int32_t gemm_ok,
                                          int32_t* pass, int32_t* row0, int32_t* n_passes) {
    if (!lengths || !pass || !row0) return set_err(Q3_INVALID_ARG, "q3_prefill_pack_plan: null argument");
    if (n < 1) return set_err(Q3_INVALID_ARG, "q3_prefill_pack_plan: %d rows", n);
    if (row_budget < 128) return set_err(Q3_INVALID_ARG, "q3_prefill_pack_plan: row budget %d below one 128-row tile", row_budget);
    for (int b = 0; b < n; ++b) {
        if (lengths[b] < 1) return set_err(Q3_INVALID_ARG, "q3_prefill_pack_plan: row %d: %d positions", b, lengths[b]);
        if (hit_pages && hit_pages[b] < 0) return set_err(Q3_INVALID_ARG, "q3_prefill_pack_plan: row %d: %d hit pages", b, hit_pages[b]);
    }
    const int np = pack_plan(lengths, hit_pages, nullptr, n, row_budget, gemm_ok != 0, pass, row0);
    if (n_passes) *n_passes = np;
    return Q3_OK;
}
extern "C" q3_status q3_session_prefill_info(const q3_session* s, int32_t info[8]) {
    if (!s || !info) return set_err(Q3_INVALID_ARG, "q3_session_prefill_info: null argument");
    for (int i = 0; i < 8; ++i) info[i] = s->prefill_info[i];
    return Q3_OK;
}
// the row budget of a pack: prefill_gemm_chunk's, read per call (a pack is one chunk)
static int pack_row_budget() {
    const char* e = getenv("Q3_PREFILL_ROWS");
    const int r = e ? atoi(e) : 4224;
    return r < 128 ? 128 : r;
}
// may this session's ragged rows pack at all (the per-row conditions are pack_plan's)
static bool pack_session_ok(const q3_session* s) {
    const char* e = getenv("Q3_PREFILL_PACK");           // read per call; 0 = the grouped path
    if (e && atoi(e) == 0) return false;
    if (!s->paged || s->debug || s->profile || s->no_chunk || !d_nh_ok(s->m->cfg)) return false;
    // the attention A/B aids select kernels the packed launches do not have
    for (const char* k : {"Q3_PREFILL_ATTN_VALU", "Q3_PREFILL_ATTN_GEN2", "Q3_PREFILL_ATTN_NOSPLIT", "Q3_GEMM_NO_PLANES"}) if (getenv(k)) return false;
    return true;
}

// q3_session_prefill of a ragged first batch (session_create_any): the idle rows never run — every row's state comes from a side
// session. Rows whose prompts take the GEMM path from position 0 share packed passes (pack_plan): each is the one-row
// side session of a batch-1 run, staged and finished by that run's own code, and only the layers run once for all of them. The
// other rows are grouped by prefill length in row order; a group of G rows is one batched side prefill.
static q3_status prefill_ragged(q3_session* s) {
    if (s->debug || s->profile) return set_err(Q3_UNSUPPORTED, "debug / profiling sessions need rows of one prefill length");
    const int B = s->B;
    for (int& v : s->prefill_info) v = 0;
    s->kv_in_bf16 = s->kv_bf16;                          // the idle rows hold no pages: nothing to convert
    s->prefilled = true; s->frames_run = 0; s->codes_host_valid = false;      // transplant_row stamps rows with start_run = frames_run
    std::vector<char> placed((size_t)B, 0);
    // prefix cache: rows of one length that would reuse different numbers of cached pages go into different groups (a batched
    // prefill runs all its rows through the same passes). The look is a plan only: each side session looks again and links.
    std::vector<int> hit((size_t)B, 0);
    // The plan takes the regime and the rounding of a one-row group (the width of a group is not known before the groups are);
    // where those depend on the width — the decode-step path, several chunks at ratio 1 — a group may link less than planned:
    // its side session links what its shortest chain allows (prefix_common), which keeps the bits right and only costs hits.
    std::vector<PromptShape> shape((size_t)B);
    for (int b = 0; b < B; ++b) shape[(size_t)b] = prompt_shape(s->ragged[(size_t)b].r);
    if (prefix_session_ok(s))
        for (int b = 0; b < B; ++b) {
            const q3_request& r = s->ragged[(size_t)b].r;
            const int el = shape[(size_t)b].prefix_pages, S = shape[(size_t)b].prefill_len;
            if (el > 0) hit[(size_t)b] = prefix_usable_pages_of(s->m, 1, S, prefix_peek(s->m, prefix_regime_of(s->m, 1, S, s->n_splits), r.instruct_ids, el));
        }
    // a failure leaves the session un-prefilled and holding no page (rows of earlier passes were moved in already)
    auto fail = [&](q3_status st) {
        (void)sync_frames(s);
        for (int b = 0; b < B; ++b) kv_release_row(s, b);
        s->prefilled = false;
        for (int& v : s->prefill_info) v = 0;
        return st;
    };
    auto row_limit = [&](int b, int* Lb) -> q3_status {
        // the row's RESOLVED limit (PromptShape::limit: under the ICL cap) is what session_create_any sized max_frames for — the
        // raw max_length of an ICL row may well exceed it
        const q3_request& r = s->ragged[(size_t)b].r;
        *Lb = shape[(size_t)b].limit;
        if (r.opts.max_length < 1 || *Lb < 1 || *Lb > s->max_frames) return set_err(Q3_INVALID_ARG, "row %d: max_length %d (resolved %d) outside 1..%d", b, r.opts.max_length, *Lb, s->max_frames);
        return Q3_OK;
    };
    // ---- packed passes ----
    std::vector<int32_t> pass((size_t)B, -1), row0((size_t)B, 0);
    int n_pass = 0;
    if (pack_session_ok(s)) {
        std::vector<int32_t> len((size_t)B); std::vector<char> ok((size_t)B, 1);
        for (int b = 0; b < B; ++b) {
            int Sg = 0; const int S = len[(size_t)b] = shape[(size_t)b].prefill_len;
            // the row's own prefill must be ONE GEMM pass over [0, S): what the pack reproduces
            ok[(size_t)b] = prefill_cut_of(s->m, S, &Sg) && Sg == S && S <= prefill_gemm_chunk(1);
        }
        n_pass = pack_plan(len.data(), hit.data(), ok.data(), B, pack_row_budget(), true, pass.data(), row0.data());
    }
    for (int p = 0; p < n_pass; ++p) {
        std::vector<int> rows;
        for (int b = 0; b < B; ++b) if (pass[(size_t)b] == p) rows.push_back(b);
        const size_t n = rows.size();
        std::vector<std::unique_ptr<q3_session>> side(n); std::vector<PrefillStaged> staged(n); std::vector<int> lim(n, 0);
        q3_status st = Q3_OK;
        for (size_t j = 0; j < n && st == Q3_OK; ++j) {
            int Lb = 0;
            st = row_limit(rows[j], &Lb);
            if (st == Q3_OK) st = side_prefill(s, &s->ragged[(size_t)rows[j]].r, &Lb, 1, false, false, true, s->stream, &side[j], &lim[j], nullptr, true);
            if (st == Q3_OK) st = prefill_stage(side[j].get(), staged[j]);
            placed[(size_t)rows[j]] = 1;
        }
        // a row that links cached pages after all (the plan was only a look) starts at P0 > 0: it runs its own layers
        PrefillPack pk; std::vector<int> plen, ptrow, pkern;
        for (size_t j = 0; j < n && st == Q3_OK; ++j) {
            if (staged[j].P0 > 0 || staged[j].regroup) continue;
            const int S = side[j]->prefill_len;
            pk.side.push_back(side[j].get()); plen.push_back(S); ptrow.push_back((int)pk.side.size() - 1);
            pkern.push_back(prefill_x3_on() && S >= 256 ? AP_X3 : AP_T);      // the kernel its length selects when prefilled alone
        }
        if (st == Q3_OK && pk.side.size() >= 2) {
            const LmDims d = talker_dims(s->m->cfg);
            if (!pack_host_build(plen.data(), ptrow.data(), pkern.data(), (int)plen.size(), d.nh, d.nkv, &pk.host)) st = set_err(Q3_INVALID_ARG, "packed prefill: tables");
            if (st == Q3_OK) st = prefill_gemm(s, 0, 0, true, 0, &pk);
            if (st == Q3_OK) {
                s->prefill_info[0] += 1; s->prefill_info[1] += 1; s->prefill_info[2] += (int)pk.side.size();
                s->prefill_info[3] = std::max(s->prefill_info[3], pk.host.rows);
            }
        }
        for (size_t j = 0; j < n && st == Q3_OK; ++j) {
            const bool packed = pk.side.size() >= 2 && std::find(pk.side.begin(), pk.side.end(), side[j].get()) != pk.side.end();
            if (staged[j].regroup) { st = set_err(Q3_INVALID_ARG, "packed prefill: a one-row side session cannot regroup"); break; }
            if (!packed) { st = prefill_layers(side[j].get(), staged[j].P0); s->prefill_info[0] += 1; s->prefill_info[4] += 1; }
            if (st == Q3_OK) st = prefill_finish(side[j].get(), staged[j]);
        }
        if (st == Q3_OK && sync_frames(s) != hipSuccess) st = set_err(Q3_HIP_ERROR, "ragged prefill: stream");
        for (size_t j = 0; j < n && st == Q3_OK; ++j) st = transplant_row(s, rows[j], side[j].get(), 0, lim[j]);
        if (st != Q3_OK) { (void)sync_frames(s); return fail(st); }      // (the stream is drained before the staged vectors and the side sessions go)
    }
    // ---- equal-length groups ----
    for (int b0 = 0; b0 < B; ++b0) {
        if (placed[(size_t)b0]) continue;
        std::vector<int> rows; std::vector<q3_request> reqs; std::vector<int> limits;
        for (int b = b0; b < B; ++b) {
            if (placed[(size_t)b] || shape[(size_t)b].prefill_len != shape[(size_t)b0].prefill_len || hit[(size_t)b] != hit[(size_t)b0]) continue;
            const q3_request& r = s->ragged[(size_t)b].r;
            int Lb = 0;
            const q3_status ls = row_limit(b, &Lb);
            if (ls != Q3_OK) return fail(ls);
            limits.push_back(Lb);
            rows.push_back(b); reqs.push_back(r); placed[(size_t)b] = 1;
        }
        std::unique_ptr<q3_session> side; std::vector<int> lim(rows.size(), 0);
        q3_status st = side_prefill(s, reqs.data(), limits.data(), (int)reqs.size(), false, false, true, s->stream, &side, lim.data());
        if (st == Q3_OK && sync_frames(s) != hipSuccess) st = set_err(Q3_HIP_ERROR, "ragged prefill: stream");
        for (size_t j = 0; j < rows.size() && st == Q3_OK; ++j) st = transplant_row(s, rows[j], side.get(), (int)j, lim[j]);
        if (st != Q3_OK) return fail(st);
        s->prefill_info[0] += 1; s->prefill_info[4] += (int)rows.size();
    }
    s->ragged.clear();
    return Q3_OK;
}

static q3_status frame_capture(q3_session* s, bool stream_busy);
static q3_status prefill_stage(q3_session* s, PrefillStaged& g) {
    const q3_model* m = s->m; const q3_config& c = m->cfg;
    const int B = s->B, H = c.hidden, S = s->prefill_len;
    // prefix cache: the rows link the cached pages of their instructions and the prompt is computed from position P0 on
    const bool cached = g.cached = prefix_session_ok(s);
    int& P0 = g.P0;
    if (cached) {
        // a prefill that failed after linking (a later row's Q3_KV_OVERFLOW) left pages in the rows: they go back first, so that
        // this attempt links again instead of computing [0, P) into pages the cache and other rows hold
        bool leftover = false;
        for (int b = 0; b < B; ++b) leftover = leftover || !s->kv_rows[(size_t)b].empty();
        if (leftover) {
            HIPC(sync_frames(s));
            for (int b = 0; b < B; ++b) { kv_release_row(s, b); s->seq[(size_t)b].reused = 0; }
        }
        q3_status lst = Q3_OK;
        P0 = prefix_link(s, &lst);
        Q3C(lst);
        if (P0 < 0) { g.regroup = true; return Q3_OK; }      // rows that hit differently: each group keeps the bits of its own run
    }
    for (int b = 0; b < B; ++b) Q3C(kv_reserve_row(s, b, S + 1));      // paged KV: the prompt's positions and the first frame's
    // 1. ids to project, per sequence: [instruct…, IM_START, ASSISTANT, NEWLINE, TTS_PAD, TTS_BOS, text…, TTS_EOS]
    std::vector<uint32_t>& ids = g.ids; ids.clear(); ids.reserve(s->n_rows_total);
    std::vector<int>& text_row = g.text_row; std::vector<int>& codec_id = g.codec_id;
    text_row.assign((size_t)B * S, -1); codec_id.assign((size_t)B * S, -1);
    std::vector<int>& trail_base = g.trail_base; std::vector<int>& trail_len = g.trail_len; std::vector<int>& pad_row = g.pad_row;
    trail_base.assign((size_t)B, 0); trail_len.assign((size_t)B, 0); pad_row.assign((size_t)B, 0);
    std::vector<float>& xv = g.xv; xv.assign((size_t)B * H, 0.0f);
    for (int b = 0; b < B; ++b) {
        SeqInfo& q = s->seq[b];
        for (uint32_t id : q.instruct) ids.push_back(id);
        ids.push_back(IM_START); ids.push_back(ASSISTANT); ids.push_back(NEWLINE); ids.push_back(TTS_PAD); ids.push_back(TTS_BOS);
        for (uint32_t id : q.ref_text) ids.push_back(id);      // (ICL rows alone hold one)
        for (uint32_t id : q.text) ids.push_back(id);
        ids.push_back(TTS_EOS);
        const q3_request r = q.request();
        const PromptShape sh = prompt_shape(r);
        if (sh.prefill_len != S) return set_err(Q3_INVALID_ARG, "prefill: row %d has %d positions, the session %d", b, sh.prefill_len, S);
        q.pad_row = q.row_base + sh.r_pad; q.trail_base = q.row_base + sh.trail_base;
        if (q.opened) { q.trail_base = slot_row0(s, b); open_counts(q); }      // open text: trailing rows in the row's slot (below)
        trail_base[b] = q.trail_base; trail_len[b] = q.trailing_len; pad_row[b] = q.pad_row;
        prompt_positions(sh, r, q.row_base, &text_row[(size_t)b * S], &codec_id[(size_t)b * S]);
        if (!q.xvec.empty()) memcpy(&xv[(size_t)b * H], q.xvec.data(), (size_t)H * 4);
    }
    uint32_t* ids_dev = s->ids_dev; int *tr_dev = s->tr_dev, *ci_dev = s->ci_dev;
    if ((int)ids.size() != s->n_rows_total) return set_err(Q3_INVALID_ARG, "prefill: row count mismatch (%zu vs %d)", ids.size(), s->n_rows_total);
    // reference frames of ICL sequences (also needed later by the ICL decode)
    std::vector<size_t> ref_off(B, 0); size_t ref_total = 0;
    for (int b = 0; b < B; ++b) { ref_off[b] = ref_total; ref_total += s->seq[b].ref_codes.size(); }
    if (ref_total && !s->ref_codes_dev) {
        HIPC(s->pool.alloc(&s->ref_codes_dev, ref_total));
        for (int b = 0; b < B; ++b)
            if (!s->seq[b].ref_codes.empty())
                HIPC(q3_hipMemcpy(s->ref_codes_dev + ref_off[b], s->seq[b].ref_codes.data(), s->seq[b].ref_codes.size() * 4, hipMemcpyHostToDevice));
    }
    // uploads ride the session stream (the host vectors live in PrefillStaged until the synchronisation that ends the prefill)
    HIPC(hipMemcpyAsync(ids_dev, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(tr_dev, text_row.data(), text_row.size() * 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(ci_dev, codec_id.data(), codec_id.size() * 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->xvec, xv.data(), xv.size() * 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->trail_base, trail_base.data(), B * 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->trail_len, trail_len.data(), B * 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->pad_row, pad_row.data(), B * 4, hipMemcpyHostToDevice, s->stream));
    q3_status st = text_project(s, ids_dev, (int)ids.size(), s->rows);
    if (st == Q3_OK) {
        hipError_t e = hipSuccess;
        for (int b = 0; b < B && e == hipSuccess; ++b)
            e = launch_assemble_rows(s->rows, tr_dev + (size_t)b * S, m->codec_emb, ci_dev + (size_t)b * S, s->xvec + (size_t)b * H,
                                     s->embeds + (size_t)b * S * H, S, H, s->stream,
                                     s->ref_codes_dev ? s->ref_codes_dev + ref_off[b] : nullptr, m->cp_embs_dev);
        if (e != hipSuccess) st = set_err(Q3_HIP_ERROR, "prefill assembly: %s", hipGetErrorString(e));
    }
    std::vector<int>& ready_v = g.ready_v; std::vector<int>& limit_v = g.limit_v;
    ready_v.clear(); limit_v.clear();
    if (st == Q3_OK && s->text_ready) {
        // open rows: the trailing rows received so far (+ tts_eos if the text closed before the prefill) go through the appended
        // rows' projection path, whatever arrived when; text_ready / limit of every row published with the rest
        for (int b = 0; b < B && st == Q3_OK; ++b) {
            const SeqInfo& q = s->seq[b];
            if (!q.opened) continue;
            std::vector<uint32_t> t; open_trailing_ids(q, t);
            if (q.text_closed) t.push_back(TTS_EOS);
            st = project_appended(s, b, t, 0);
        }
        for (int b = 0; b < B; ++b) { ready_v.push_back(s->seq[b].ready); limit_v.push_back(s->seq[b].limit); }
        if (st == Q3_OK) {
            hipError_t e = hipMemcpyAsync(s->text_ready, ready_v.data(), B * 4, hipMemcpyHostToDevice, s->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(s->limit, limit_v.data(), B * 4, hipMemcpyHostToDevice, s->stream);
            if (e != hipSuccess) st = set_err(Q3_HIP_ERROR, "prefill: open text state: %s", hipGetErrorString(e));
        }
    }
    if (st != Q3_OK) { (void)sync_frames(s); return st; }
    return Q3_OK;
}
static q3_status prefill_layers(q3_session* s, int P0) {
    const int B = s->B, H = s->m->cfg.hidden, S = s->prefill_len;
    // 2. run_prefill_layers (talker.rs:823-841): causal attention ⇒ token-by-token decode steps
    //    and the GEMV kernels take up to 16 rows for the price of one, so each weight pass carries a CHUNK of
    //    16/B consecutive positions per sequence (q3_kernels.h AttnArgs::rows_per_seq). Bit-identical to the
    //    one-position-at-a-time schedule (rows are independent in the GEMV; attention sees the same K/V).
    //    Long prompts run their first Sg positions as GEMM passes and only a short tail here (prefill_cut). Positions below P0
    //    are in linked pages already: neither schedule computes them again.
    const int chunk = prefill_step_chunk(s);
    int t_begin = P0, Sg = 0;
    if (prefill_cut(s, S, &Sg)) {
        if (P0 < Sg) Q3C(prefill_gemm(s, S, Sg, Sg == S, P0));
        t_begin = Sg;
    }
    for (int t0 = t_begin; t0 < S; t0 += chunk) {
        const int ch = (S - t0) < chunk ? (S - t0) : chunk;
        for (int b = 0; b < B; ++b)
            HIPC(launch_copy_rows(s->embeds + ((size_t)b * S + t0) * H, H, s->tb.X + (size_t)b * ch * H, H, ch, H, s->stream));
        Q3C(talker_step(s, nullptr, t0, t0 + ch >= S, ch));
    }
    return Q3_OK;
}
static q3_status prefill_finish(q3_session* s, const PrefillStaged& g) {
    const int B = s->B, S = s->prefill_len; const bool cached = g.cached;
    // 3. first sampling decision (lib.rs:558-571)
    std::vector<int> posv(B, S), zero(B, 0);
    HIPC(hipMemcpyAsync(s->pos, posv.data(), B * 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->frame_idx, zero.data(), B * 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->token_count, zero.data(), B * 4, hipMemcpyHostToDevice, s->stream));
    SampleArgs a; fill_sample_args(s, a); a.advance = 0;
    HIPC(launch_sample(a, s->stream));
    // Callers that are going to replay the frame (q3_session_run, q3_session_next_chunk) have it captured and converted HERE, while
    // the prompt's kernels run: ~2 ms of host work that used to sit between the prefill and the first frame (time to first audio).
    // (bf16-KV sessions capture later: which attention kernel the frame holds depends on the conversion below.)
    if (s->precapture && !s->kv_bf16 && !s->debug && !s->profile) Q3C(frame_capture(s, true));
    HIPC(sync_frames(s));
    if (cached) {      // the stream is drained: the rows' eligible pages that are not cached yet get a second holder, the cache (no copy)
        const PrefixRegime rg = prefix_regime(s);
        for (int b = 0; b < B; ++b) {
            const SeqInfo& q = s->seq[(size_t)b];
            const int el = prefix_eligible_pages(q);
            if (el > 0 && (int)s->kv_rows[(size_t)b].size() >= el) prefix_insert(s->m, rg, q.instruct.data(), el, s->kv_rows[(size_t)b].data());
        }
    }
    if (s->kv_bf16 && !s->kv_in_bf16) Q3C(kv_convert_to_bf16(s));       // the prompt's K/V moves into pages of the bf16 pool, once
    s->prefilled = true; s->frames_run = 0; s->codes_host_valid = false;
    return Q3_OK;
}
extern "C" q3_status q3_session_prefill(q3_session* s) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (s->prefilled) return set_err(Q3_INVALID_ARG, "session already prefilled");
    HIPC(hipSetDevice(s->m->device));
    if (!s->ragged.empty()) return prefill_ragged(s);
    PrefillStaged g;
    Q3C(prefill_stage(s, g));
    if (g.regroup) { prefix_regroup(s); return prefill_ragged(s); }
    Q3C(prefill_layers(s, g.P0));
    return prefill_finish(s, g);
}

static q3_status refresh_codes(q3_session* s) {
    if (s->codes_host_valid) return Q3_OK;
    HIPC(sync_frames(s));
    s->codes_host.resize((size_t)s->B * s->max_frames * 16);
    if (s->text_ready) {          // opened rows (a held row ran frames it did not commit): their count is the device frame_idx
        std::vector<int> fi((size_t)s->B);
        HIPC(q3_hipMemcpy(fi.data(), s->frame_idx, s->B * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < s->B; ++b) if (s->seq[b].opened) s->seq[b].committed = fi[(size_t)b];
    }
    auto ran_of = [s](const SeqInfo& q) { return q.opened ? q.committed : s->frames_run - q.start_run; };
    for (int b = 0; b < s->B; ++b) {
        int ran = ran_of(s->seq[b]);
        if (ran > s->seq[b].limit) ran = s->seq[b].limit;
        if (ran > 0)
            HIPC(q3_hipMemcpy(&s->codes_host[(size_t)b * s->max_frames * 16], s->codes + (size_t)b * s->max_frames * 16,
                           (size_t)ran * 16 * 4, hipMemcpyDeviceToHost));
    }
    std::vector<uint32_t> tok(s->B);
    HIPC(q3_hipMemcpy(tok.data(), s->tok, s->B * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < s->B; ++b) {
        SeqInfo& q = s->seq[b];
        int n = ran_of(q); bool done = false;      // frames this row has run (rows swapped in later started later)
        if (n > q.limit) n = q.limit;
        if (n < 0) n = 0;
        const int eos = q.req.opts.eos_token_id;                     // per row (SampleRow)
        if (eos >= 0) {
            const int ran = n;
            for (int f = 0; f < ran; ++f)
                if ((int)s->codes_host[((size_t)b * s->max_frames + f) * 16] == eos) { n = f; done = true; break; }
            if (!done && ran < q.limit && (int)tok[b] == eos) done = true;     // EOS sampled for the next frame
        }
        if (n >= q.limit) done = true;
        q.n_frames = n; q.done = done;
    }
    s->codes_host_valid = true;
    return Q3_OK;
}

q3_status session_refresh_codes(q3_session* s) { return refresh_codes(s); }
static bool all_done(q3_session* s) { for (auto& q : s->seq) if (!q.done) return false; return true; }
// frames the session still has to run for its longest-remaining row (lockstep sessions: max_frames - frames_run)
// An opened row can commit frames up to what its text allows; a held or finished one none.
static int row_capacity(const q3_session* s, const SeqInfo& q) {
    if (!q.opened) return q.limit - (s->frames_run - q.start_run);
    if (q.done) return 0;
    return std::min(q.ready, q.limit) - q.committed;
}
static int session_remaining(const q3_session* s) {
    int r = 0;
    for (const auto& q : s->seq) { const int left = row_capacity(s, q); if (left > r) r = left; }
    return r;
}
// n more frames were handed to the device: what each opened row commits of them (k_sample holds it at text_ready, freezes it at limit)
static void open_rows_ran(q3_session* s, int n) {
    for (auto& q : s->seq)
        if (q.opened) { const int stop = std::max(q.committed, std::min(q.ready, q.limit)); q.committed = std::min(q.committed + n, stop); }
}

// ---- open text through the batcher (q3_batcher_submit_open) ----
// The hold path of a session that was created without an open row: text_ready and the append scratch are allocated, and a frame
// that was captured without the hold kernels is dropped — the next q3_session_generate captures it again, once. The caller has
// nothing of the session in flight.
q3_status session_text_enable(q3_session* s) {
    if (s->text_ready) return Q3_OK;
    if (s->debug || s->profile) return set_err(Q3_UNSUPPORTED, "open text: not on debug / profiling sessions");
    HIPC(hipSetDevice(s->m->device));
    HIPC(sync_frames(s));
    Q3C(alloc_text_state(s));
    if (s->aql) { q3::aql_program_destroy(s->aql); s->aql = nullptr; }
    s->aql_mode = 0; s->aql_tried = false;
    if (s->graph_exec) { (void)hipGraphExecDestroy(s->graph_exec); s->graph_exec = nullptr; }
    if (s->graph) { (void)hipGraphDestroy(s->graph); s->graph = nullptr; }
    return Q3_OK;
}
// frames row b can still commit with the text (and limit) it has; its committed count (the host's view: exact between two reads)
int session_row_remaining(const q3_session* s, int b) { const int r = row_capacity(s, s->seq[(size_t)b]); return r > 0 ? r : 0; }
int session_row_committed(const q3_session* s, int b) {
    const SeqInfo& q = s->seq[(size_t)b];
    int n = q.opened ? q.committed : s->frames_run - q.start_run;
    if (n > q.limit) n = q.limit;
    return n > 0 ? n : 0;
}
// The text flush: the pieces of ANY number of open rows are projected together and published together, with ONE
// synchronisation at the end (q3_session_append_text drains, projects and synchronises per call and row). The tokens (+ tts_eos
// of a row that closes) are packed across rows into groups of eight, the last padded with its last id as project_appended pads;
// every group takes project_group, and k_scatter_rows sends its rows to the slots they belong to. The caller has nothing of the
// session in flight. All or nothing: a piece that is refused leaves every row as it was.
q3_status session_append_many(q3_session* s, const std::vector<TextPiece>& pieces) {
    if (pieces.empty()) return Q3_OK;
    if (!s->text_ready) return set_err(Q3_INVALID_ARG, "text flush: the session has no open text state");
    const q3_config& c = s->m->cfg;
    for (const TextPiece& p : pieces) {
        if (p.b < 0 || p.b >= s->B || p.n < 0 || (p.n > 0 && !p.ids)) return set_err(Q3_INVALID_ARG, "text flush: bad piece");
        const SeqInfo& q = s->seq[(size_t)p.b];
        if (!q.opened || q.text_closed) return set_err(Q3_INVALID_ARG, "text flush: row %d is not open", p.b);
        for (int i = 0; i < p.n; ++i) if (p.ids[i] >= (uint32_t)c.text_vocab) return set_err(Q3_INVALID_ARG, "text id %u out of range", p.ids[i]);
        // (the last row of a transplanted open row's slot holds its tts_pad row: transplant_row)
        if (q.n_trail + p.n + 1 > s->row_cap - 1) return set_err(Q3_UNSUPPORTED, "text flush: %d trailing text rows exceed the row's slot (%d)", q.n_trail + p.n + 1, s->row_cap - 1);
    }
    HIPC(hipSetDevice(s->m->device));
    std::vector<int> ids, dst, pub;
    for (const TextPiece& p : pieces) {
        SeqInfo& q = s->seq[(size_t)p.b];
        const int row0 = q.trail_base + q.n_trail;
        for (int i = 0; i < p.n; ++i) { ids.push_back((int)p.ids[i]); dst.push_back(row0 + i); }
        if (p.last) { ids.push_back((int)TTS_EOS); dst.push_back(row0 + p.n); }
        q.text_all.insert(q.text_all.end(), p.ids, p.ids + p.n);
        if (p.last) q.text_closed = true;
        open_counts(q);
        const int e[4] = {p.b, q.trailing_len, q.ready, q.limit};
        pub.insert(pub.end(), e, e + 4);
    }
    while (ids.size() % 8 != 0) { ids.push_back(ids.back()); dst.push_back(-1); }
    const size_t n_src = ids.size(), n_pub = pub.size() / 4;
    // one upload: [ids | destinations | entries to publish]; the buffer grows by doubling and lives as long as the session
    std::vector<int> up(ids); up.insert(up.end(), dst.begin(), dst.end()); up.insert(up.end(), pub.begin(), pub.end());
    if (up.size() > s->flush_cap) {
        size_t cap = s->flush_cap ? s->flush_cap : 256;
        while (cap < up.size()) cap *= 2;
        HIPC(s->pool.alloc(&s->flush_buf, cap));
        s->flush_cap = cap;
    }
    hipError_t er = hipMemcpyAsync(s->flush_buf, up.data(), up.size() * 4, hipMemcpyHostToDevice, s->stream);      // (`up` lives until the synchronisation below)
    for (size_t g = 0; g < n_src && er == hipSuccess; g += 8) {
        er = project_group(s, (const uint32_t*)s->flush_buf + g);
        if (er == hipSuccess) er = launch_scatter_rows(s->app_out, s->flush_buf + n_src + g, s->rows, 8, c.hidden, s->stream);
    }
    if (er == hipSuccess) er = launch_publish_text(s->flush_buf + 2 * n_src, (int)n_pub, s->trail_len, s->text_ready, s->limit, s->stream);
    const hipError_t es = sync_frames(s);
    if (er == hipSuccess) er = es;
    s->codes_host_valid = false;
    if (er != hipSuccess) return set_err(Q3_HIP_ERROR, "text flush: %s", hipGetErrorString(er));
    return Q3_OK;
}

// Which kernels of the frame keep to the activation-transport rule of q3_kernels.h (write-through + drained stores, L1-bypassing
// loads of everything an earlier node of the same frame wrote, nothing of it through the scalar cache): their packets go out
// without the agent-scope acquire / release fences (q3_aql.h). Anything not named here keeps HIP's fences — a kernel added to
// the frame later is safe by default. Development switches: Q3_AQL_T_ACQ=0 / Q3_AQL_T_REL=0 keep that half of every boundary,
// Q3_AQL_T_ONLY=<substring+substring> restricts the rule to kernels whose name holds one of the substrings (bisecting).
static void frame_fence_policy(const char* name, int* acquire, int* release) {
    static const char* const families[] = {"k_gemv_mfmaI", "k_gemv_sk2I", "k_gemv_gu24I", "k_gemv_ldsI", "k_gemv_mfma4I",
                                           "k_attn_cpI", "k_attn_fusedI", "k_attn_mergeI", "k_attn_first2I"};
    const bool drop_acq = !(getenv("Q3_AQL_T_ACQ") && atoi(getenv("Q3_AQL_T_ACQ")) == 0);
    const bool drop_rel = !(getenv("Q3_AQL_T_REL") && atoi(getenv("Q3_AQL_T_REL")) == 0);
    const std::string only = getenv("Q3_AQL_T_ONLY") ? getenv("Q3_AQL_T_ONLY") : "";
    bool conv = false;
    for (const char* f : families) conv = conv || strstr(name, f) != nullptr;
    if (conv && !only.empty()) {
        bool hit = false; size_t i = 0;
        while (i <= only.size()) {
            const size_t j = only.find_first_of(",+", i); const std::string t = only.substr(i, j == std::string::npos ? std::string::npos : j - i);
            if (!t.empty() && strstr(name, t.c_str())) hit = true;
            if (j == std::string::npos) break;
            i = j + 1;
        }
        conv = hit;
    }
    if (!conv) return;
    if (drop_acq) *acquire = 0;
    if (drop_rel) *release = 0;
}

// The frame is captured ONCE per session (frame_launch under stream capture: every per-frame quantity lives in device memory, so
// the graph is static) and turned into the packet program of the library's own AQL queue (q3_aql.cpp); only a graph the converter
// cannot take — or Q3_AQL=0 — is instantiated for hipGraphLaunch. `stream_busy`: the caller has work queued on the session's
// stream that must NOT be waited for here (q3_session_prefill captures while the prompt's kernels run: capture, conversion and
// the kernarg upload are host work, ~2 ms that used to sit between the prefill and the first frame of every session).
// Q3_AQL unset / 3 (round 6: the default; the whole -m gpu suite runs through it): boundaries between kernels that keep to the
// activation-transport rule (q3_kernels.h) without HIP's agent-scope fences. Q3_AQL=0: hipGraphLaunch; 1: own queue with HIP's
// fences on every packet (bit-identical to 0); 2: probe. Why a graph stayed on hipGraphLaunch: Q3_AQL_VERBOSE=1.
static q3_status frame_capture(q3_session* s, bool stream_busy) {
    // RELAXED capture mode: the captured region is nothing but kernel launches on the session's own non-blocking stream, while OTHER
    // host threads — the batcher's prefill worker, a server opening sessions on several threads — allocate, hipMemcpy and touch the
    // null stream as they please: in thread-local (or global) mode this HIP runtime fails THEIR calls ("operation not permitted
    // when stream is capturing") and invalidates the capture (tests/test_frame_submission.py: two sessions on two threads). An
    // invalidated capture is repeated all the same.
    for (int attempt = 0; !s->graph; ++attempt) {
        if (!stream_busy) HIPC(sync_frames(s));
        std::unique_lock<std::shared_mutex> cap(q3_capture_mu());      // no legacy-stream operation of any thread while the capture is open (q3_engine.h)
        {
            const hipError_t eb = hipStreamBeginCapture(s->stream, hipStreamCaptureModeRelaxed);
            if (eb != hipSuccess && stream_busy) { (void)hipGetLastError(); return Q3_OK; }      // not now: q3_session_generate captures on the idle stream
            HIPC(eb);
        }
        const q3_status st = frame_launch(s);
        const hipError_t e = hipStreamEndCapture(s->stream, &s->graph);
        if (st == Q3_OK && e == hipSuccess && s->graph) break;
        if (s->graph) { (void)hipGraphDestroy(s->graph); s->graph = nullptr; }
        (void)hipGetLastError();
        if (attempt >= 3) { Q3C(st); return set_err(Q3_HIP_ERROR, "hipStreamEndCapture: %s", hipGetErrorString(e)); }
    }
    if (!s->aql && !s->aql_tried) {
        s->aql_tried = true;
        const char* e = getenv("Q3_AQL");
        int mode = e ? atoi(e) : 3;
        // Packets without ANY boundary fence give WRONG codes (state that crosses frames moves with plain accesses):
        // mode 2 and the fence halves are probes and need an explicit opt-in, so that a stray environment variable cannot
        // silently corrupt a server's output.
        const bool unsafe_ok = getenv("Q3_AQL_UNSAFE") && atoi(getenv("Q3_AQL_UNSAFE")) == 1;
        const bool wants_unsafe = mode == 2 || getenv("Q3_AQL_ACQ") || getenv("Q3_AQL_REL");
        if (wants_unsafe && !unsafe_ok) {
            static std::atomic<bool> told{false};
            if (!told.exchange(true)) fprintf(stderr, "[q3] Q3_AQL=2 / Q3_AQL_ACQ / Q3_AQL_REL drop kernel-boundary fences and produce wrong results with the product kernels; "
                                                      "ignored without Q3_AQL_UNSAFE=1 (frames stay on %s)\n", mode == 2 ? "hipGraphLaunch" : "HIP's fence policy");
            if (mode == 2) mode = 0;
        }
        if (mode > 0) {
            q3::AqlPolicy pol; pol.fence = mode == 2 ? 0 : 1;
            pol.acquire = pol.release = pol.fence;
            if (mode == 3) pol.node_policy = frame_fence_policy;      // fence-free boundaries between the kernels that move their data write-through
            if (unsafe_ok) {
                if (const char* a = getenv("Q3_AQL_ACQ")) pol.acquire = atoi(a);        // probes: the two fences of a boundary priced separately
                if (const char* r = getenv("Q3_AQL_REL")) pol.release = atoi(r);
                fprintf(stderr, "[q3] WARNING: Q3_AQL_UNSAFE=1: frames are submitted with acquire=%d release=%d — results are NOT valid with the product kernels\n", pol.acquire, pol.release);
            }
            std::string why;
            s->aql = q3::aql_program_create(s->graph, s->m->device, pol, &why);
            if (s->aql) {
                s->aql_mode = mode == 2 ? 2 : mode == 3 ? 3 : 1;
                if (const char* c = getenv("Q3_FRAME_CUS")) { std::string w; if (atoi(c) > 0) q3::aql_restrict_cus(s->aql, atoi(c), &w); }   // measurement aid: the queue keeps this mask
            } else if (getenv("Q3_AQL_VERBOSE")) fprintf(stderr, "[q3] AQL submission unavailable, staying on hipGraphLaunch: %s\n", why.c_str());
        }
    }
    if (!s->aql && !s->graph_exec) HIPC(hipGraphInstantiate(&s->graph_exec, s->graph, nullptr, nullptr, 0));
    return Q3_OK;
}
// `n` replays of the captured frame enqueued WITHOUT waiting for them (streaming read-ahead): on the own queue behind whatever it
// holds, or as graph launches on the session's stream. The caller reserved the K/V pages (kv_reserve_frames) and, on the own queue,
// made sure everything the first frame reads has landed (the queue is not ordered with the HIP stream). sync_frames waits for both.
static q3_status frames_enqueue(q3_session* s, int n) {
    if (n <= 0) return Q3_OK;
    if (s->aql) {
        std::string why; int handed = 0;
        const bool ok = q3::aql_submit(s->aql, n, &why, &handed);
        s->frames_run += handed; open_rows_ran(s, handed);
        if (!ok) { s->aql_failed = true; s->codes_host_valid = false; return set_err(Q3_HIP_ERROR, "AQL frame submission: %s", why.c_str()); }
    } else {
        if (!s->graph_exec) return set_err(Q3_INVALID_ARG, "frames_enqueue: no captured frame");
        for (int i = 0; i < n; ++i) HIPC(hipGraphLaunch(s->graph_exec, s->stream));
        s->frames_run += n; open_rows_ran(s, n);
    }
    s->codes_host_valid = false;
    return Q3_OK;
}

extern "C" q3_status q3_session_generate(q3_session* s, int n_frames, int use_graph) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (!s->prefilled) return set_err(Q3_INVALID_ARG, "session not prefilled");
    if (s->aql_failed) return set_err(Q3_HIP_ERROR, "session unusable: an earlier frame submission on the AQL queue failed or timed out");
    HIPC(hipSetDevice(s->m->device));
    if (s->debug || s->profile) use_graph = 0;
    int todo = n_frames;
    // open rows: no frame is replayed in which no row can commit — a burst is the most frames any row's text (or limit) allows,
    // nothing when every live row is held or done
    if (s->text_ready) Q3C(refresh_codes(s));
    { const int left = session_remaining(s); if (todo > left) todo = left; }
    if (todo <= 0) return Q3_OK;
    Q3C(kv_reserve_frames(s, todo));        // paged KV: every page these frames can reach, before the first of them is queued
    if (use_graph) Q3C(frame_capture(s, false));
    bool on_aql = use_graph && s->aql;
    if (on_aql) HIPC(sync_frames(s));     // the queue is not ordered with the HIP stream: prefill / swaps must have landed
    bool eos_on = false;
    for (const auto& q : s->seq) eos_on = eos_on || q.req.opts.eos_token_id >= 0;
    const int check_every = 32;
    while (todo > 0) {
        const int burst = eos_on ? (todo < check_every ? todo : check_every) : todo;
        if (on_aql) {
            // (a failed submission or wait marks the session failed: the ring may still hold — or run — packets that write this
            // session's buffers, so nothing may replay behind them; frames_run stays in step with what the device was given)
            q3_status st = frames_enqueue(s, burst);
            if (st == Q3_OK && sync_frames(s) != hipSuccess) st = Q3_HIP_ERROR;
            if (st != Q3_OK) { s->aql_failed = true; s->codes_host_valid = false; return st; }
        } else
        for (int i = 0; i < burst; ++i) {
            if (use_graph) HIPC(hipGraphLaunch(s->graph_exec, s->stream));
            else Q3C(frame_launch(s));
            s->frames_run += 1; open_rows_ran(s, 1);
        }
        todo -= burst;
        s->codes_host_valid = false;
        if (eos_on) { Q3C(refresh_codes(s)); if (all_done(s)) break; }
        if (s->text_ready) { const int left = session_remaining(s); if (todo > left) todo = left; }
    }
    HIPC(sync_frames(s));
    if (s->profile && !s->prof_events.empty()) {
        for (size_t i = 0; i < s->prof_events.size(); ++i) {
            float ms = 0; hipEventElapsedTime(&ms, s->prof_events[i].first, s->prof_events[i].second);
            s->prof_linear.ms += ms; s->prof_linear.bytes += s->prof_event_bytes[i]; s->prof_linear.launches += 1;
        }
        s->prof_events.clear(); s->prof_event_bytes.clear(); s->prof_pool_next = 0;
    }
    return Q3_OK;
}

// ---- streaming: one fill, one cut, one vocoder enqueue under the four chunk entries ----
// A row has ONE streaming position (SeqInfo::stream_pos: frames already handed out) and every entry follows it, so the entries
// may be mixed on a row: q3_session_next_chunk (one row, with read-ahead), q3_session_next_chunk_row, q3_session_next_chunks[_out].
static int chunk_frames_of(const q3_session* s) { return s->opts.chunk_frames > 0 ? s->opts.chunk_frames : 10; }
// Fill: generate until row b has a chunk buffered behind its position or ends (lib.rs:1663-1748). An opened row waits for its
// own text: it stops generating when it is held. (One row: session_remaining is max(row_capacity, 0), the same test.)
static q3_status chunk_fill(q3_session* s, int b) {
    const SeqInfo& q = s->seq[(size_t)b];
    const int chunk = chunk_frames_of(s);
    while (!q.done && q.n_frames - q.stream_pos < chunk && (q.opened ? row_capacity(s, q) : session_remaining(s)) > 0) {
        Q3C(q3_session_generate(s, chunk - (q.n_frames - q.stream_pos), 1));
        Q3C(refresh_codes(s));
    }
    return Q3_OK;
}
// Cut: what row b gets now. avail: frames (a chunk until the row ends, the rest then); held: an opened row whose text does not
// reach a whole chunk yet gets nothing now (chunk boundaries stay those of the closed run); ends: what `done` will report.
struct ChunkCut { int avail; bool held, ends; };
static ChunkCut chunk_cut(const q3_session* s, int b) {
    const SeqInfo& q = s->seq[(size_t)b];
    const int chunk = chunk_frames_of(s);
    int a = std::min(q.n_frames - q.stream_pos, chunk);
    const bool held = q.opened && !q.done && a < chunk;
    if (a < 0 || held) a = 0;
    return {a, held, !held && (a <= 0 || (q.done && q.stream_pos + a >= q.n_frames))};
}
// Vocode: the one range decode (vocode_enqueue, q3_codec_run.hip). A row's frames as it takes them: its codes on the device from frame f0; with_ref: behind the reference
// frames of an ICL row that was prefilled, from the host copy (a row swapped in by q3_session_replace brings its own) — their
// samples are cut (lib.rs:1022-1041)
static VocodeSrc row_src(const q3_session* s, int b, int f0 = 0, bool with_ref = false) {
    const SeqInfo& q = s->seq[(size_t)b];
    const bool ref = with_ref && s->prefilled && !q.ref_codes.empty();
    return {ref ? q.ref_codes.data() : nullptr, ref ? (int)(q.ref_codes.size() / 16) : 0, s->codes + ((size_t)b * s->max_frames + f0) * 16, false};
}
// context-free: frames [f0, f0 + T) of row b decoded as an utterance of their own (the reference's per-chunk decode, lib.rs:1755-1758)
static q3_status range_vocode_enqueue(q3_session* s, int b, int f0, int T, hipStream_t st, VocodePcm* pcm) {
    return vocode_enqueue(s->m, s->cws, st, row_src(s, b, f0), 0, T, 0, 0, pcm);
}
// frames [stream_pos, stream_pos + avail) of row b in the session's stream mode, enqueued on st; nothing is waited for
static q3_status chunk_vocode_enqueue(q3_session* s, int b, int avail, hipStream_t st, VocodePcm* pcm) {
    const SeqInfo& q = s->seq[(size_t)b];
    if (s->stream_mode != 1 || q.icl) return range_vocode_enqueue(s, b, q.stream_pos, avail, st, pcm);
    // continuous mode (q3_session_set_stream_mode): the chunk's samples are identical to the same frames of a whole-utterance decode
    Q3C(codec_reserve(s->m, s->cws, chunk_frames_of(s) + CODEC_CTX_FRAMES, s->max_frames));
    return vocode_enqueue(s->m, s->cws, st, row_src(s, b), q.stream_pos, q.stream_pos + avail, vocode_ctx_start(q.stream_pos), 0, pcm);
}
// the vocoder pass of one row's chunk on the session's stream
static q3_status chunk_decode_row(q3_session* s, int b, int avail, float* pcm_host, size_t cap, size_t* n_samples) {
    VocodePcm pcm;
    Q3C(chunk_vocode_enqueue(s, b, avail, s->stream, &pcm));
    HIPC(sync_frames(s));
    return vocode_copy_out(pcm, pcm_host, cap, n_samples, nullptr);
}

// Streaming with several sequences in one session: the next chunk of row b (StreamingSession::next_chunk, lib.rs:1650-1759,
// one per row). Rows advance in lockstep, so asking row after row costs the frames once: the first call generates them for
// every row, the others find theirs buffered and only run their vocoder. One row: q3_session_next_chunk (with read-ahead).
extern "C" q3_status q3_session_next_chunk_row(q3_session* s, int b, float* pcm_host, size_t cap, size_t* n_samples, int* done) {
    if (!s || b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "bad sequence index");
    HIPC(hipSetDevice(s->m->device));
    if (!s->prefilled) Q3C(q3_session_prefill(s));
    Q3C(refresh_codes(s));
    Q3C(chunk_fill(s, b));
    const ChunkCut cut = chunk_cut(s, b);
    if (n_samples) *n_samples = 0;
    if (cut.avail > 0) {
        Q3C(chunk_decode_row(s, b, cut.avail, pcm_host, cap, n_samples));
        s->seq[(size_t)b].stream_pos += cut.avail;
    }
    if (done) *done = cut.ends ? 1 : 0;
    return Q3_OK;
}

// q3_session_next_chunk_row for every row in one call. The frames come first, exactly as the per-row calls in row order would
// ask for them (generation does not depend on how it is cut into bursts, and a row's chunk is `chunk` frames until it ends and
// the rest then: the boundaries are the per-row calls'). Then one vocoder pass: in stream mode 1 every row that is not ICL
// goes through the session's codec stream (q3_codec_stream.hip) in ONE push — a chunk costs its own frames, not the utterance
// so far, and the launches do not multiply with the rows; ICL rows and stream mode 0 keep the per-row context-free decode.
// `out`: q3_session_next_chunks_out — the same rounds, every row's samples through its row of the session's output stage
// (out_host / cap in samples of the session's output); a row's stage row is flushed in the call that reports it done.
static q3_status next_chunks(q3_session* s, float* const* pcm_host, const size_t* cap, size_t* n_samples, int* done, bool out, void* const* out_host);
extern "C" q3_status q3_session_next_chunks(q3_session* s, float* const* pcm_host, const size_t* cap, size_t* n_samples, int* done) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (!n_samples || !done) return set_err(Q3_INVALID_ARG, "q3_session_next_chunks: n_samples and done are required");
    if (s->m->device < 0) return set_err(Q3_INVALID_ARG, "q3_session_next_chunks: the model has no device");
    return next_chunks(s, pcm_host, cap, n_samples, done, false, nullptr);
}
extern "C" q3_status q3_session_set_output(q3_session* s, uint32_t sample_rate, int format) {
    if (!s) return set_err(Q3_INVALID_ARG, "q3_session_set_output: null session");
    std::vector<OutSettings> next = s->out;
    for (OutSettings& o : next) Q3C(out_set_output("q3_session_set_output", o, sample_rate, format));
    if (s->m->device < 0) return set_err(Q3_INVALID_ARG, "q3_session_set_output: the model has no device");
    bool started = s->out_started;
    for (const SeqInfo& q : s->seq) started = started || q.stream_pos > 0;
    if (started) return set_err(Q3_INVALID_ARG, "q3_session_set_output: the session has streamed its first chunk: the output is set before it");
    s->out = next;
    return Q3_OK;
}
// The per-row setters (b = -1: every row): `edit` on a copy of each row's setting — no row changes unless every row accepts —, then
// the window, then the rows' settings and, where the stage exists, its rows. what: the setting's name in the window's refusal.
template <class Edit>
static q3_status session_set_rows(q3_session* s, int b, const char* who, const char* what, Edit edit) {
    if (!s) return set_err(Q3_INVALID_ARG, "%s: null session", who);
    if (b < -1 || b >= s->B) return set_err(Q3_INVALID_ARG, "%s: row %d out of range (%d rows; -1 = every row)", who, b, s->B);
    const int b0 = b < 0 ? 0 : b, b1 = b < 0 ? s->B : b + 1;
    std::vector<OutSettings> next(s->out.begin() + b0, s->out.begin() + b1);
    for (OutSettings& o : next) Q3C(edit(who, o));
    if (s->m->device < 0) return set_err(Q3_INVALID_ARG, "%s: the model has no device", who);
    for (int r = b0; r < b1; ++r)
        if (s->seq[(size_t)r].stream_pos > 0)
            return set_err(Q3_INVALID_ARG, "%s: row %d has streamed its first chunk: the %s is set before it, or after q3_session_replace", who, r, what);
    for (int r = b0; r < b1; ++r) {
        if (s->ostage) Q3C(pcm_stage_apply(s->ostage, r, who, next[(size_t)(r - b0)]));
        s->out[(size_t)r] = next[(size_t)(r - b0)];
    }
    return Q3_OK;
}
extern "C" q3_status q3_session_set_tempo(q3_session* s, int b, int tempo_permille) {
    return session_set_rows(s, b, "q3_session_set_tempo", "tempo", [&](const char* who, OutSettings& o) { return out_set_tempo(who, o, tempo_permille); });
}
extern "C" q3_status q3_session_set_pitch(q3_session* s, int b, int cents) {
    return session_set_rows(s, b, "q3_session_set_pitch", "pitch", [&](const char* who, OutSettings& o) { return out_set_pitch(who, o, cents); });
}
extern "C" q3_status q3_session_set_level(q3_session* s, int b, int gain_mB, int ceiling_mB) {
    return session_set_rows(s, b, "q3_session_set_level", "level", [&](const char* who, OutSettings& o) { return out_set_level(who, o, gain_mB, ceiling_mB); });
}
extern "C" q3_status q3_session_set_loudness(q3_session* s, int b, int mode, int target_mB, int prior_mB) {
    return session_set_rows(s, b, "q3_session_set_loudness", "loudness step",
                            [&](const char* who, OutSettings& o) { return out_set_loudness(who, o, mode, target_mB, prior_mB); });
}
extern "C" q3_status q3_session_loudness(q3_session* s, int b, float* mean_square, float* gain, int* blocks, int* gated) {
    if (!s) return set_err(Q3_INVALID_ARG, "q3_session_loudness: null session");
    if (b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "q3_session_loudness: row %d out of range (%d rows)", b, s->B);
    if (s->out[(size_t)b].loud == Q3_LOUD_OFF)
        return set_err(Q3_INVALID_ARG, "q3_session_loudness: row %d has no loudness step (q3_session_set_loudness)", b);
    if (!s->ostage) { out_loudness_at_rest(s->out[(size_t)b], mean_square, gain, blocks, gated); return Q3_OK; }      // nothing streamed yet
    return q3_pcm_stage_loudness(s->ostage, b, mean_square, gain, blocks, gated);
}
extern "C" q3_status q3_session_set_silence(q3_session* s, int b, int threshold_mB, int edge_ms, int pause_ms) {
    return session_set_rows(s, b, "q3_session_set_silence", "silence step",
                            [&](const char* who, OutSettings& o) { return out_set_silence(who, o, threshold_mB, edge_ms, pause_ms); });
}
extern "C" q3_status q3_session_set_mark(q3_session* s, int b, uint64_t key, int strength_mB) {
    return session_set_rows(s, b, "q3_session_set_mark", "mark", [&](const char* who, OutSettings& o) { return out_set_mark(who, o, key, strength_mB); });
}
extern "C" q3_status q3_session_silence(q3_session* s, int b, int64_t* n_in, int64_t* n_out, int64_t* lead_cut, int64_t* pause_cut, int64_t* trail_cut) {
    if (!s) return set_err(Q3_INVALID_ARG, "q3_session_silence: null session");
    if (b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "q3_session_silence: row %d out of range (%d rows)", b, s->B);
    if (s->out[(size_t)b].sil_mB == 0)
        return set_err(Q3_INVALID_ARG, "q3_session_silence: row %d has no silence step (q3_session_set_silence)", b);
    if (!s->ostage) { out_silence_at_rest(n_in, n_out, lead_cut, pause_cut, trail_cut); return Q3_OK; }      // nothing streamed yet
    return q3_pcm_stage_silence(s->ostage, b, n_in, n_out, lead_cut, pause_cut, trail_cut);
}
extern "C" q3_status q3_session_next_chunks_out(q3_session* s, void* const* out_host, const size_t* cap_samples, size_t* n_samples, int* done) {
    if (!s) return set_err(Q3_INVALID_ARG, "q3_session_next_chunks_out: null session");
    if (!n_samples || !done || !out_host || !cap_samples) return set_err(Q3_INVALID_ARG, "q3_session_next_chunks_out: null argument");
    if (s->m->device < 0) return set_err(Q3_INVALID_ARG, "q3_session_next_chunks_out: the model has no device");
    if (!s->ostage) {
        Q3C(q3_pcm_stage_create(s->m->device, s->B, (size_t)chunk_frames_of(s) * samples_per_frame(s->m->cfg), &s->ostage));
        for (int b = 0; b < s->B; ++b) Q3C(pcm_stage_apply(s->ostage, b, "q3_session_next_chunks_out", s->out[(size_t)b]));
    }
    s->out_started = true;
    return next_chunks(s, nullptr, cap_samples, n_samples, done, true, out_host);
}
static q3_status next_chunks(q3_session* s, float* const* pcm_host, const size_t* cap, size_t* n_samples, int* done, bool out, void* const* out_host) {
    HIPC(hipSetDevice(s->m->device));
    if (!s->prefilled) Q3C(q3_session_prefill(s));
    Q3C(refresh_codes(s));
    const int spf = samples_per_frame(s->m->cfg);
    for (int b = 0; b < s->B; ++b) Q3C(chunk_fill(s, b));
    // what every row gets; refused as a whole before any row moves
    std::vector<ChunkCut> cuts;
    for (int b = 0; b < s->B; ++b) {
        const ChunkCut c = chunk_cut(s, b);
        cuts.push_back(c);
        if (out) {
            const size_t cnt = pcm_stage_count(s->ostage, b, (size_t)c.avail * spf, c.ends);
            if (cnt > 0 && (!out_host[b] || cap[b] < cnt))
                return set_err(Q3_INVALID_ARG, "q3_session_next_chunks_out: output buffer of row %d too small (%zu samples needed)", b, cnt);
        } else if (c.avail > 0 && pcm_host && pcm_host[b] && (!cap || cap[b] < (size_t)c.avail * spf))
            return set_err(Q3_INVALID_ARG, "q3_session_next_chunks: pcm buffer of row %d too small", b);
    }
    std::vector<CsPush> pushes;
    std::vector<float> tmp;
    for (int b = 0; b < s->B; ++b) {
        const SeqInfo& q = s->seq[b];
        const int a = cuts[(size_t)b].avail, last = cuts[(size_t)b].ends ? 1 : 0;
        n_samples[b] = out ? 0 : (size_t)a * spf;
        if (a <= 0 && !(out && last)) continue;          // (out: a == 0 but last flushes the stage row)
        if (s->stream_mode == 1 && !q.icl) {
            if (!s->cstream) Q3C(codec_stream_create(s->m, s->B, s->max_frames, s->stream, &s->cstream));
            int sp = 0;
            CsPush p{b, 0, 0, nullptr, nullptr, nullptr};
            if (a > 0) {
                // the row's state follows the row: behind it (q3_session_next_chunk[_row] moved the row on) the push catches up,
                // ahead of it (another utterance's) it starts over
                if (codec_stream_pos(s->cstream, b) > q.stream_pos) codec_stream_reset(s->cstream, b);
                sp = codec_stream_pos(s->cstream, b);
                p.n = q.stream_pos + a - sp; p.skip = q.stream_pos - sp;
            }
            p.dev = s->codes + ((size_t)b * s->max_frames + sp) * 16;
            if (out) { p.ps = s->ostage; p.ps_row = b; p.last = last; p.out_host = out_host[b]; p.n_out = &n_samples[b]; }
            else p.pcm_host = pcm_host ? pcm_host[b] : nullptr;
            pushes.push_back(p);
        } else if (out) {
            // ICL rows and stream mode 0 keep the per-row context-free decode; its samples take the stage's host entry
            tmp.resize((size_t)a * spf);
            if (a > 0) Q3C(chunk_decode_row(s, b, a, tmp.data(), tmp.size(), nullptr));
            const float* in = tmp.data(); const size_t n_in = tmp.size();
            Q3C(q3_pcm_stage_push(s->ostage, 1, &b, &in, &n_in, &last, &out_host[b], &cap[b], &n_samples[b]));
        } else {
            Q3C(chunk_decode_row(s, b, a, pcm_host ? pcm_host[b] : nullptr, cap ? cap[b] : 0, nullptr));
        }
    }
    if (!pushes.empty()) Q3C(codec_stream_push(s->cstream, pushes));
    for (int b = 0; b < s->B; ++b) {
        s->seq[(size_t)b].stream_pos += cuts[(size_t)b].avail;
        done[b] = cuts[(size_t)b].ends ? 1 : 0;
    }
    return Q3_OK;
}

extern "C" q3_status q3_session_frames(q3_session* s, int b, int* n_frames, int* done) {
    if (!s || b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "bad sequence index");
    HIPC(hipSetDevice(s->m->device));
    Q3C(refresh_codes(s));
    if (n_frames) *n_frames = s->seq[b].n_frames;
    if (done) *done = s->seq[b].done ? 1 : 0;
    return Q3_OK;
}

extern "C" q3_status q3_session_codes(q3_session* s, int b, uint32_t* codes_host, int cap_frames, int* n_frames) {
    if (!s || b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "bad sequence index");
    HIPC(hipSetDevice(s->m->device));
    Q3C(refresh_codes(s));
    const int n = s->seq[b].n_frames;
    if (n_frames) *n_frames = n;
    if (codes_host) {
        if (cap_frames < n) return set_err(Q3_INVALID_ARG, "codes buffer too small (%d < %d frames)", cap_frames, n);
        memcpy(codes_host, &s->codes_host[(size_t)b * s->max_frames * 16], (size_t)n * 16 * 4);
    }
    return Q3_OK;
}

extern "C" q3_status q3_session_decode(q3_session* s, int b, int f0, int f1, float* pcm_host, size_t cap, size_t* n_samples) {
    if (!s || b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "bad sequence index");
    HIPC(hipSetDevice(s->m->device));
    Q3C(refresh_codes(s));
    if (f0 < 0 || f1 < f0 || f1 > s->seq[b].n_frames) return set_err(Q3_INVALID_ARG, "bad frame range [%d,%d) of %d", f0, f1, s->seq[b].n_frames);
    if (n_samples) *n_samples = 0;
    if (f1 == f0) return Q3_OK;
    // a part of a row: context-free, an utterance of its own; the whole row: behind its reference frames where it is an ICL row
    VocodePcm pcm;
    Q3C(vocode_enqueue(s->m, s->cws, s->stream, row_src(s, b, f0, f0 == 0 && f1 == s->seq[b].n_frames), 0, f1 - f0, 0, 0, &pcm));
    HIPC(sync_frames(s));
    return vocode_copy_out(pcm, pcm_host, cap, n_samples, nullptr);
}

// ---- q3_session_run: the knobs, the lanes, the serial and the overlapped vocoder phase ----
using run_clk = std::chrono::steady_clock;
static double run_ms(run_clk::time_point a, run_clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
// The environment knobs of q3_session_run (A/B aids), clamped. overlap, resident, seg, tail and log are read on every call
// (tests set them per test); pairs and cus once per process.
struct RunKnobs {
    int overlap;       // Q3_DECODE_OVERLAP: 0 the serial path, 1 overlap on, -1 (unset) DECODE_OVERLAP_DEFAULT below
    int resident;      // Q3_DECODE_RESIDENT = 0|1|2 (1): the residency cap of the segments decoded beside the frames (0 = none: the unsplit overlap of round 6)
    int seg, tail;     // Q3_DECODE_SEG (256) / Q3_DECODE_TAIL (32), 16 at least: the segment schedule (run_overlapped)
    int pairs;         // Q3_DECODE_PAIRS = 1..8 (2): utterances vocoded at a time (run_serial)
    int cus;           // Q3_DECODE_CUS (0 = off; 8..248 in eighths): the chip split while both run (run_overlapped)
    bool log;          // Q3_DECODE_LOG: one line per overlapped run on stderr
};
static int env_int(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
static RunKnobs read_run_knobs() {
    static const int pairs = std::min(std::max(env_int("Q3_DECODE_PAIRS", 2), 1), 8);
    static const int cus = [] { const int v = env_int("Q3_DECODE_CUS", 0); return v <= 0 ? 0 : (v < 8 ? 8 : (v > 248 ? 248 : v & ~7)); }();
    const char* overlap = getenv("Q3_DECODE_OVERLAP");
    return {overlap ? (atoi(overlap) != 0 ? 1 : 0) : -1, std::min(std::max(env_int("Q3_DECODE_RESIDENT", 1), 0), 2),
            std::max(env_int("Q3_DECODE_SEG", 256), 16), std::max(env_int("Q3_DECODE_TAIL", 32), 16), pairs, cus, getenv("Q3_DECODE_LOG") != nullptr};
}
// Utterances vocoded side by side, each on its own workspace and stream: lane 0 is the session's own pair, decode_lanes makes
// the n - 1 others once (they live as long as the session)
struct Lane { CodecWS& ws; hipStream_t st; };
static q3_status decode_lanes(q3_session* s, int n) {
    while ((int)s->par_ws.size() < n - 1) {
        hipStream_t st = nullptr;
        HIPC(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        s->par_ws.emplace_back(); s->par_streams.push_back(st);
    }
    return Q3_OK;
}
static Lane lane(q3_session* s, int k) { return k == 0 ? Lane{s->cws, s->stream} : Lane{s->par_ws[(size_t)k - 1], s->par_streams[(size_t)k - 1]}; }

// The serial path: every frame, then every row's vocoder. frames_done: when the frames were.
static q3_status run_serial(q3_session* s, int use_graph, const RunKnobs& kn, float** pcm_host, const size_t* cap, run_clk::time_point* frames_done) {
    Q3C(q3_session_generate(s, s->max_frames, use_graph));
    Q3C(refresh_codes(s));
    *frames_done = run_clk::now();
    const int spf = samples_per_frame(s->m->cfg), conc = kn.pairs;
    bool any_icl = false;
    for (auto& q : s->seq) any_icl = any_icl || !q.ref_codes.empty();
    if (conc == 1 || s->B == 1 || any_icl) {                 // one lane: row after row, as q3_session_decode gives them
        for (int b = 0; b < s->B; ++b) Q3C(q3_session_decode(s, b, 0, s->seq[b].n_frames, pcm_host ? pcm_host[b] : nullptr, cap ? cap[b] : 0, nullptr));
        return Q3_OK;
    }
    // Two utterances are vocoded at a time, each on its own stream and workspace: most of a decode saturates the
    // chip, but its front (the pre-transformer's ~90 launches on 10-160 workgroups) is latency-bound and fills in beside
    // the other utterance's convolutions. Q3_DECODE_PAIRS=n: n at a time (1 = serial; A/B aid). Re-measured in round 6
    // (profiles/r6_decode_knobs_ab.txt): 8 x 640 frames 155.3 / 157.7 / 162.1 ms at 2 / 4 / 8 at a time, 64 x 640 frames
    // 1261 / 1274 ms at 2 / 4 — four was the round-1 optimum, when the front was 4 of 28 ms; it is 2 of 19.8 now.
    Q3C(decode_lanes(s, conc));
    if (pcm_host)                                            // refused as a whole before any row's samples move
        for (int b = 0; b < s->B; ++b)
            if (pcm_host[b] && s->seq[b].n_frames && (!cap || cap[b] < (size_t)s->seq[b].n_frames * spf)) return set_err(Q3_INVALID_ARG, "pcm buffer too small");
    for (int b0 = 0; b0 < s->B; b0 += conc) {
        const int nb = (s->B - b0) < conc ? (s->B - b0) : conc;
        for (int k = 0; k < nb; ++k) {
            const int b = b0 + k, T = s->seq[b].n_frames;
            if (T == 0) continue;
            const Lane ln = lane(s, k);
            VocodePcm pcm;
            Q3C(vocode_enqueue(s->m, ln.ws, ln.st, row_src(s, b), 0, T, 0, 0, &pcm));
            // the samples leave for the host on the utterance's own stream, beside the other utterances' decodes
            // (synthesize returns host samples, lib.rs:718-784); pinned caller buffers make this a true async copy
            Q3C(vocode_copy_out(pcm, pcm_host ? pcm_host[b] : nullptr, cap ? cap[b] : 0, nullptr, ln.st));
        }
        for (int k = 0; k < nb; ++k) HIPC(hipStreamSynchronize(lane(s, k).st));
    }
    return Q3_OK;
}

// synthesize_with_timing for the whole batch. In the overlapped path (Q3_DECODE_OVERLAP=1, or unset: DECODE_OVERLAP_DEFAULT
// below; never with an ICL sequence) the vocoder does not
// wait for the last frame: every Q3_DECODE_SEG (default 256) generated frames a helper thread enqueues the segment's
// decode (exact: CODEC_CTX_FRAMES of left context re-run, see codec_decode_dev) on a second stream beside the frame
// loop, the samples going straight to the caller's buffers; the last Q3_DECODE_TAIL (32) frames of a row are the only
// segment nothing overlaps.
// Why the UNSPLIT overlap lost in round 6 (1.7B, 8 x 640 frames: frame loop 1636 -> 1767 ms, decode tail 155 -> 54 ms,
// 2843 -> 2797 frames/s): registers. The conv kernels run three workgroups per CU at 150-168 VGPRs per lane, 3 x 160 = 480 of a
// SIMD's 512. A frame kernel's workgroup is 8 waves, two per SIMD, at 88-168 VGPRs (k_gemv_mfma 101, k_gemv_sk2 118, k_gemv_gu24
// 152, k_attn_fused 92, k_gemv_lds 166): it needs HALF a CU's registers, 2 x 104..168 per SIMD. A retiring conv workgroup frees
// 160 per SIMD: only the next conv workgroup of the same launch fits that hole, so the frame node waits until the conv launch
// drains — for each of 549 dependent nodes. Splitting the chip (Q3_DECODE_CUS below) costs the frames more than the vocoder takes.
// Hence the residency cap (Q3_DECODE_RESIDENT, default 1; ConvArgs::resident): the segments decoded beside the frames hold one
// conv workgroup per CU, 160 + 2 x 168 = 496 <= 512 registers per SIMD, so a frame workgroup always finds room on every CU; the
// tail after the loop runs uncapped on the whole chip. Measured (profiles/decode_resident_overlap_ab.txt): with 128-frame segments
// the cap turns the loss into a tie (no cap / 1 / 2 per CU: 2789 / 2836 / 2777 frames/s against 2835 serial); each segment re-runs
// the front over [0, e) and 12 context frames, and with 256-frame segments the capped overlap wins: 2898-2899 against 2836-2847
// (frame loop +101 ms, exposed decode 160 -> 21 ms). The enqueue thread never holds up the frame loop (Q3_DECODE_LOG: < 0.02 ms).
// DECODE_OVERLAP_DEFAULT: what Q3_DECODE_OVERLAP unset means for sessions of 2 to 16 rows (16 rows: 3983-4051 -> 4139-4141 frames/s).
// A single row has 21 ms of vocoder to hide and ends in a tie (413.8-415.3 serial, 414.0-414.6 overlapped): serial. Wider sessions run
// the k_wide* frame kernels with other register counts and lose 6.5-12.8 % with every overlap variant: serial. DESIGN 4.3 / 7a / 8.3.
static constexpr bool DECODE_OVERLAP_DEFAULT = true;
struct SegJob { int b, a, e; };
// one segment: codes -> workspace, vocoder over [a - context, e), the samples of [a, e) straight to the caller's buffer
// (resident: the residency cap of this decode's launches — the knob beside the frames, 0 for the tail on the whole chip)
static q3_status seg_enqueue(q3_session* s, const SegJob& j, CodecWS& ws, hipStream_t st, int resident, float** pcm_host, const size_t* cap) {
    const size_t at = (size_t)j.a * samples_per_frame(s->m->cfg);
    float* host = pcm_host ? pcm_host[j.b] : nullptr;
    VocodePcm pcm;
    Q3C(vocode_enqueue(s->m, ws, st, row_src(s, j.b), j.a, j.e, vocode_ctx_start(j.a), resident, &pcm));
    return vocode_copy_out(pcm, host ? host + at : nullptr, cap && cap[j.b] > at ? cap[j.b] - at : 0, nullptr, st);
}
// the segments that are ready behind dec_pos (final_pass: whatever is left), at most seg new frames each: every call stays within the workspace
static std::vector<SegJob> seg_collect(const q3_session* s, std::vector<int>& dec_pos, int seg, bool final_pass) {
    std::vector<SegJob> jobs;
    for (int b = 0; b < s->B; ++b) {
        const SeqInfo& q = s->seq[b];
        const int e = (q.done || final_pass) ? q.n_frames : (q.n_frames < s->frames_run ? q.n_frames : s->frames_run);
        if (e > dec_pos[(size_t)b] && (final_pass || q.done || e - dec_pos[(size_t)b] >= 16)) {
            for (int a = dec_pos[(size_t)b]; a < e; a += seg) jobs.push_back({b, a, a + seg < e ? a + seg : e});
            dec_pos[(size_t)b] = e;
        }
    }
    return jobs;
}
struct OverlapMarks { run_clk::time_point frames_done; int n_dispatch = 0; double join_wait_ms = 0.0; };      // join_wait_ms: what the frame loop's thread spent waiting for the enqueue thread (Q3_DECODE_LOG)
static q3_status run_overlapped(q3_session* s, int use_graph, const RunKnobs& kn, float** pcm_host, const size_t* cap, OverlapMarks* marks) {
    HIPC(hipSetDevice(s->m->device));
    // Q3_DECODE_CUS=n (measurement aid, default 0 = off) SPLITS the chip while both run: the frames keep the first 256 - n bits of the CU
    // mask on their own queue, the decode stream gets the last n (n / 8 CUs of every XCD, see aql_restrict_cus), so a frame kernel's
    // workgroups are never dealt onto a CU the vocoder holds. Measured in round 6 (profiles/r6_split_chip_overlap_ab.txt): the vocoder
    // beside the frames then costs them only 3 %, but the frames ALONE on 224 / 192 / 128 CUs are 16 / 15 / 23 % slower — their grids are
    // one workgroup per CU of the whole chip, and the slowest workgroup of every one of 549 dependent launches sets the pace.
    if (!s->dec_stream) {
        if (kn.cus) {
            uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = 256 - kn.cus; i < 256; ++i) mask[i >> 5] |= 1u << (i & 31);
            HIPC(hipExtStreamCreateWithCUMask(&s->dec_stream, 8, mask));
        } else {
            int least = 0, greatest = 0;
            HIPC(hipDeviceGetStreamPriorityRange(&least, &greatest));
            HIPC(hipStreamCreateWithPriority(&s->dec_stream, hipStreamNonBlocking, least));
        }
    }
    Q3C(codec_reserve(s->m, s->seg_ws, kn.seg + CODEC_CTX_FRAMES, s->max_frames));
    struct Split {                                         // the whole chip goes back to the frames' queue on every way out
        q3::AqlProgram* p = nullptr;
        void release() { if (p) { std::string why; q3::aql_restrict_cus(p, 0, &why); p = nullptr; } }
        ~Split() { release(); }
    } split;
    if (kn.cus && s->aql && !s->aql_failed) { std::string why; if (q3::aql_restrict_cus(s->aql, 256 - kn.cus, &why)) split.p = s->aql; }
    std::vector<int> dec_pos((size_t)s->B, 0);
    std::thread worker; q3_status wst = Q3_OK; std::string werr;
    auto join = [&]() -> q3_status {
        if (worker.joinable()) worker.join();
        if (wst != Q3_OK) return set_err(wst, "%s", werr.c_str());
        return Q3_OK;
    };
    auto dispatch = [&]() -> q3_status {
        std::vector<SegJob> jobs = seg_collect(s, dec_pos, kn.seg, false);
        if (jobs.empty()) return Q3_OK;
        {   // the previous segment's enqueue must be over: normally long since (its thread only enqueues; a segment of frames is ~0.3 s)
            const auto j0 = run_clk::now();
            Q3C(join());
            marks->join_wait_ms += run_ms(j0, run_clk::now()); ++marks->n_dispatch;
        }
        worker = std::thread([s, jobs, resident = kn.resident, pcm_host, cap, &wst, &werr]() {
            if (hipSetDevice(s->m->device) != hipSuccess) { wst = Q3_HIP_ERROR; werr = "hipSetDevice failed in the decode thread"; return; }
            for (const SegJob& j : jobs) {
                const q3_status st = seg_enqueue(s, j, s->seg_ws, s->dec_stream, resident, pcm_host, cap);
                if (st != Q3_OK) { wst = st; werr = q3_last_error(); return; }
            }
        });
        return Q3_OK;
    };
    // the last segment of a row is the only one nothing overlaps: it is kept short (Q3_DECODE_TAIL frames, default 32)
    q3_status st = Q3_OK;
    while (st == Q3_OK && session_remaining(s) > 0 && !all_done(s)) {
        int n = kn.seg;
        const int left = session_remaining(s);
        if (left > kn.tail && left - n < kn.tail) n = left - kn.tail;        // ... so the step before it stops kn.tail frames short of the end
        st = q3_session_generate(s, n, use_graph);
        if (st == Q3_OK) st = refresh_codes(s);
        if (st == Q3_OK && session_remaining(s) > 0 && !all_done(s)) st = dispatch();
    }
    marks->frames_done = run_clk::now();
    split.release();
    { const q3_status js = join(); if (st == Q3_OK) st = js; }
    if (st != Q3_OK) { hipStreamSynchronize(s->dec_stream); return st; }
    // what is left runs on the whole chip beside the confined stream's backlog: utterances side by side as in the plain path.
    // Whatever happens, nothing returns while a stream may still be copying samples into the caller's buffers.
    const int conc = 2;
    auto tail = [&]() -> q3_status {
        std::vector<SegJob> jobs = seg_collect(s, dec_pos, kn.seg, true);
        Q3C(decode_lanes(s, conc));
        for (int k = 0; k < conc; ++k) Q3C(codec_reserve(s->m, lane(s, k).ws, kn.seg + CODEC_CTX_FRAMES, s->max_frames));
        for (size_t i = 0; i < jobs.size(); ++i) { const Lane ln = lane(s, (int)(i % conc)); Q3C(seg_enqueue(s, jobs[i], ln.ws, ln.st, 0, pcm_host, cap)); }
        return Q3_OK;
    };
    st = tail();
    hipError_t he = hipStreamSynchronize(s->dec_stream);
    for (int k = 0; k < conc && k <= (int)s->par_streams.size(); ++k) { const hipError_t e2 = hipStreamSynchronize(lane(s, k).st); if (he == hipSuccess) he = e2; }
    if (st != Q3_OK) return st;
    HIPC(he);
    return Q3_OK;
}

// Open-text check, prefill, knobs, one of the two paths above, the counts and the timing
extern "C" q3_status q3_session_run(q3_session* s, int use_graph, float** pcm_host, const size_t* cap, size_t* n_samples, q3_timing* timing) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (any_open_text(s)) return set_err(Q3_UNSUPPORTED, "q3_session_run: a row's text is still open (q3_session_append_text with last != 0 closes it; or drive the session with q3_session_generate)");
    const auto t0 = run_clk::now();
    s->precapture = use_graph != 0;
    Q3C(q3_session_prefill(s));
    const auto t1 = run_clk::now();
    const RunKnobs kn = read_run_knobs();
    const bool overlap_wanted = kn.overlap >= 0 ? kn.overlap != 0 : (DECODE_OVERLAP_DEFAULT && s->B >= 2 && s->B <= 16);
    bool overlap = overlap_wanted && !s->debug && !s->profile && s->max_frames > kn.seg;
    for (auto& q : s->seq) if (!q.ref_codes.empty()) overlap = false;
    OverlapMarks marks;
    Q3C(overlap ? run_overlapped(s, use_graph, kn, pcm_host, cap, &marks) : run_serial(s, use_graph, kn, pcm_host, cap, &marks.frames_done));
    // (an ICL row's count too: its reference frames' samples are cut whole)
    int total = 0;
    for (int b = 0; b < s->B; ++b) {
        if (n_samples) n_samples[b] = (size_t)s->seq[b].n_frames * samples_per_frame(s->m->cfg);
        total += s->seq[b].n_frames;
    }
    const auto t2 = marks.frames_done, t3 = run_clk::now();
    if (timing) { timing->prefill_ms = run_ms(t0, t1); timing->generation_ms = run_ms(t1, t2); timing->decode_ms = run_ms(t2, t3); timing->generation_frames = total; }
    // Q3_DECODE_LOG=1 (A/B aid): one line per run on stderr — did the enqueue thread ever hold up the frame loop, how long was the exposed tail
    if (overlap && kn.log)
        fprintf(stderr, "q3_session_run overlap: resident %d seg %d tail %d, %d dispatches, frame loop waited %.3f ms for the enqueue thread, frames %.1f ms, exposed decode %.1f ms\n",
                kn.resident, kn.seg, kn.tail, marks.n_dispatch, marks.join_wait_ms, run_ms(t1, t2), run_ms(t2, t3));
    return Q3_OK;
}

extern "C" q3_status q3_session_set_stream_mode(q3_session* s, int mode) {
    if (!s || (mode != 0 && mode != 1)) return set_err(Q3_INVALID_ARG, "q3_session_set_stream_mode: mode must be 0 (context-free) or 1 (continuous)");
    s->stream_mode = mode;
    return Q3_OK;
}

extern "C" q3_status q3_session_next_chunk(q3_session* s, float* pcm_host, size_t cap, size_t* n_samples, int* done) {
    if (!s) return set_err(Q3_INVALID_ARG, "null session");
    if (s->B != 1) return set_err(Q3_UNSUPPORTED, "streaming sessions are batch 1 (StreamingSession, lib.rs:1484)");
    if (!s->prefilled) { s->precapture = true; Q3C(q3_session_prefill(s)); }
    Q3C(refresh_codes(s));
    Q3C(chunk_fill(s, 0));
    // (open text: the fill stopped at the held frame, and the read-ahead below never goes past what the text allows: session_remaining)
    const ChunkCut cut = chunk_cut(s, 0);
    if (cut.avail <= 0) { if (n_samples) *n_samples = 0; if (done) *done = cut.ends ? 1 : 0; return Q3_OK; }
    SeqInfo& q = s->seq[0];
    const int chunk = chunk_frames_of(s), avail = cut.avail;
    // Read-ahead: the frames of the NEXT chunk are enqueued (no host wait for them) while this chunk is vocoded and handed
    // over, so the frame loop keeps going while the host copies out, returns and plays the chunk.
    // First chunk: its vocoder is enqueued first, on the session's stream, then the replays. As graph launches they queue behind
    // it on the same stream and the host waits on an event, not on the stream. On the own (AQL) queue, which is not ordered
    // with the stream, launch_ahead synchronises the stream before it submits: the first chunk is then serial — vocoder,
    // wait, replays handed over, return — and time-to-first-audio is what it is without read-ahead.
    // Later chunks: the replays go first and the chunk's vocoder runs beside them on its own stream — a chunk then costs
    // max(generation, decode) instead of their sum (streaming RTF 0.046 -> 0.042 on the 1.7B model); on the AQL path the
    // stream that launch_ahead synchronises holds only the K/V table updates then. After EOS the device-side done flag turns
    // extra replays into no-ops. Q3_STREAM_NO_AHEAD=1 restores the serial schedule (A/B aid).
    static const bool no_ahead = getenv("Q3_STREAM_NO_AHEAD") != nullptr;
    int ahead = 0;
    if (!no_ahead && !q.done && (s->aql || s->graph_exec) && !s->aql_failed && !s->debug && !s->profile) {
        ahead = chunk - (q.n_frames - (q.stream_pos + avail));
        if (ahead > session_remaining(s)) ahead = session_remaining(s);
        if (ahead < 0) ahead = 0;
    }
    const bool first = q.stream_pos == 0;
    auto launch_ahead = [&]() -> q3_status {
        Q3C(kv_reserve_frames(s, ahead));                        // (its table updates ride s->stream)
        if (s->aql) HIPC(hipStreamSynchronize(s->stream));       // the own queue is not ordered with the stream
        return frames_enqueue(s, ahead);                         // the next call re-reads codes / EOS state after sync_frames
    };
    hipStream_t dst = s->stream;
    if (ahead > 0 && !first) {
        if (!s->dec_stream) HIPC(hipStreamCreateWithFlags(&s->dec_stream, hipStreamNonBlocking));
        Q3C(launch_ahead());
        dst = s->dec_stream;
    }
    VocodePcm pcm;
    Q3C(chunk_vocode_enqueue(s, 0, avail, dst, &pcm));
    if (ahead > 0 && first) {
        if (!s->dec_ev) HIPC(hipEventCreateWithFlags(&s->dec_ev, hipEventDisableTiming));
        HIPC(hipEventRecord(s->dec_ev, s->stream));
        Q3C(launch_ahead());
        HIPC(hipEventSynchronize(s->dec_ev));
    } else {
        HIPC(hipStreamSynchronize(dst));
    }
    Q3C(vocode_copy_out(pcm, pcm_host, cap, n_samples, nullptr));
    q.stream_pos += avail;
    if (done) *done = cut.ends ? 1 : 0;
    return Q3_OK;
}

extern "C" q3_status q3_session_get(q3_session* s, int what, int b, void* out, size_t bytes) {
    if (!s || !out || b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "bad argument");
    const q3_config& c = s->m->cfg;
    HIPC(hipSetDevice(s->m->device));
    HIPC(sync_frames(s));
    const void* src = nullptr; size_t need = 0;
    switch (what) {
        case Q3_GET_PREFILL_EMBEDS: src = s->embeds + (size_t)b * s->prefill_len * c.hidden; need = (size_t)s->prefill_len * c.hidden * 4; break;
        case Q3_GET_LAST_HIDDEN: src = s->LASTH + (size_t)b * c.hidden; need = (size_t)c.hidden * 4; break;
        case Q3_GET_LOGITS: src = s->LOGITS + (size_t)b * c.codec_vocab; need = (size_t)c.codec_vocab * 4; break;
        case Q3_GET_TRAILING: src = s->rows + (size_t)s->seq[b].trail_base * c.hidden; need = (size_t)s->seq[b].trailing_len * c.hidden * 4; break;
        case Q3_GET_PAD_EMBED: src = s->rows + (size_t)s->seq[b].pad_row * c.hidden; need = (size_t)c.hidden * 4; break;
        case Q3_GET_LOGITS_HIST:
            if (!s->logits_hist) return set_err(Q3_INVALID_ARG, "session has no debug capture");
            src = s->logits_hist + (size_t)b * (s->max_frames + 1) * c.codec_vocab; need = (size_t)(s->frames_run + 1) * c.codec_vocab * 4; break;
        case Q3_GET_TOKEN: src = s->tok + b; need = 4; break;
        case Q3_GET_CP_LOGITS: {
            // [15][B][V] on device → [15][V] for sequence b
            need = (size_t)15 * c.cp_vocab * 4;
            if (bytes < need) return set_err(Q3_INVALID_ARG, "buffer too small");
            for (int g = 0; g < 15; ++g)
                HIPC(q3_hipMemcpy((char*)out + (size_t)g * c.cp_vocab * 4, s->CP_LOGITS + ((size_t)g * s->B + b) * c.cp_vocab, (size_t)c.cp_vocab * 4, hipMemcpyDeviceToHost));
            return Q3_OK;
        }
        case Q3_GET_CP_LOGITS_HIST: {
            if (!s->cp_logits_hist) return set_err(Q3_INVALID_ARG, "session has no debug capture");
            need = (size_t)s->frames_run * 15 * c.cp_vocab * 4;
            if (bytes < need) return set_err(Q3_INVALID_ARG, "buffer too small");
            for (int f = 0; f < s->frames_run; ++f)
                for (int g = 0; g < 15; ++g)
                    HIPC(q3_hipMemcpy((char*)out + ((size_t)f * 15 + g) * c.cp_vocab * 4,
                                   s->cp_logits_hist + (((size_t)f * 15 + g) * s->B + b) * c.cp_vocab, (size_t)c.cp_vocab * 4, hipMemcpyDeviceToHost));
            return Q3_OK;
        }
        default: return set_err(Q3_INVALID_ARG, "unknown item %d", what);
    }
    if (bytes < need) return set_err(Q3_INVALID_ARG, "buffer too small (%zu < %zu)", bytes, need);
    HIPC(q3_hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
    return Q3_OK;
}

