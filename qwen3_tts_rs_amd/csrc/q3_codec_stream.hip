// q3_codec_stream.hip — the codec stream: the vocoder with per-row decode state, many rows per pass
// (a unit of the engine: q3_engine.h says which holds what)
//
// State of a row, for its frames [0, pos): K (after RoPE) and V of every pre-transformer layer as [layer][K | V][QD][cap], the
// front's output latent [LAT][cap], and the last two quantiser output columns [Q][2] (what the k = 3 pre_conv reads to the left
// of the next frame). A push runs the front over the NEW columns of all pushed rows, concatenated along L (codec_run's own
// stages: every launch of theirs is per-column work), and the convolutional stack over each row's [a0 - CODEC_CTX_FRAMES, e),
// again concatenated: every layer of the stack is causal and sums an output in a position-independent order, so the samples of
// a row's frames >= a0 depend on its own CODEC_CTX_FRAMES context columns only — what sits to the left of those (the previous
// row's tail) reaches the context columns' outputs alone, which are dropped. That is the argument codec_decode_dev(..., c0)
// rests on, for several rows. A row still inside its first CODEC_CTX_FRAMES frames needs the zero padding of every inner layer,
// which no neighbour can stand in for: it runs the stack on its own [0, e).
//
// A BLOCKED stream (q3_codec_stream_create_blocked) keeps K | V and the latent of a row in blocks of bf frames (bf % 32 == 0), one
// block = [layer][K | V][QD][bf] followed by [LAT][bf], taken from the stream's free list when a push reaches them and given back
// at reset: a row holds what its frames need, not max_frames. Frame f of a row is column f % bf of its block f / bf. Blocks are
// never cleared: every kernel reads a frame only below the row's position. The launches are the same ones with block-aware
// descriptors, and the attention is the third instance of attn_c_tile (k_attn_cb), which differs in addressing only.
#include "q3_engine.h"

struct CsRow { int pos = 0; float* kv = nullptr; float* lat = nullptr; float* hist = nullptr; std::vector<float*> blocks; };
struct q3_codec_stream {
    q3_model* m = nullptr; int R = 0, cap = 0;
    int bf = 0, max_blocks = 0;                              // blocked stream: frames per block (0 = whole-row state), block limit (0 = none)
    std::vector<float*> free_blocks; int blocks_total = 0, blocks_in_use = 0, blocks_peak = 0;
    hipStream_t st = nullptr; bool owns_stream = false;
    std::vector<CsRow> rows;
    CodecWS ws;
    float *cs = nullptr, *sn = nullptr;                      // RoPE table [cap][32]
    char* desc = nullptr; size_t desc_cap = 0;               // the descriptor block of one push (one upload)
    float* stage = nullptr; float* stage_host = nullptr; size_t stage_cap = 0;      // the wanted samples of all rows: device, pinned host
};

static size_t kv_floats(const q3_codec_stream* cs) {
    const q3_config& c = cs->m->cfg;
    return (size_t)c.dec_layers * 2 * c.dec_heads * c.dec_head_dim * cs->cap;
}

static size_t block_floats(const q3_codec_stream* cs) {
    const q3_config& c = cs->m->cfg;
    return ((size_t)c.dec_layers * 2 * c.dec_heads * c.dec_head_dim + c.dec_latent) * cs->bf;
}

q3_status codec_stream_create(q3_model* m, int rows, int max_frames, hipStream_t st, q3_codec_stream** out, int block_frames, int max_blocks) {
    if (!m || !m->finalized) return set_err(Q3_INVALID_ARG, "model not finalized");
    if (!out || rows < 1 || max_frames < 1) return set_err(Q3_INVALID_ARG, "q3_codec_stream_create: rows and max_frames must be positive");
    if (m->device < 0) return set_err(Q3_INVALID_ARG, "q3_codec_stream_create: the model has no device (manifest-only): the vocoder runs on the GPU");
    if (m->cfg.dec_head_dim != 64) return set_err(Q3_INVALID_ARG, "q3_codec_stream_create: decoder head dim must be 64");
    HIPC(hipSetDevice(m->device));
    std::unique_ptr<q3_codec_stream> cs(new q3_codec_stream());
    cs->m = m; cs->R = rows; cs->cap = max_frames; cs->rows.resize(rows);
    cs->bf = block_frames; cs->max_blocks = max_blocks;
    m->refs.fetch_add(1);
    auto fail = [&](q3_status s) { q3_codec_stream_free(cs.release()); return s; };
    if (st) cs->st = st;
    else {
        q3_relax_capture_mode();
        const hipError_t e = hipStreamCreateWithFlags(&cs->st, hipStreamNonBlocking);
        if (e != hipSuccess) { cs->st = nullptr; return fail(set_err(Q3_HIP_ERROR, "hipStreamCreateWithFlags: %s", hipGetErrorString(e))); }
        cs->owns_stream = true;
    }
    if (dev_malloc((void**)&cs->cs, (size_t)max_frames * 32 * 4) != hipSuccess || dev_malloc((void**)&cs->sn, (size_t)max_frames * 32 * 4) != hipSuccess)
        return fail(set_err(Q3_OOM, "q3_codec_stream_create: RoPE table of %d frames", max_frames));
    const q3_status s = codec_rope_table(m->cfg, max_frames, cs->cs, cs->sn);
    if (s != Q3_OK) return fail(s);
    *out = cs.release();
    return Q3_OK;
}

extern "C" q3_status q3_codec_stream_create(q3_model* m, int rows, int max_frames, q3_codec_stream** out) {
    return codec_stream_create(m, rows, max_frames, nullptr, out);
}

extern "C" q3_status q3_codec_stream_create_blocked(q3_model* m, int rows, int max_frames, int block_frames, int max_blocks, q3_codec_stream** out) {
    if (block_frames < 32 || block_frames % 32 != 0)
        return set_err(Q3_INVALID_ARG, "q3_codec_stream_create_blocked: block_frames %d is not a positive multiple of 32 (a 32-key attention tile must lie inside one block)", block_frames);
    if (max_blocks < 0) return set_err(Q3_INVALID_ARG, "q3_codec_stream_create_blocked: negative max_blocks");
    return codec_stream_create(m, rows, max_frames, nullptr, out, block_frames, max_blocks);
}
extern "C" q3_status q3_codec_stream_info(q3_codec_stream* cs, int* block_frames, size_t* block_bytes, int* blocks_total, int* blocks_in_use, int* blocks_peak) {
    if (!cs) return set_err(Q3_INVALID_ARG, "q3_codec_stream_info: null stream");
    if (block_frames) *block_frames = cs->bf;
    if (block_bytes) *block_bytes = block_floats(cs) * 4;
    if (blocks_total) *blocks_total = cs->blocks_total;
    if (blocks_in_use) *blocks_in_use = cs->blocks_in_use;
    if (blocks_peak) *blocks_peak = cs->blocks_peak;
    return Q3_OK;
}

extern "C" void q3_codec_stream_free(q3_codec_stream* cs) {
    if (!cs) return;
    q3_model* m = cs->m;
    (void)hipSetDevice(m->device);
    if (cs->st) (void)hipStreamSynchronize(cs->st);
    for (CsRow& r : cs->rows) { dev_free(r.kv); dev_free(r.lat); dev_free(r.hist); for (float* b : r.blocks) dev_free(b); }
    for (float* b : cs->free_blocks) dev_free(b);
    cs->ws.release();
    dev_free(cs->cs); dev_free(cs->sn); dev_free(cs->desc); dev_free(cs->stage);
    if (cs->stage_host) (void)hipHostFree(cs->stage_host);
    if (cs->owns_stream && cs->st) (void)hipStreamDestroy(cs->st);
    delete cs;
    if (m->refs.fetch_sub(1) == 1) model_destroy(m);
}

int codec_stream_pos(const q3_codec_stream* cs, int row) { return cs->rows[row].pos; }
// blocked stream: the blocks row holds, and how many more it takes to reach frame `upto` (0 / 0 on an unblocked stream)
void codec_stream_blocks(const q3_codec_stream* cs, int row, int upto, int* held, int* need) {
    const CsRow& r = cs->rows[row];
    *held = (int)r.blocks.size();
    *need = cs->bf ? std::max(0, (upto + cs->bf - 1) / cs->bf - *held) : 0;
}
// the caches are only read below pos; a blocked row's blocks go back to the free list (no push is in flight: each ends with a wait)
void codec_stream_reset(q3_codec_stream* cs, int row) {
    CsRow& r = cs->rows[row];
    r.pos = 0;
    cs->blocks_in_use -= (int)r.blocks.size();
    cs->free_blocks.insert(cs->free_blocks.end(), r.blocks.begin(), r.blocks.end());
    r.blocks.clear();
}

extern "C" q3_status q3_codec_stream_reset(q3_codec_stream* cs, int row) {
    if (!cs || row < 0 || row >= cs->R) return set_err(Q3_INVALID_ARG, "q3_codec_stream_reset: bad row");
    codec_stream_reset(cs, row);
    return Q3_OK;
}
extern "C" q3_status q3_codec_stream_pos(q3_codec_stream* cs, int row, int* n_frames) {
    if (!cs || row < 0 || row >= cs->R || !n_frames) return set_err(Q3_INVALID_ARG, "q3_codec_stream_pos: bad row");
    *n_frames = cs->rows[row].pos;
    return Q3_OK;
}

namespace {
// the descriptor block of a push: arrays laid out back to back on the host, uploaded once, addressed by offset on the device
struct DescBlock {
    std::vector<char> host;
    template <typename T> size_t add(const std::vector<T>& v) {
        const size_t off = (host.size() + 15) & ~(size_t)15;
        host.resize(off + v.size() * sizeof(T));
        if (!v.empty()) memcpy(host.data() + off, v.data(), v.size() * sizeof(T));
        return off;
    }
};
}  // namespace

// Every row at most once, 0 <= row < R, pos + n <= cap, codes on the host (all rows) or on the device (all rows): checked by the
// callers' entry points, which refuse before anything changes. pcm_host[i] receives the (n - skip) * spf samples of the row's last
// n - skip frames.
// Rows that name an output stage (CsPush::ps, one stage per push): their samples go through it on the stream's stream, behind the
// copy that gathers them and in front of the copy to the host, which then carries the converted bytes. The stage's descriptors
// ride in this push's descriptor block. The stage's rows move on only when the push has succeeded; nothing here restarts them.
q3_status codec_stream_push(q3_codec_stream* cs, const std::vector<CsPush>& all) {
    q3_model* m = cs->m;
    const q3_config& c = m->cfg;
    std::vector<CsPush> P;
    for (const CsPush& p : all) if (p.n > 0) P.push_back(p);
    q3_pcm_stage* ps = nullptr;
    std::vector<const CsPush*> flush;                       // no frames, but the row's stage row ends: only its tail comes out
    for (const CsPush& p : all) {
        if (p.ps) ps = p.ps;
        if (p.n_out) *p.n_out = 0;
        if (p.n <= 0 && p.ps && p.last) flush.push_back(&p);
    }
    if (P.empty()) {
        if (flush.empty()) return Q3_OK;
        std::vector<PsSeg> segs; std::vector<void*> outs; std::vector<size_t> cnt(flush.size(), 0);
        for (const CsPush* f : flush) { segs.push_back({f->ps_row, nullptr, 0, 1}); outs.push_back(f->out_host); }
        Q3C(pcm_stage_push_dev(ps, segs, cs->st, outs.data(), cnt.data()));
        for (size_t k = 0; k < flush.size(); ++k) if (flush[k]->n_out) *flush[k]->n_out = cnt[k];
        return Q3_OK;
    }
    HIPC(hipSetDevice(m->device));
    hipStream_t st = cs->st;
    const int Q = c.dec_q_dim, LAT = c.dec_latent, QD = c.dec_heads * c.dec_head_dim, cap = cs->cap, spf = samples_per_frame(c);
    const int nP = (int)P.size();
    const bool on_dev = P[0].dev != nullptr;
    const int bf = cs->bf, kp = bf ? bf : cap;              // pitch of a row's K / V / latent columns
    const size_t lat_off = (size_t)c.dec_layers * 2 * QD * bf;      // blocked: the latent inside a block
    // A push that returns before its rows' positions move (a workspace, staging or descriptor allocation that fails below) gives the
    // blocks it took back: a row never holds more than ceil(pos / bf), whatever the way out.
    struct Untake {
        q3_codec_stream* cs; const std::vector<CsPush>& P; bool armed = true;
        ~Untake() {
            if (!armed || !cs->bf) return;
            for (const CsPush& p : P) {
                CsRow& r = cs->rows[p.row];
                while ((int)r.blocks.size() > (r.pos + cs->bf - 1) / cs->bf) { cs->free_blocks.push_back(r.blocks.back()); r.blocks.pop_back(); cs->blocks_in_use--; }
            }
        }
    } untake{cs, P};
    if (bf) {
        // the blocks this push reaches: all of them or none, before anything changes
        int need = 0;
        for (const CsPush& p : P) {
            const CsRow& r = cs->rows[p.row];
            need += std::max(0, (r.pos + p.n + bf - 1) / bf - (int)r.blocks.size());
        }
        if (cs->max_blocks > 0 && cs->blocks_in_use + need > cs->max_blocks)
            return set_err(Q3_OOM, "codec stream: block pool exhausted: the push needs %d more block(s) of %d frames, %d of %d are in use",
                           need, bf, cs->blocks_in_use, cs->max_blocks);
        while ((int)cs->free_blocks.size() < need) {
            float* b = nullptr;
            if (dev_malloc((void**)&b, block_floats(cs) * 4) != hipSuccess) {
                (void)hipGetLastError();
                return set_err(Q3_OOM, "codec stream: block %d (%zu KB each)", cs->blocks_total, block_floats(cs) * 4 >> 10);
            }
            cs->free_blocks.push_back(b); cs->blocks_total++;
        }
        for (const CsPush& p : P) {
            CsRow& r = cs->rows[p.row];
            if (!r.hist && dev_malloc((void**)&r.hist, (size_t)Q * 2 * 4) != hipSuccess) {
                (void)hipGetLastError(); r.hist = nullptr;
                return set_err(Q3_OOM, "codec stream: history columns of row %d", p.row);
            }
        }
        for (const CsPush& p : P) {
            CsRow& r = cs->rows[p.row];
            while ((int)r.blocks.size() * bf < r.pos + p.n) { r.blocks.push_back(cs->free_blocks.back()); cs->free_blocks.pop_back(); cs->blocks_in_use++; }
        }
    }
    // row state on first use
    for (const CsPush& p : P) {
        CsRow& r = cs->rows[p.row];
        if (bf || r.kv) continue;
        if (dev_malloc((void**)&r.kv, kv_floats(cs) * 4) != hipSuccess || dev_malloc((void**)&r.lat, (size_t)LAT * cap * 4) != hipSuccess ||
            dev_malloc((void**)&r.hist, (size_t)Q * 2 * 4) != hipSuccess) {
            (void)hipGetLastError();
            dev_free(r.kv); dev_free(r.lat); dev_free(r.hist); r.kv = r.lat = r.hist = nullptr;
            return set_err(Q3_OOM, "codec stream: state of row %d (%zu MB)", p.row, (kv_floats(cs) + (size_t)LAT * cap) * 4 >> 20);
        }
    }
    // the plan: new columns N (front), Np with two history columns per row (pre_conv), the stack's concatenation Lc and the
    // rows that run the stack alone
    // (a push may carry `skip` leading frames that only bring the row's state up to date: the front takes them, the stack and
    // the samples start behind them, at a0)
    int N = 0, W = 0, Lc = 0, solo_max = 0, max_tiles = 0;
    std::vector<int> col0(nP), out0(nP), conc, solo;
    for (int i = 0; i < nP; ++i) {
        const int f0 = cs->rows[P[i].row].pos, a0 = f0 + P[i].skip, e = f0 + P[i].n;
        col0[i] = N; N += P[i].n;
        out0[i] = W; W += e - a0;
        if (e > a0) {
            if (a0 > CODEC_CTX_FRAMES) { conc.push_back(i); Lc += e - a0 + CODEC_CTX_FRAMES; }
            else { solo.push_back(i); solo_max = std::max(solo_max, e); }
        }
        max_tiles = std::max(max_tiles, ((e - 1) >> 5) - (f0 >> 5) + 1);
    }
    const int Np = N + 2 * nP;
    {
        // the workspace is sized for every row of the stream pushing what the widest row of this push does (a session's steady
        // state: rows x (chunk + context)), so it is reserved once and not again as rows join; a long catch-up push does not
        // multiply by the rows beyond CS_WIDE frames
        const int CS_WIDE = 2048;
        int max_n = 0; for (const CsPush& p : P) max_n = std::max(max_n, p.n);
        const int T = std::max(1, std::max(Lc, solo_max));
        const long long Tw = (long long)cs->R * (max_n + CODEC_CTX_FRAMES), Fw = (long long)cs->R * (max_n + 2);
        Q3C(codec_reserve(m, cs->ws, (int)std::max<long long>(T, std::min<long long>(Tw, CS_WIDE)),
                          (int)std::max<long long>(Np, std::min<long long>(Fw, CS_WIDE))));
    }
    CodecWS& ws = cs->ws;
    if ((size_t)W * spf > cs->stage_cap) {
        HIPC(hipStreamSynchronize(st));
        dev_free(cs->stage); cs->stage = nullptr;
        if (cs->stage_host) { (void)hipHostFree(cs->stage_host); cs->stage_host = nullptr; }
        cs->stage_cap = 0;
        HIPC(dev_malloc((void**)&cs->stage, (size_t)W * spf * 4));
        HIPC(hipHostMalloc((void**)&cs->stage_host, (size_t)W * spf * 4, hipHostMallocDefault));
        cs->stage_cap = (size_t)W * spf;
    }
    // the output stage's part of the plan: the delivered samples of its rows, where launch_copy_segs puts them
    std::vector<PsSeg> psegs; std::vector<const CsPush*> pseg_of; std::vector<void*> pouts; PsPlan plan;
    if (ps) {
        for (int i = 0; i < nP; ++i)
            if (P[i].ps) { psegs.push_back({P[i].ps_row, cs->stage + (size_t)out0[i] * spf, (size_t)(P[i].n - P[i].skip) * spf, P[i].last}); pseg_of.push_back(&P[i]); }
        for (const CsPush* f : flush) { psegs.push_back({f->ps_row, nullptr, 0, 1}); pseg_of.push_back(f); }
        for (const CsPush* p : pseg_of) pouts.push_back(p->out_host);
        // (with a silence step on some row, DESIGN 4.12e, what the rows hand on is known once their samples exist: plan.desc is
        // then empty here, and the stage plans behind the vocoder, in pcm_stage_run)
        Q3C(pcm_stage_begin(ps, psegs, plan));
    }
    float *A = ws.bufA, *B = ws.bufB, *C = ws.bufC, *F = ws.bufF;
    float* knew = A + (size_t)QD * N;                       // k | v of the new columns, [2*QD][N] (codec_front_transformer)
    // descriptors
    std::vector<int> pos(N);
    std::vector<AttnCsRow> arows(nP);
    std::vector<ColCopy> xin(Np), hist(2 * nP), compact(N), kvsc(N), latsc(N), latg(Lc), solog;
    std::vector<SegCopy> segs;
    std::vector<AttnCbRow> brows(bf ? nP : 0);
    std::vector<const float*> tabs;                         // blocked: the block lists of the pushed rows, back to back
    // frame f of a row: its K column of layer 0 (the layer and V are offsets of the copy / the kernel) and its latent column
    auto kv_col = [&](const CsRow& r, int f) { return bf ? r.blocks[f / bf] + f % bf : r.kv + f; };
    auto lat_col = [&](const CsRow& r, int f) { return bf ? r.blocks[f / bf] + lat_off + f % bf : r.lat + f; };
    std::vector<const uint32_t*> fsrc(on_dev ? N : 0);
    std::vector<uint32_t> fhost(on_dev ? 0 : (size_t)N * 16);
    for (int i = 0; i < nP; ++i) {
        const CsRow& r = cs->rows[P[i].row];
        const int f0 = r.pos, n = P[i].n, x0 = col0[i] + 2 * i;      // x0: the row's first column in the pre_conv input
        arows[i] = {r.kv, f0, f0 + n, col0[i]};
        if (bf) { brows[i] = {(int)tabs.size(), f0, f0 + n, col0[i]}; tabs.insert(tabs.end(), r.blocks.begin(), r.blocks.end()); }
        // pre_conv input: the two columns before f0 (zeros before the row's frame 0: the causal pad), then the new ones
        for (int h = 0; h < 2; ++h) xin[x0 + h] = {f0 - 2 + h >= 0 ? r.hist + h : nullptr, A + x0 + h, 2, Np};
        // ... whose last two columns are the next push's history
        for (int h = 0; h < 2; ++h) hist[2 * i + h] = {A + x0 + n + h, r.hist + h, Np, 2};
        for (int j = 0; j < n; ++j) {
            const int col = col0[i] + j;
            pos[col] = f0 + j;
            xin[x0 + 2 + j] = {B + col, A + x0 + 2 + j, N, Np};
            compact[col] = {B + x0 + 2 + j, C + col, Np, N};
            kvsc[col] = {knew + col, kv_col(r, f0 + j), N, kp};
            latsc[col] = {C + col, lat_col(r, f0 + j), N, kp};
            if (on_dev) fsrc[col] = P[i].dev + (size_t)j * 16;
            else memcpy(&fhost[(size_t)col * 16], P[i].host + (size_t)j * 16, 64);
        }
    }
    {
        int l0 = 0;
        for (int i : conc) {
            const CsRow& r = cs->rows[P[i].row];
            const int a0 = r.pos + P[i].skip, c0 = a0 - CODEC_CTX_FRAMES, len = P[i].n - P[i].skip + CODEC_CTX_FRAMES;
            for (int j = 0; j < len; ++j) latg[l0 + j] = {lat_col(r, c0 + j), F + l0 + j, kp, Lc};
            segs.push_back({(unsigned long long)(l0 + CODEC_CTX_FRAMES) * spf, (unsigned long long)out0[i] * spf, (unsigned long long)(P[i].n - P[i].skip) * spf});
            l0 += len;
        }
        for (int i : solo) {
            // blocked: the row's latent [0, e) is gathered column by column (e may lie past a block edge)
            const CsRow& r = cs->rows[P[i].row];
            const int e = r.pos + P[i].n;
            if (bf) for (int f = 0; f < e; ++f) solog.push_back({lat_col(r, f), F + f, kp, e});
            segs.push_back({(unsigned long long)(cs->rows[P[i].row].pos + P[i].skip) * spf, (unsigned long long)out0[i] * spf,
                            (unsigned long long)(P[i].n - P[i].skip) * spf});
        }
    }
    DescBlock db;
    const size_t o_pos = db.add(pos), o_arows = db.add(arows), o_xin = db.add(xin), o_hist = db.add(hist), o_compact = db.add(compact),
                 o_kvsc = db.add(kvsc), o_latsc = db.add(latsc), o_latg = db.add(latg), o_segs = db.add(segs), o_fsrc = db.add(fsrc),
                 o_brows = db.add(brows), o_tabs = db.add(tabs), o_solog = db.add(solog), o_ps = db.add(plan.desc);
    if (db.host.size() > cs->desc_cap) {
        HIPC(hipStreamSynchronize(st));
        dev_free(cs->desc); cs->desc = nullptr; cs->desc_cap = 0;
        HIPC(dev_malloc((void**)&cs->desc, db.host.size() * 2));
        cs->desc_cap = db.host.size() * 2;
    }
    // (the stream is idle here: every push ends with a wait for it, a failed one in `failed`)
    // From here on the rows' state is written on the device (history columns, K/V, latent) before pos moves: a push that fails
    // past this point waits for the stream and leaves its rows at frame 0, so that stale state is never read as current (a
    // session's next call catches such a row up from its codes).
    struct Failed {
        q3_codec_stream* cs; const std::vector<CsPush>& P; bool armed = true;
        ~Failed() {
            if (!armed) return;
            (void)hipStreamSynchronize(cs->st);
            for (const CsPush& p : P) codec_stream_reset(cs, p.row);
        }
    } failed{cs, P};
    HIPC(q3_hipMemcpy(cs->desc, db.host.data(), db.host.size(), hipMemcpyHostToDevice));
    auto D = [&](size_t off) { return (const void*)(cs->desc + off); };
    if (on_dev) HIPC(launch_gather_frames((const uint32_t* const*)D(o_fsrc), ws.frames, N, st));
    else HIPC(q3_hipMemcpy(ws.frames, fhost.data(), fhost.size() * 4, hipMemcpyHostToDevice));

    const CodecScope scope(m);
    // front over the new columns
    Q3C(codec_front_quant(m, ws, N, st));                                             // B [Q][N]
    HIPC(launch_copy_cols((const ColCopy*)D(o_xin), Np, Q, 0, 0, st));                 // A [Q][Np]: history | new, per row
    HIPC(launch_copy_cols((const ColCopy*)D(o_hist), 2 * nP, Q, 0, 0, st));
    Q3C(codec_front_preconv(m, A, B, Np, st));                                        // B [LAT][Np]
    HIPC(launch_copy_cols((const ColCopy*)D(o_compact), N, LAT, 0, 0, st));            // C [LAT][N]: the history columns' outputs dropped
    const float scale = (float)pow((double)c.dec_head_dim, -0.5);
    Q3C(codec_front_transformer(m, ws, N, st, [&](int l, float* q, float* k, float*, float* ao) -> q3_status {
        const size_t layer_off = (size_t)l * 2 * QD * kp;
        HIPC(launch_rope_c_pos(q, k, cs->cs, cs->sn, (const int*)D(o_pos), c.dec_heads, c.dec_head_dim, N, st));
        HIPC(launch_copy_cols((const ColCopy*)D(o_kvsc), N, 2 * QD, 0, layer_off, st));
        if (bf) HIPC(launch_attn_cb(q, ao, (const AttnCbRow*)D(o_brows), (const float* const*)D(o_tabs), nP, max_tiles, layer_off, c.dec_heads, c.dec_head_dim, N, bf, scale, st));
        else HIPC(launch_attn_cs(q, ao, (const AttnCsRow*)D(o_arows), nP, max_tiles, layer_off, c.dec_heads, c.dec_head_dim, N, cap, scale, st));
        return Q3_OK;
    }));
    HIPC(launch_copy_cols((const ColCopy*)D(o_latsc), N, LAT, 0, 0, st));
    // the convolutional stack: once over the rows past their context, concatenated; alone for each row that is not
    const SegCopy* dsegs = (const SegCopy*)D(o_segs);
    if (!conc.empty()) {
        size_t max_n = 0; for (int i : conc) max_n = std::max(max_n, (size_t)(P[i].n - P[i].skip) * spf);
        HIPC(launch_copy_cols((const ColCopy*)D(o_latg), Lc, LAT, 0, 0, st));
        Q3C(codec_stack_dev(m, ws, F, Lc, st, nullptr, scope));
        HIPC(launch_copy_segs(ws.pcm, cs->stage, dsegs, (int)conc.size(), max_n, st));
    }
    for (size_t k = 0, g0 = 0; k < solo.size(); ++k) {
        const int i = solo[k]; const CsRow& r = cs->rows[P[i].row];
        const int e = r.pos + P[i].n;
        if (bf) { HIPC(launch_copy_cols((const ColCopy*)D(o_solog) + g0, e, LAT, 0, 0, st)); g0 += (size_t)e; }
        else HIPC(launch_copy_rows(r.lat, cap, F, e, LAT, e, st));
        Q3C(codec_stack_dev(m, ws, F, e, st, nullptr, scope));
        HIPC(launch_copy_segs(ws.pcm, cs->stage, dsegs + conc.size() + k, 1, (size_t)(P[i].n - P[i].skip) * spf, st));
    }
    bool raw = false;                                       // rows that take their 24 kHz f32 as it is (every row, without a stage)
    for (int i = 0; i < nP; ++i) raw = raw || !P[i].ps;
    if (W > 0 && raw) HIPC(hipMemcpyAsync(cs->stage_host, cs->stage, (size_t)W * spf * 4, hipMemcpyDeviceToHost, st));
    if (ps) Q3C(pcm_stage_run(ps, psegs, plan, (const PsDesc*)D(o_ps), st));      // (with a silence step: waits for the stream once, its kept counts come back)
    HIPC(hipStreamSynchronize(st));
    if (ps) pcm_stage_finish(ps, psegs, plan, pouts.data(), nullptr);
    for (size_t k = 0; k < psegs.size(); ++k) if (pseg_of[k]->n_out) *pseg_of[k]->n_out = plan.count[k];
    for (int i = 0; i < nP; ++i) {
        if (P[i].pcm_host && !P[i].ps) memcpy(P[i].pcm_host, cs->stage_host + (size_t)out0[i] * spf, (size_t)(P[i].n - P[i].skip) * spf * 4);
        cs->rows[P[i].row].pos += P[i].n;
    }
    failed.armed = false; untake.armed = false;
    cs->blocks_peak = std::max(cs->blocks_peak, cs->blocks_in_use);
    return Q3_OK;
}

extern "C" q3_status q3_codec_stream_push(q3_codec_stream* cs, int n_rows, const int* rows, const uint32_t* const* frames_host,
                                          const int* n_frames, float* const* pcm_host, const size_t* cap) {
    if (!cs) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push: null stream");
    if (n_rows < 0 || (n_rows > 0 && (!rows || !frames_host || !n_frames || !pcm_host || !cap)))
        return set_err(Q3_INVALID_ARG, "q3_codec_stream_push: null argument");
    const int spf = samples_per_frame(cs->m->cfg);
    std::vector<char> seen(cs->R, 0);
    std::vector<CsPush> P;
    for (int i = 0; i < n_rows; ++i) {
        const int r = rows[i], n = n_frames[i];
        if (r < 0 || r >= cs->R) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push: row %d out of range (%d rows)", r, cs->R);
        if (seen[r]) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push: row %d listed twice", r);
        seen[r] = 1;
        if (n < 0) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push: negative frame count for row %d", r);
        if (n == 0) continue;
        if (cs->rows[r].pos + n > cs->cap)
            return set_err(Q3_INVALID_ARG, "q3_codec_stream_push: row %d would reach %d frames, the stream holds %d", r, cs->rows[r].pos + n, cs->cap);
        if (!frames_host[i] || !pcm_host[i]) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push: null frames or pcm pointer for row %d", r);
        if (cap[i] < (size_t)n * spf) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push: pcm buffer of row %d too small (%zu < %zu samples)", r, cap[i], (size_t)n * spf);
        for (int f = 0; f < n; ++f)
            for (int g = 1; g < 16; ++g)
                if (frames_host[i][(size_t)f * 16 + g] >= (uint32_t)cs->m->cfg.dec_cb_size)
                    return set_err(Q3_INVALID_ARG, "code %u out of range for codebook %d (row %d, frame %d)", frames_host[i][(size_t)f * 16 + g], g, r, f);
        P.push_back({r, n, 0, frames_host[i], nullptr, pcm_host[i]});
    }
    return codec_stream_push(cs, P);
}

extern "C" q3_status q3_codec_stream_push_out(q3_codec_stream* cs, int n_rows, const int* rows, const uint32_t* const* frames_host, const int* n_frames,
                                              q3_pcm_stage* ps, const int* ps_rows, const int* last,
                                              void* const* out_host, const size_t* cap_samples, size_t* n_samples) {
    if (!cs) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: null stream");
    if (!ps) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: null stage");
    if (n_rows < 0 || (n_rows > 0 && (!rows || !frames_host || !n_frames || !ps_rows || !out_host || !cap_samples || !n_samples)))
        return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: null argument");
    Q3C(pcm_stage_check_rows(ps, "q3_codec_stream_push_out", n_rows, ps_rows));
    const int spf = samples_per_frame(cs->m->cfg);
    std::vector<char> seen(cs->R, 0);
    std::vector<CsPush> P;
    for (int i = 0; i < n_rows; ++i) {
        const int r = rows[i], n = n_frames[i], lst = last ? last[i] : 0;
        if (r < 0 || r >= cs->R) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: row %d out of range (%d rows)", r, cs->R);
        if (seen[r]) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: row %d listed twice", r);
        seen[r] = 1;
        n_samples[i] = 0;
        if (n < 0) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: negative frame count for row %d", r);
        if (n == 0 && !lst) continue;
        if (cs->rows[r].pos + n > cs->cap)
            return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: row %d would reach %d frames, the stream holds %d", r, cs->rows[r].pos + n, cs->cap);
        if (n > 0 && !frames_host[i]) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: null frames pointer for row %d", r);
        const size_t cnt = pcm_stage_count(ps, ps_rows[i], (size_t)n * spf, lst);
        if (cap_samples[i] < cnt) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: output buffer of row %d too small (%zu < %zu samples)", r, cap_samples[i], cnt);
        if (cnt > 0 && !out_host[i]) return set_err(Q3_INVALID_ARG, "q3_codec_stream_push_out: null output pointer for row %d", r);
        for (int f = 0; f < n; ++f)
            for (int g = 1; g < 16; ++g)
                if (frames_host[i][(size_t)f * 16 + g] >= (uint32_t)cs->m->cfg.dec_cb_size)
                    return set_err(Q3_INVALID_ARG, "code %u out of range for codebook %d (row %d, frame %d)", frames_host[i][(size_t)f * 16 + g], g, r, f);
        CsPush p{r, n, 0, frames_host[i], nullptr, nullptr};
        p.ps = ps; p.ps_row = ps_rows[i]; p.last = lst; p.out_host = out_host[i]; p.n_out = &n_samples[i];
        P.push_back(p);
    }
    return codec_stream_push(cs, P);
}

extern "C" q3_status q3_codec_stream_prime(q3_codec_stream* cs, int row, const uint32_t* frames_host, int n_frames) {
    if (!cs) return set_err(Q3_INVALID_ARG, "q3_codec_stream_prime: null stream");
    if (row < 0 || row >= cs->R) return set_err(Q3_INVALID_ARG, "q3_codec_stream_prime: row %d out of range (%d rows)", row, cs->R);
    if (cs->rows[row].pos != 0) return set_err(Q3_INVALID_ARG, "q3_codec_stream_prime: row %d is at frame %d, state-only frames come first", row, cs->rows[row].pos);
    if (n_frames < 0 || (n_frames > 0 && !frames_host)) return set_err(Q3_INVALID_ARG, "q3_codec_stream_prime: bad frames argument");
    if (n_frames > cs->cap) return set_err(Q3_INVALID_ARG, "q3_codec_stream_prime: %d frames, the stream holds %d", n_frames, cs->cap);
    for (int f = 0; f < n_frames; ++f)
        for (int g = 1; g < 16; ++g)
            if (frames_host[(size_t)f * 16 + g] >= (uint32_t)cs->m->cfg.dec_cb_size)
                return set_err(Q3_INVALID_ARG, "code %u out of range for codebook %d (row %d, frame %d)", frames_host[(size_t)f * 16 + g], g, row, f);
    // a push whose frames are all `skip`: the front fills the caches, no stack runs and there are no samples
    return codec_stream_push(cs, {CsPush{row, n_frames, n_frames, frames_host, nullptr, nullptr}});
}
