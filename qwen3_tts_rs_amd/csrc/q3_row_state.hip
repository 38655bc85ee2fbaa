// q3_row_state.hip — a running row's state as an object: k_row_move (one launch per exchange), q3_session_park_row / _resume_row,
// q3_parked_* (the kernel's op-level test entry q3_row_move is in q3_testapi.hip)
// (one of the units of the engine: q3_engine.h says which holds what)
#include "q3_engine.h"
#include "q3_prefix_cache.h"

// ------------------------------------------------------------------------------------------------
// k_row_move: a table of byte segments {src, dst, bytes, mode}, one launch. Grid = (16-byte tiles, segment); a segment's tiles
// are walked with a grid stride, so one launch serves a 4-byte counter and an 8 MB run of text rows alike.
//   body   16-byte vector accesses when src and dst share their offset within 16 bytes (after the head both are aligned);
//          4-byte words when they only share it within 4; single bytes otherwise
//   head   the bytes in front of dst's next 16-byte (4-byte) boundary, tail: what the body's unit leaves over — single bytes, by
//          the first threads of the segment's first block
// mode ROW_MOVE_EXCHANGE swaps the two runs (both are read, then both written, element by element; the runs of one launch must
// not overlap one another). Plain loads and stores only: the launch sits between two frames, on the session's stream, with a
// stream synchronisation behind it — where transplant_row's copies sit.
// ------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void row_move_unit(int mode, char* src, char* dst, unsigned long long i) {
    T* ps = reinterpret_cast<T*>(src) + i; T* pd = reinterpret_cast<T*>(dst) + i;
    const T v = *ps;
    if (mode == ROW_MOVE_EXCHANGE) { const T w = *pd; *pd = v; *ps = w; }
    else *pd = v;
}
__global__ __launch_bounds__(256) void k_row_move(const RowSeg* __restrict__ segs) {
    const RowSeg s = segs[blockIdx.y];
    if (s.bytes == 0) return;
    char* src = (char*)s.src; char* dst = (char*)s.dst;
    const unsigned long long sa = (unsigned long long)src, da = (unsigned long long)dst;
    // the widest unit both runs can be walked in
    const unsigned unit = ((sa ^ da) & 15) == 0 ? 16u : ((sa ^ da) & 3) == 0 ? 4u : 1u;
    unsigned long long head = (unit - (unsigned)(da & (unit - 1))) & (unit - 1);
    if (head > s.bytes) head = s.bytes;
    const unsigned long long n_body = (s.bytes - head) / unit, tail0 = head + n_body * unit, n_tail = s.bytes - tail0;
    const unsigned long long i0 = (unsigned long long)blockIdx.x * 256 + threadIdx.x, step = (unsigned long long)gridDim.x * 256;
    if (unit == 16) { for (unsigned long long i = i0; i < n_body; i += step) row_move_unit<uint4>(s.mode, src + head, dst + head, i); }
    else if (unit == 4) { for (unsigned long long i = i0; i < n_body; i += step) row_move_unit<uint32_t>(s.mode, src + head, dst + head, i); }
    else { for (unsigned long long i = i0; i < n_body; i += step) row_move_unit<uint8_t>(s.mode, src + head, dst + head, i); }
    if (blockIdx.x == 0) {           // head and tail: fewer than 16 bytes each
        if (threadIdx.x < head) row_move_unit<uint8_t>(s.mode, src, dst, threadIdx.x);
        else if (threadIdx.x >= 32 && threadIdx.x - 32 < n_tail) row_move_unit<uint8_t>(s.mode, src + tail0, dst + tail0, threadIdx.x - 32);
    }
}
hipError_t launch_row_move(const RowSeg* segs_dev, int n_segs, size_t max_bytes, hipStream_t st) {
    if (n_segs <= 0 || n_segs > 65535) return hipErrorInvalidValue;
    size_t gx = (max_bytes + 4095) / 4096;      // 256 threads x 16 bytes per pass
    if (gx < 1) gx = 1; if (gx > 512) gx = 512;
    hipLaunchKernelGGL(k_row_move, dim3((unsigned)gx, (unsigned)n_segs), dim3(256), 0, st, segs_dev);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Park and resume (no reference counterpart: the reference runs one utterance per call to its end). A record takes everything of a
// row that crosses a frame boundary — what the captured frame (frame_launch, q3_session.hip) reads before it writes:
//   cp_run          LASTH (pass 0), tok (the semantic embedding), codes[frame_idx] (written this frame), frame_idx
//   k_frame_embed   tok, frame_idx, trail_base / trail_len / pad_row and the text rows they name, text_ready
//   talker_step     pos, the row's K/V pages (positions 0 .. pos), LASTH of a held row (kept by rmsnorm_hold)
//   k_sample        seen, the row's U stripe at token_count, limit, text_ready, sample_rows[b]; it advances tok, token_count,
//                   frame_idx, pos
// plus LOGITS (Q3_GET_LOGITS), the codes committed so far and the host SeqInfo. Not in the set: tb / cb activations, CP_IN,
// CP_LOGITS and the code predictor's K/V — every frame writes them (from position 0) before it reads them.
// The pages are not copied: the row's page list moves into the record and back. The device state goes through k_row_move into ONE
// block of the device-memory cache (dev_malloc: blocks kept per device and size, so a record may outlive its session).
// ------------------------------------------------------------------------------------------------
struct q3_parked {
    q3_model* m = nullptr; uint64_t session_uid = 0; int B = 0, max_frames = 0, H = 0, V = 0;
    SeqInfo seq; int committed = 0, n_frames = 0; bool done = false;
    std::vector<float*> pages; bool pages_bf16 = false;
    char* stash = nullptr; size_t stash_bytes = 0, block = 0; std::shared_ptr<ParkShelf> shelf;      // block: the stash's allocated size
    std::vector<uint32_t> codes_host;           // committed x 16 (q3_parked_codes: a parked ticket that is cancelled)
    // byte offsets of the parts within the stash (each a multiple of 16)
    size_t o_lasth = 0, o_logits = 0, o_seen = 0, o_u = 0, o_codes = 0, o_text = 0, o_pad = 0, o_scalars = 0;
    int n_text_rows = 0; bool has_ready = false;
};
// the stash's scalars, 16 bytes apart: tok, token_count, pos, frame_idx, limit, trail_len, text_ready, then the SampleRow
enum { PS_TOK = 0, PS_COUNT, PS_POS, PS_FIDX, PS_LIMIT, PS_TLEN, PS_READY, PS_SROW, PS_N };
static size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }
// the segments between row b and a stash, in one direction; trail rows / pad row live at `trail_row` / `pad_row` of s->rows
static void park_segments(q3_session* s, int b, const q3_parked& p, int trail_row, int pad_row, bool to_stash, std::vector<RowSeg>& out, size_t* max_bytes) {
    const int H = p.H, V = p.V;
    auto add = [&](void* row_side, size_t off, size_t bytes) {
        if (bytes == 0) return;
        out.push_back(to_stash ? RowSeg{row_side, p.stash + off, bytes, ROW_MOVE_COPY, 0} : RowSeg{p.stash + off, row_side, bytes, ROW_MOVE_COPY, 0});
        if (bytes > *max_bytes) *max_bytes = bytes;
    };
    add(s->LASTH + (size_t)b * H, p.o_lasth, (size_t)H * 4);
    add(s->LOGITS + (size_t)b * V, p.o_logits, (size_t)V * 4);
    add(s->seen + (size_t)b * V, p.o_seen, (size_t)V);
    add(s->U + (size_t)b * (s->max_frames + 2), p.o_u, (size_t)(s->max_frames + 2) * 4);
    add(s->codes + (size_t)b * s->max_frames * 16, p.o_codes, (size_t)p.committed * 64);
    add(s->rows + (size_t)trail_row * H, p.o_text, (size_t)p.n_text_rows * H * 4);
    add(s->rows + (size_t)pad_row * H, p.o_pad, (size_t)H * 4);
    add(s->tok + b, p.o_scalars + 16 * PS_TOK, 4);
    add(s->token_count + b, p.o_scalars + 16 * PS_COUNT, 4);
    add(s->pos + b, p.o_scalars + 16 * PS_POS, 4);
    add(s->frame_idx + b, p.o_scalars + 16 * PS_FIDX, 4);
    add(s->limit + b, p.o_scalars + 16 * PS_LIMIT, 4);
    add(s->trail_len + b, p.o_scalars + 16 * PS_TLEN, 4);
    // (a record parked before the session had open-text state carries no text_ready: the resume writes "closed" itself)
    if (p.has_ready && s->text_ready) add(s->text_ready + b, p.o_scalars + 16 * PS_READY, 4);
    add(s->sample_rows + b, p.o_scalars + 16 * PS_SROW, sizeof(SampleRow));
}
// descriptors (+ a few host-made ints behind them) in one upload to the session's table, then the one launch
static_assert(sizeof(RowSeg) == 32, "PARK_DESC_BYTES counts 32-byte descriptors");
// a record's device block: from the session's shelf, else from the device-memory cache (only while the session has never had as
// many blocks of that size out at once); back to the shelf while the session lives
static hipError_t stash_take(q3_session* s, size_t block, char** out) {
    {
        std::lock_guard<std::mutex> g(s->shelf->mu);
        auto& v = s->shelf->blocks;
        for (size_t i = 0; i < v.size(); ++i) if (v[i].second == block) { *out = (char*)v[i].first; v.erase(v.begin() + (long)i); return hipSuccess; }
    }
    return dev_malloc((void**)out, block);
}
static void stash_give(q3_parked* p);
static q3_status park_launch(q3_session* s, std::vector<RowSeg>& segs, size_t max_bytes, const int* payload, int n_payload, std::vector<char>& up) {
    if (!s->park_desc) return set_err(Q3_UNSUPPORTED, "row state: needs the paged K/V cache");
    if ((int)segs.size() > PARK_MAX_SEGS || n_payload > PARK_PAYLOAD_INTS) return set_err(Q3_INVALID_ARG, "row state: descriptor table too small");
    up.assign((size_t)PARK_MAX_SEGS * sizeof(RowSeg) + PARK_PAYLOAD_INTS * 16, 0);
    memcpy(up.data(), segs.data(), segs.size() * sizeof(RowSeg));
    for (int i = 0; i < n_payload; ++i) memcpy(up.data() + (size_t)PARK_MAX_SEGS * sizeof(RowSeg) + (size_t)i * 16, &payload[i], 4);
    HIPC(hipMemcpyAsync(s->park_desc, up.data(), up.size(), hipMemcpyHostToDevice, s->stream));      // (`up` lives until the caller's synchronisation)
    HIPC(launch_row_move((const RowSeg*)s->park_desc, (int)segs.size(), max_bytes, s->stream));
    return Q3_OK;
}
static char* park_payload_dev(q3_session* s, int i) { return s->park_desc + (size_t)PARK_MAX_SEGS * sizeof(RowSeg) + (size_t)i * 16; }

extern "C" q3_status q3_session_park_row(q3_session* s, int b, q3_parked** out) {
    if (!s || !out) return set_err(Q3_INVALID_ARG, "q3_session_park_row: null argument");
    if (b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "q3_session_park_row: bad sequence index %d", b);
    if (!s->prefilled) return set_err(Q3_INVALID_ARG, "q3_session_park_row: session not prefilled");
    if (s->aql_failed) return set_err(Q3_HIP_ERROR, "session unusable: an earlier frame submission on the AQL queue failed or timed out");
    if (!s->paged) return set_err(Q3_UNSUPPORTED, "q3_session_park_row: needs the paged K/V cache (Q3_KV_CONTIGUOUS is set)");
    if (s->debug || s->profile) return set_err(Q3_UNSUPPORTED, "q3_session_park_row: not on debug / profiling sessions");
    if (s->kv_bf16 != s->kv_in_bf16) return set_err(Q3_UNSUPPORTED, "q3_session_park_row: the session's K/V conversion has not happened yet");
    if (s->seq[(size_t)b].idle) return set_err(Q3_INVALID_ARG, "q3_session_park_row: row %d is idle", b);
    if (s->seq[(size_t)b].stream_pos > 0)
        return set_err(Q3_UNSUPPORTED, "q3_session_park_row: row %d has delivered chunks (q3_session_next_chunk*): its stream position does not travel", b);
    q3_model* m = s->m; const q3_config& c = m->cfg;
    HIPC(hipSetDevice(m->device));
    HIPC(sync_frames(s));
    Q3C(session_refresh_codes(s));               // an opened row's committed count, every row's n_frames / done
    SeqInfo& q = s->seq[(size_t)b];
    std::unique_ptr<q3_parked> p(new q3_parked());
    p->session_uid = s->uid; p->B = s->B; p->max_frames = s->max_frames; p->H = c.hidden; p->V = c.codec_vocab;
    p->committed = session_row_committed(s, b); p->n_frames = q.n_frames; p->done = q.done;
    p->n_text_rows = q.trailing_len; p->has_ready = s->text_ready != nullptr; p->pages_bf16 = s->kv_in_bf16;
    size_t off = 0;
    auto part = [&](size_t bytes) { const size_t o = off; off += al16(bytes); return o; };
    p->o_lasth = part((size_t)p->H * 4); p->o_logits = part((size_t)p->V * 4); p->o_seen = part((size_t)p->V);
    p->o_u = part((size_t)(s->max_frames + 2) * 4); p->o_codes = part((size_t)p->committed * 64);
    p->o_text = part((size_t)p->n_text_rows * p->H * 4); p->o_pad = part((size_t)p->H * 4);
    p->o_scalars = part((size_t)16 * PS_SROW + sizeof(SampleRow));
    p->stash_bytes = off;
    // the vacated row's own page (below) and the stash: the two things that can be refused, before anything changes
    KvPool& pool = s->kv_in_bf16 ? m->kv_pool16 : m->kv_pool;
    std::vector<float*> own;
    if (kv_take(m, pool, 1, own) != hipSuccess)
        return set_err(Q3_KV_OVERFLOW, "q3_session_park_row: KV page pool exhausted: the vacated row needs one page of its own (budget: %ld of %ld half-pages in use)", m->kv_budget.used, m->kv_budget.limit);
    // (powers of two from 64 KB on, so that the blocks on the session's shelf fit the next record)
    size_t block = 65536; while (block < p->stash_bytes) block <<= 1;
    p->block = block; p->shelf = s->shelf;
    if (stash_take(s, block, &p->stash) != hipSuccess) { (void)hipGetLastError(); pool.give(own); return set_err(Q3_OOM, "q3_session_park_row: %zu bytes of row state refused by the device", p->stash_bytes); }
    std::vector<RowSeg> segs; size_t max_bytes = 0; std::vector<char> up;
    park_segments(s, b, *p, q.trail_base, q.pad_row, true, segs, &max_bytes);
    q3_status st = park_launch(s, segs, max_bytes, nullptr, 0, up);
    // The vacated row is left as session_idle_row leaves a row: frozen at the frames it has committed. A frozen row still runs
    // through every frame and rewrites the K/V of its frozen position — and every page it held has just left with the record: EVERY
    // entry of its table is repointed at one zero-filled page of its own (finite keys), which it holds like any idle row (one page
    // in the pool's figures and in the batcher's admission).
    const int frozen[2] = {p->committed, 0x7fffffff};
    std::vector<unsigned long long> ent((size_t)KV_MAX_PAGES, (unsigned long long)own[0]);
    hipError_t e = hipSuccess;
    if (st == Q3_OK) {
        e = hipMemcpyAsync(s->kv_table + (size_t)b * KV_MAX_PAGES, ent.data(), ent.size() * 8, hipMemcpyHostToDevice, s->stream);
        const size_t run_bytes = pool.run_floats * pool.elem_bytes, pitch = pool.layer_stride() * pool.elem_bytes;
        if (e == hipSuccess) e = hipMemset2DAsync(own[0], pitch, 0, run_bytes, (size_t)pool.n_layers, s->stream);
        if (e == hipSuccess) e = hipMemset2DAsync((char*)own[0] + pool.v_delta() * pool.elem_bytes, pitch, 0, run_bytes, (size_t)pool.n_layers, s->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s->limit + b, &frozen[0], 4, hipMemcpyHostToDevice, s->stream);      // (behind the launch that read it)
        if (e == hipSuccess && s->text_ready) e = hipMemcpyAsync(s->text_ready + b, &frozen[1], 4, hipMemcpyHostToDevice, s->stream);
    }
    const hipError_t es = sync_frames(s);
    if (st == Q3_OK && (e != hipSuccess || es != hipSuccess)) st = set_err(Q3_HIP_ERROR, "q3_session_park_row: %s", hipGetErrorString(e != hipSuccess ? e : es));
    if (st != Q3_OK) {
        // a device error, not a refusal: the table copy may have landed, so the page stays with the row (no entry may name a page
        // that is back in the pool); everything is drained, the block goes back
        s->kv_rows[(size_t)b].push_back(own[0]);
        stash_give(p.get());
        return st;
    }
    // host side: the codes so far, the page list and the SeqInfo leave with the record
    p->codes_host.assign(s->codes_host.begin() + (ptrdiff_t)((size_t)b * s->max_frames * 16), s->codes_host.begin() + (ptrdiff_t)(((size_t)b * s->max_frames + (size_t)p->committed) * 16));
    p->pages.assign(s->kv_rows[(size_t)b].begin(), s->kv_rows[(size_t)b].end());
    s->kv_rows[(size_t)b].assign(1, own[0]);
    p->seq = q; p->seq.req = p->seq.request();      // the request's arrays live in the record's own vectors
    q.opened = false; q.text_closed = true; q.ready = 0x7fffffff;      // the vacated row: a closed row frozen at its count
    q.limit = p->committed; q.start_run = s->frames_run - p->committed; q.committed = p->committed;
    q.idle = true; q.stream_pos = 0;
    s->codes_host_valid = false;
    p->m = m; m->refs.fetch_add(1);
    *out = p.release();
    return Q3_OK;
}

extern "C" q3_status q3_session_resume_row(q3_session* s, int b, q3_parked* p) {
    if (!s || !p) return set_err(Q3_INVALID_ARG, "q3_session_resume_row: null argument");
    if (b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "q3_session_resume_row: bad sequence index %d", b);
    if (p->session_uid != s->uid || p->m != s->m) return set_err(Q3_INVALID_ARG, "q3_session_resume_row: the record was parked by another session");
    if (s->aql_failed) return set_err(Q3_HIP_ERROR, "session unusable: an earlier frame submission on the AQL queue failed or timed out");
    q3_model* m = s->m;
    HIPC(hipSetDevice(m->device));
    HIPC(sync_frames(s));
    Q3C(session_refresh_codes(s));
    if (!s->seq[(size_t)b].idle && !s->seq[(size_t)b].done) return set_err(Q3_INVALID_ARG, "q3_session_resume_row: row %d is live (a record enters an idle row or one that has ended)", b);
    if (p->n_text_rows + 1 > s->row_cap) return set_err(Q3_UNSUPPORTED, "q3_session_resume_row: %d text rows exceed the row's slot (%d)", p->n_text_rows + 1, s->row_cap);
    // the row's text goes to ITS slot of the session's text rows, laid out as an open row's: trailing rows from the slot's first
    // row on (later text lands behind them), tts_pad in its last row
    const int row0 = s->repl_base + b * s->row_cap, pad_row = row0 + s->row_cap - 1;
    std::vector<RowSeg> segs; size_t max_bytes = 0; std::vector<char> up;
    park_segments(s, b, *p, row0, pad_row, false, segs, &max_bytes);
    const int payload[3] = {row0, pad_row, 0x7fffffff};
    if (!s->park_desc) return set_err(Q3_UNSUPPORTED, "q3_session_resume_row: needs the paged K/V cache");
    segs.push_back(RowSeg{park_payload_dev(s, 0), s->trail_base + b, 4, ROW_MOVE_COPY, 0});
    segs.push_back(RowSeg{park_payload_dev(s, 1), s->pad_row + b, 4, ROW_MOVE_COPY, 0});
    // The session got its open-text state AFTER this record was parked (the batcher enables it with the first open ticket): the row
    // the record enters may still carry the text_ready of an open row that ended unclosed, which would HOLD this row. A record
    // without the value is a closed row.
    if (!p->has_ready && s->text_ready) segs.push_back(RowSeg{park_payload_dev(s, 2), s->text_ready + b, 4, ROW_MOVE_COPY, 0});
    q3_status st = park_launch(s, segs, max_bytes, payload, 3, up);
    hipError_t e = hipSuccess;
    if (st == Q3_OK && !p->pages.empty())      // (entries behind the row's pages are written by kv_reserve_row before a frame reaches them)
        e = hipMemcpyAsync(s->kv_table + (size_t)b * KV_MAX_PAGES, p->pages.data(), p->pages.size() * 8, hipMemcpyHostToDevice, s->stream);
    const hipError_t es = sync_frames(s);
    if (st == Q3_OK && (e != hipSuccess || es != hipSuccess)) st = set_err(Q3_HIP_ERROR, "q3_session_resume_row: %s", hipGetErrorString(e != hipSuccess ? e : es));
    if (st != Q3_OK) return st;
    // nothing can fail from here on: the row's pages go back, the record's are linked, the record is consumed
    kv_release_row(s, b);
    s->kv_rows[(size_t)b].assign(p->pages.begin(), p->pages.end()); p->pages.clear();
    SeqInfo nq = p->seq;
    nq.row_base = row0; nq.trail_base = row0; nq.pad_row = pad_row;
    // every `frames_run - start_run` of the engine keeps meaning "frames this row has committed" (an opened row counts in `committed`)
    nq.start_run = s->frames_run - p->committed; nq.committed = p->committed;
    nq.idle = false; nq.stream_pos = 0;
    s->seq[(size_t)b] = nq; s->seq[(size_t)b].req = s->seq[(size_t)b].request();
    if (s->cstream) codec_stream_reset(s->cstream, b);
    if (s->ostage) pcm_stage_reset(s->ostage, b);
    s->codes_host_valid = false;
    stash_give(p);
    if (m->refs.fetch_sub(1) == 1) model_destroy(m);      // (never the last one here: the session holds its own)
    delete p;
    return Q3_OK;
}

static void stash_give(q3_parked* p) {
    if (!p->stash) return;
    bool kept = false;
    if (p->shelf) {
        std::lock_guard<std::mutex> g(p->shelf->mu);
        if (p->shelf->alive) { p->shelf->blocks.emplace_back(p->stash, p->block); kept = true; }
    }
    if (!kept) dev_free(p->stash);
    p->stash = nullptr;
}
extern "C" void q3_parked_free(q3_parked* p) {
    if (!p) return;
    q3_model* m = p->m;
    if (m) {
        (void)hipSetDevice(m->device);
        if (!p->pages.empty()) (p->pages_bf16 ? m->kv_pool16 : m->kv_pool).give(p->pages);
        stash_give(p);
    }
    delete p;
    if (m && m->refs.fetch_sub(1) == 1) model_destroy(m);      // the record outlived its session and the model handle
}

extern "C" q3_status q3_parked_info(const q3_parked* p, int* frames_committed, int* limit, int* done, int* kv_pages, size_t* state_bytes) {
    if (!p) return set_err(Q3_INVALID_ARG, "q3_parked_info: null record");
    if (frames_committed) *frames_committed = p->committed;
    if (limit) *limit = p->seq.limit;
    if (done) *done = p->done ? 1 : 0;
    if (kv_pages) *kv_pages = (int)p->pages.size();
    if (state_bytes) *state_bytes = p->stash_bytes;
    return Q3_OK;
}

// for the batcher (a parked ticket that is cancelled or read): the record's frames as q3_session_codes would report them
int parked_frames(const q3_parked* p, const uint32_t** codes) { if (codes) *codes = p->codes_host.data(); return p->n_frames; }
int parked_committed(const q3_parked* p) { return p->committed; }
int parked_pages(const q3_parked* p) { return (int)p->pages.size(); }
bool parked_done(const q3_parked* p) { return p->done; }
const SeqInfo& parked_seq(const q3_parked* p) { return p->seq; }
