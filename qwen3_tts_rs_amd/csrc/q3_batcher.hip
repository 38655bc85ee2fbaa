// q3_batcher.hip — continuous batching: q3_session_replace (side prefill + transplant) and the native batcher q3_batcher_*
// (one of the units of the engine: q3_engine.h says which holds what)
#include "q3_engine.h"
#include "q3_prefix_cache.h"
#include <condition_variable>
#include <deque>

// Continuous batching: swap a finished row of a running session for a new request (include/q3tts.h). The reference keeps all
// per-utterance state per call (KV caches, sampling context, penalty mask, trailing text: lib.rs:743-756, 1484-1541); here
// that state is the row's slice of the session's device arrays, so a swap = prefill the request in a one-row side session
// (the unchanged prefill path) and copy its slice in: K/V extents of the prompt positions, last hidden state, first sampled
// token, penalty mask, counters, the pre-drawn PCG stream, projected text rows. The captured frame graph is untouched — it
// only ever reads these arrays — and the other rows do not notice: their state, and therefore their bits, are unchanged.
// Row j of a prefilled side session becomes row b of the host session: the per-row state the captured frame graph reads is
// copied in, the prompt's K/V pages are relinked (contiguous extents: copied). Both streams are idle (the caller drained them).
q3_status transplant_row(q3_session* s, int b, q3_session* side, int j, int limit) {
    const q3_model* m = s->m; const q3_config& c = m->cfg;
    const SeqInfo& sq = side->seq[(size_t)j];
    const int H = c.hidden, S = sq.prefill_len, nkv = c.n_kv_heads;
    const size_t row_bytes = (size_t)HEAD_DIM * 4;
    if (s->paged) {
        // the prompt's K/V is not copied: the side session's pages become the row's (its old ones go back to the pool), and the
        // row's table entries are rewritten
        kv_release_row(s, b);
        std::vector<float*>& row = s->kv_rows[(size_t)b];
        row.assign(side->kv_rows[(size_t)j].begin(), side->kv_rows[(size_t)j].end());
        side->kv_rows[(size_t)j].clear();
        HIPC(hipMemcpyAsync(s->kv_table + (size_t)b * KV_MAX_PAGES, row.data(), row.size() * 8, hipMemcpyHostToDevice, s->stream));
    } else
    for (int l = 0; l < c.n_layers; ++l) {
        const size_t so = (size_t)l * side->kv_layer_stride + (size_t)j * nkv * side->max_seq * HEAD_DIM, dof = (size_t)l * s->kv_layer_stride + (size_t)b * nkv * s->max_seq * HEAD_DIM;
        HIPC(hipMemcpy2DAsync(s->kcache + dof, s->max_seq * row_bytes, side->kcache + so, side->max_seq * row_bytes, S * row_bytes, nkv, hipMemcpyDeviceToDevice, s->stream));
        HIPC(hipMemcpy2DAsync(s->vcache + dof, s->max_seq * row_bytes, side->vcache + so, side->max_seq * row_bytes, S * row_bytes, nkv, hipMemcpyDeviceToDevice, s->stream));
    }
    auto d2d = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s->stream); };
    HIPC(d2d(s->LASTH + (size_t)b * H, side->LASTH + (size_t)j * H, (size_t)H * 4));
    // the row's first logits (Q3_GET_LOGITS after the prefill; the next frame overwrites every row's)
    HIPC(d2d(s->LOGITS + (size_t)b * c.codec_vocab, side->LOGITS + (size_t)j * c.codec_vocab, (size_t)c.codec_vocab * 4));
    // a one-length session that prefilled its rows in groups (prefix cache): its own prompt embeddings were never assembled
    if (s->regrouped && S == s->prefill_len)
        HIPC(d2d(s->embeds + (size_t)b * S * H, side->embeds + (size_t)j * S * H, (size_t)S * H * 4));
    HIPC(d2d(s->tok + b, side->tok + j, 4));
    HIPC(d2d(s->seen + (size_t)b * c.codec_vocab, side->seen + (size_t)j * c.codec_vocab, (size_t)c.codec_vocab));
    HIPC(d2d(s->token_count + b, side->token_count + j, 4));
    HIPC(d2d(s->pos + b, side->pos + j, 4));
    HIPC(d2d(s->frame_idx + b, side->frame_idx + j, 4));
    // the row's pre-drawn PCG stream: the side session drew max_frames(side) + 1 >= limit + 1 of them (an ICL cap may make it the shorter one)
    HIPC(d2d(s->U + (size_t)b * (s->max_frames + 2), side->U + (size_t)j * (side->max_frames + 2),
             (size_t)((side->max_frames < s->max_frames ? side->max_frames : s->max_frames) + 2) * 4));
    const int row0 = s->repl_base + b * s->row_cap;
    int hv[4] = {row0 + (sq.trail_base - sq.row_base), sq.trailing_len, row0 + (sq.pad_row - sq.row_base), limit};
    if (sq.opened) {
        // An open row (q3_batcher_submit_open) keeps the layout q3_session_open_text gives it: its trailing rows from the first row
        // of the slot on, so that later text (session_append_many) lands behind them; the one prompt row the frames still read,
        // tts_pad, goes to the slot's last row. Nothing else of the prompt's rows is read after the prefill.
        if (!s->text_ready) return set_err(Q3_INVALID_ARG, "transplant_row: an open row needs the session's hold path (session_text_enable)");
        hv[0] = row0; hv[2] = row0 + s->row_cap - 1;
        if (sq.trailing_len > 0) HIPC(d2d(s->rows + (size_t)row0 * H, side->rows + (size_t)sq.trail_base * H, (size_t)sq.trailing_len * H * 4));
        HIPC(d2d(s->rows + (size_t)hv[2] * H, side->rows + (size_t)sq.pad_row * H, (size_t)H * 4));
    } else
        HIPC(d2d(s->rows + (size_t)row0 * H, side->rows + (size_t)sq.row_base * H, (size_t)sq.n_rows * H * 4));
    HIPC(hipMemcpyAsync(s->trail_base + b, &hv[0], 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->trail_len + b, &hv[1], 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->pad_row + b, &hv[2], 4, hipMemcpyHostToDevice, s->stream));
    HIPC(hipMemcpyAsync(s->limit + b, &hv[3], 4, hipMemcpyHostToDevice, s->stream));
    // frames the row's text allows: everything for a closed request (also in a row that was open before), the side row's own
    // count for an open one
    const int ready = sq.opened ? sq.ready : 0x7fffffff;
    if (s->text_ready) HIPC(hipMemcpyAsync(s->text_ready + b, &ready, 4, hipMemcpyHostToDevice, s->stream));
    const SampleRow srow = sample_row(sq.req.opts);
    HIPC(hipMemcpyAsync(s->sample_rows + b, &srow, sizeof srow, hipMemcpyHostToDevice, s->stream));
    HIPC(sync_frames(s));
    SeqInfo nq = sq;
    nq.row_base = row0; nq.trail_base = hv[0]; nq.pad_row = hv[2];
    nq.start_run = s->frames_run; nq.limit = limit; nq.n_frames = 0; nq.done = false; nq.stream_pos = 0; nq.req.opts.max_length = limit; nq.idle = false;
    // (opened, text_closed, text_all, n_trail, ready came along with sq) an open ICL row resolves its length cap against the
    // request's own max_length when its text closes (open_counts): the side session was created with the session's frame budget
    if (sq.opened) { nq.committed = 0; nq.max_length_req = limit; }
    s->seq[(size_t)b] = nq;
    s->seq[(size_t)b].req = s->seq[(size_t)b].request();      // the request's arrays live in the row's own vectors (the caller's pointers need not outlive the call)
    if (s->cstream) codec_stream_reset(s->cstream, b);      // q3_session_next_chunks: the row's vocoder state belonged to the old utterance
    if (s->ostage) pcm_stage_reset(s->ostage, b);           // q3_session_next_chunks_out: so did its output row's
    s->codes_host_valid = false;
    return Q3_OK;
}
// what a side session must satisfy before its rows may enter the host session
static q3_status transplant_check(q3_session* s, q3_session* side, int j, int limit_req, int* limit_out) {
    const SeqInfo& sq = side->seq[(size_t)j];
    if (side->opts.chunk_frames != s->opts.chunk_frames) return set_err(Q3_UNSUPPORTED, "q3_session_replace: chunk_frames is a property of the session");
    const int limit = limit_req < sq.limit ? limit_req : sq.limit;
    if (sq.n_rows > s->row_cap) return set_err(Q3_UNSUPPORTED, "q3_session_replace: the request's %d text rows exceed the session's slot (%d rows: 1024, or the longest text of the original batch)", sq.n_rows, s->row_cap);
    if (sq.opened && sq.trailing_len + 1 > s->row_cap - 1) return set_err(Q3_UNSUPPORTED, "q3_session_replace: the open request's %d trailing text rows exceed the session's slot (%d rows)", sq.trailing_len + 1, s->row_cap - 1);
    if (s->paged != side->paged) return set_err(Q3_UNSUPPORTED, "q3_session_replace: the sessions disagree on KV paging");
    if (s->kv_bf16 != s->kv_in_bf16) return set_err(Q3_UNSUPPORTED, "q3_session_replace: the session's K/V conversion has not happened yet");
    // max_seq bounds a row in both layouts: the captured frame was specialised for it (key splits, the page-table form of the
    // attention kernel); with pages it reserves nothing — only the pages a row really reaches are taken from the pool
    if (sq.prefill_len + limit + 1 > s->max_seq) return set_err(Q3_KV_OVERFLOW, "q3_session_replace: prompt of %d positions + %d frames exceeds the row's KV extent (%d)", sq.prefill_len, limit, s->max_seq);
    *limit_out = limit;
    return Q3_OK;
}

// The one side prefill (q3_engine.h): q3_session_replace, the batcher's stage worker and the groups of a ragged first batch.
q3_status side_prefill(q3_session* host, const q3_request* reqs, const int* limit_req, int n, bool open_text, bool closed,
                       bool prefix_common, hipStream_t borrow, std::unique_ptr<q3_session>* side_out, int* limit_out,
                       const std::function<void()>& created, bool staged_only) {
    std::vector<q3_request> rq(reqs, reqs + n);
    for (q3_request& r : rq) r.opts.max_length = host->max_frames;      // the side session draws the rows' PCG streams with the host session's stride
    q3_session* side_raw = nullptr;
    // (an open request: with the host's frame budget — an ICL row's length cap, which would size the side session, is not known yet)
    Q3C(session_create(host->m, rq.data(), n, open_text ? host->max_frames : 0, 0, &side_raw, borrow));
    std::unique_ptr<q3_session> side(side_raw);
    side->kv_bf16 = host->kv_bf16;                      // the side session prefills in f32 and converts, as the host session did
    side->prefix_common = prefix_common;
    if (open_text) Q3C(q3_session_open_text(side.get(), 0));       // the one request is taken with its text open
    if (open_text && closed) Q3C(q3_session_append_text(side.get(), 0, nullptr, 0, 1));      // ... and closed again: the close came before the prefill
    if (created) created();
    // (sampling options are per row — SampleRow —, resolved by the side session: an ICL request's repetition-penalty floor and
    // length cap, lib.rs:913-929, come along)
    for (int j = 0; j < n; ++j) Q3C(transplant_check(host, side.get(), j, limit_req[j], &limit_out[j]));
    if (!staged_only) Q3C(q3_session_prefill(side.get()));                // ends with a synchronisation of the side stream
    *side_out = std::move(side);
    return Q3_OK;
}
static q3_status session_replace(q3_session* s, int b, const q3_request* req, bool open_text, bool closed);
extern "C" q3_status q3_session_replace(q3_session* s, int b, const q3_request* req) { return session_replace(s, b, req, false, false); }
// open_text: the batcher's open tickets (the public call installs a closed request)
static q3_status session_replace(q3_session* s, int b, const q3_request* req, bool open_text, bool closed) {
    if (!s || !req || b < 0 || b >= s->B) return set_err(Q3_INVALID_ARG, "q3_session_replace: bad argument");
    if (!s->prefilled) return set_err(Q3_INVALID_ARG, "q3_session_replace: session not prefilled");
    if (s->debug || s->profile) return set_err(Q3_UNSUPPORTED, "q3_session_replace: not on debug / profiling sessions");
    const q3_model* m = s->m;
    HIPC(hipSetDevice(m->device));
    const int limit_req = req->opts.max_length;
    if (limit_req < 1 || limit_req > s->max_frames) return set_err(Q3_UNSUPPORTED, "q3_session_replace: max_length %d outside 1..%d (the session's frame budget)", limit_req, s->max_frames);
    static const bool timing = getenv("Q3_REPLACE_TIMING") != nullptr;      // development aid: where a swap's milliseconds go
    const auto tp0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (timing) fprintf(stderr, "[q3 replace] %-8s %.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count());
    };
    std::unique_ptr<q3_session> side; int limit = 0;
    // on the host's stream: its frames and this prefill are serial anyway
    Q3C(side_prefill(s, req, &limit_req, 1, open_text, closed, false, s->stream, &side, &limit, [&] { lap("create"); }));
    lap("prefill");
    HIPC(sync_frames(s));             // no frame of the host session in flight while its row changes
    Q3C(transplant_row(s, b, side.get(), 0, limit));
    lap("copies");
    side.reset();
    lap("free");
    return Q3_OK;
}

// ------------------------------------------------------------------------------------------------
// Continuous batcher: a queue of requests through the rows of ONE session (the native form of what a serving loop does
// with q3_session_replace). No thread of its own: the host calls q3_batcher_step from its loop — submit / step / poll /
// fetch may interleave freely (one thread at a time). A step fills free rows from the queue (one-row side prefill + state
// copy, rows of any prompt kind), runs up to n_frames frames of the shared frame graph, and collects the rows that ended
// (codes, and the PCM if the request asked for it). Every request gets the bits of its own batch-1 run.
// ------------------------------------------------------------------------------------------------
struct BatTicket {
    BatReq req; int state = Q3_TICKET_QUEUED; int row = -1; bool want_pcm = false;
    std::vector<uint32_t> codes; std::vector<float> pcm; int n_frames = 0;
    q3_status st = Q3_OK; std::string err;
    // vocoded by the batcher's decode worker (below): queued / running there until dec_done; the row it ran in is long refilled
    bool decoding = false; std::atomic<bool> dec_done{false}; q3_status dec_st = Q3_OK; std::string dec_err;
    // A streamed ticket (q3_batcher_submit_streamed): its frames go to the worker step by step (StreamPart), its samples land in
    // spcm and leave through q3_batcher_read. The host thread owns streamed / s_pushed / s_ended; the worker owns s_all / s_deliv;
    // s_pending, spcm, s_read, s_failed, s_st and s_err are shared under the worker's mutex.
    bool streamed = false, s_started = false, s_ended = false; int s_pushed = 0;          // frames handed to the worker so far; the row has been collected
    int s_pending = 0; std::vector<float> spcm; size_t s_read = 0;     // parts queued or running; landed samples; samples read
    bool s_failed = false; q3_status s_st = Q3_OK; std::string s_err;
    std::vector<uint32_t> s_all; int s_deliv = 0;                      // reference | generated frames seen so far; frames whose samples landed
    // An open ticket (q3_batcher_submit_open): text_all = every token received so far (q3_batcher_append_text only records), closed =
    // the host has closed the text. n_taken / close_taken = what the ticket's row — or the side session that is being prefilled
    // for it — already holds; the rest goes in with the next flush of q3_batcher_step. Host thread only.
    bool open = false, closed = false, close_taken = false; std::vector<uint32_t> text_all; size_t n_taken = 0;
    bool cancelled = false;                             // q3_batcher_cancel took its row (or its place in the queue)
    // A streamed ticket's own output (q3_batcher_ticket_*; host thread, fixed before the step that follows `born`). Other than
    // out.plain(), its samples go through the worker's output stage and land, as bytes of that format, in sout (under the worker's
    // mutex, like spcm, which stays empty) and leave through q3_batcher_read_out alone. lo_* / si: the readings of its loudness
    // and silence steps after the parts that have landed (under the worker's mutex; until then: out_*_at_rest)
    long born = 0; OutSettings out;
    float lo_M = 0.0f, lo_gain = 1.0f; int lo_blocks = 0, lo_gated = 0; int64_t si[5] = {0, 0, 0, 0, 0};
    std::vector<char> sout; size_t o_read = 0;
    // Parking (q3_batcher_set_parking; host thread). rec: the ticket's row as a record while it reads PARKED; want_in: it
    // wants a row again (parked by the scheduler, or q3_batcher_unpark) — it stands in the waiting list once a frame is runnable;
    // units: its admission claim, which it keeps while parked; entered: frames it had committed when it entered its row (the time
    // slice counts from there); last_row: the row it left; srow: its row of the worker's codec stream and output stage when
    // parking is on (the stream row follows the ticket, not the slot), -1 = none
    q3_parked* rec = nullptr; bool want_in = false, in_queue = false; long units = 0; int entered = 0, last_row = -1, srow = -1;
};
// frames [f0, f0 + n) of a streamed ticket for the stream row of its slot: `first` resets the row (and primes it with the ticket's
// reference frames), `last` gives the row's blocks back once the samples have landed
struct StreamPart { BatTicket* t; int row; std::vector<uint32_t> frames; bool first, last; };      // (row: of the worker's stream — the slot, or the ticket's own row with parking on)
struct DecJob { BatTicket* whole = nullptr; std::vector<StreamPart> parts; };      // a whole-ticket decode OR one step's stream parts
struct q3_batcher {
    q3_model* m = nullptr; int slots = 0, frame_budget = 0, prompt_budget = 0, chunk_frames = 0;
    q3_session* s = nullptr;
    std::vector<int64_t> owner;                       // ticket running in each row, -1 = free
    std::vector<long> commit;                         // KvBudget units row r may still come to hold (worst case of its request), 0 = free row
    std::vector<int64_t> queue;                       // the ONE waiting list: fresh tickets (QUEUED) and parked ones that want a row again (PARKED)
    // Parking (q3_batcher_set_parking): off with max_parked = 0 — nothing below is then touched and every entry point behaves as before
    int max_parked = 0, quantum = 0; bool fresh_first = false;
    std::vector<int64_t> parked;                      // tickets that hold a record, in park order
    long long n_parks = 0, n_resumes = 0, n_moved = 0;
    std::vector<int> srow_free;                       // free rows of the worker's stream / stage (slots + max_parked of them), highest first
    int stream_rows() const { return slots + max_parked; }
    std::unordered_map<int64_t, std::unique_ptr<BatTicket>> t;
    int64_t next_id = 1;
    // Round 6: the head of the queue is prefilled AHEAD of the row it will enter. A worker thread opens its one-row side session
    // and runs the (unchanged) prefill on a stream of its own while the captured frame keeps replaying for the live rows — the
    // frame leaves most of the chip idle —; when a row ends, the swap is only the state copy (transplant_row) at that frame
    // boundary. The other rows used to stand still for the whole side prefill (1.9 ms for a short prompt, 45 ms for a 4k-token
    // one). Bits are unchanged: the same kernels on the same inputs, only on another stream. Off under a page limit
    // (q3_model_kv_pool_limit: admission must see a row's pages when it decides) and with Q3_BAT_NO_STAGE=1 (A/B aid).
    struct Stage {
        int64_t id = -1; std::thread thr; q3_session* side = nullptr; q3_status st = Q3_OK; std::string err; int limit = 0;
    } stage;
    std::unique_ptr<struct BatDecoder> dec;           // the decode worker of finished rows (below)
    // streamed tickets: the parts of the step in progress (one job at its end), the stream's shape (environment, read at create)
    std::vector<StreamPart> sparts; int n_streamed = 0;
    int s_block_frames = 128, s_max_blocks = 0;
    long steps = 0;                                   // q3_batcher_step calls so far (q3_batcher_ticket_output: before the ticket's first)
    bool want_text = false;                           // an open ticket was submitted: the session runs the frame with the hold kernels
    // Q3_BAT_TEXT_STATS=1 (development aid): what the text flushes did, printed when the batcher is freed
    long tx_flushes = 0, tx_tokens = 0, tx_steps = 0; double tx_ms = 0;
};
// Round 6: a finished row's vocoder no longer stalls the session either. bat_collect used to decode the row's samples on the session's
// own stream before the row could be refilled — every live row stood still for ~20 ms per 640 frames. The codes are on the host
// by then, so the decode goes to a worker thread with its own stream and workspace (one decode at a time, in order), the row is
// idled and refilled at once, and the ticket counts as RUNNING until its samples have landed (poll; fetch waits for them). Same
// kernels on the same codes as q3_session_decode: the same samples. ICL rows (reference frames prepended and cut, lib.rs:1022-1041)
// and Q3_BAT_SYNC_DECODE=1 keep the synchronous decode.
// Streamed tickets use the same worker, stream and queue: at the end of a step its frames are on the host and go in as ONE job
// that covers every streamed row; the worker pushes them through a block-allocated codec stream (q3_codec_stream.hip, one stream
// row per slot) and the samples land in the tickets' buffers. Jobs run in order, so the last part of a slot's previous owner
// precedes the first part of its next one.
struct BatDecoder {
    std::thread thr; std::mutex mu; std::condition_variable cv, cv_done; std::deque<DecJob> q; bool stop = false;
    hipStream_t stream = nullptr; CodecWS ws;
    q3_codec_stream* cs = nullptr;                    // the streamed tickets' vocoder state (created by the first stream job)
    q3_pcm_stage* ps = nullptr;                       // their output stage, one row per slot (created by the first part of a ticket with an output of its own)
    int info_bf = 0, info_total = 0, info_use = 0, info_peak = 0; size_t info_bytes = 0;      // its figures after the last job (under mu)
    // Q3_BAT_STREAM_STATS=1 (development aid): what the worker did, printed when the batcher is freed
    long st_jobs = 0, st_pushes = 0, st_frames = 0, st_depth_sum = 0; int st_depth_max = 0; double st_busy_ms = 0;
};
static void decoder_main(q3_batcher* b);
static void decoder_enqueue(q3_batcher* b, DecJob&& j) {
    BatDecoder& d = *b->dec;
    std::lock_guard<std::mutex> g(d.mu);
    if (!d.thr.joinable()) d.thr = std::thread(decoder_main, b);
    for (StreamPart& p : j.parts) p.t->s_pending++;
    d.q.push_back(std::move(j));
    d.st_depth_sum += (long)d.q.size(); if ((int)d.q.size() > d.st_depth_max) d.st_depth_max = (int)d.q.size();
    d.cv.notify_one();
}
static void decoder_push(q3_batcher* b, BatTicket* t) { DecJob j; j.whole = t; decoder_enqueue(b, std::move(j)); }
// the parts gathered since the last flush become one job; the step does not wait for it
static void stream_flush(q3_batcher* b) {
    if (b->sparts.empty()) return;
    DecJob j; j.parts = std::move(b->sparts); b->sparts.clear();
    decoder_enqueue(b, std::move(j));
}
// a collected streamed ticket whose parts have all been served is DONE (or FAILED with the worker's reason)
static void stream_settle(q3_batcher* b, BatTicket& t, bool wait) {
    if (!t.streamed) return;
    stream_flush(b);
    BatDecoder& d = *b->dec;
    std::unique_lock<std::mutex> lk(d.mu);
    if (wait) d.cv_done.wait(lk, [&] { return t.s_pending == 0; });
    if (t.state != Q3_TICKET_RUNNING || t.row >= 0) return;
    if (t.s_failed) { t.state = Q3_TICKET_FAILED; t.st = t.s_st; t.err = t.s_err; }
    else if (t.s_ended && t.s_pending == 0) t.state = t.cancelled ? Q3_TICKET_CANCELLED : Q3_TICKET_DONE;
}
static void ticket_wait_decode(q3_batcher* b, BatTicket& t) {
    if (!t.decoding) return;
    BatDecoder& d = *b->dec;
    {
        std::unique_lock<std::mutex> lk(d.mu);
        d.cv_done.wait(lk, [&] { return t.dec_done.load(); });
    }
    t.decoding = false;
    if (t.dec_st != Q3_OK) { t.state = Q3_TICKET_FAILED; t.st = t.dec_st; t.err = t.dec_err; t.pcm.clear(); }
    else t.state = t.cancelled ? Q3_TICKET_CANCELLED : Q3_TICKET_DONE;
}
static void decoder_stop(q3_batcher* b) {
    BatDecoder& d = *b->dec;
    {
        std::lock_guard<std::mutex> g(d.mu);
        d.stop = true; d.cv.notify_all();
    }
    if (d.thr.joinable()) d.thr.join();
    if (d.st_jobs > 0 && getenv("Q3_BAT_STREAM_STATS"))
        fprintf(stderr, "[q3 batcher stream] %ld stream jobs (one per step), %ld pushes, %ld frames through the front, worker busy %.1f ms (%.2f ms per job), "
                        "queue depth at enqueue: max %d\n", d.st_jobs, d.st_pushes, d.st_frames, d.st_busy_ms, d.st_busy_ms / d.st_jobs, d.st_depth_max);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    if (d.cs) { q3_codec_stream_free(d.cs); d.cs = nullptr; }
    if (d.ps) { q3_pcm_stage_free(d.ps); d.ps = nullptr; }
    if (d.stream) { (void)hipStreamDestroy(d.stream); d.stream = nullptr; }
    d.ws.release();
}
static q3_status decoder_run(q3_batcher* b, BatTicket& t) {
    BatDecoder& d = *b->dec;
    const q3_model* m = b->m;
    HIPC(hipSetDevice(m->device));
    if (!d.stream) HIPC(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    VocodePcm pcm;
    Q3C(vocode_enqueue(m, d.ws, d.stream, VocodeSrc{nullptr, 0, t.codes.data(), true}, 0, t.n_frames, 0, 0, &pcm));
    Q3C(vocode_copy_out(pcm, t.pcm.data(), t.pcm.size(), nullptr, d.stream));
    HIPC(hipStreamSynchronize(d.stream));
    return Q3_OK;
}
// One step's parts of the streamed tickets. Parts are pushed together, a row at most once per push (a slot whose owner changed
// inside the step has two parts: the push is cut there). A row's push starts at the stream row's position: normally the part's
// own frames; after a failed push put the row back to frame 0, everything from the ticket's first (reference) frame, with `skip`
// set to what was already delivered — no sample is lost or repeated. A joint push that is refused or fails is repeated row by
// row, and the tickets whose own push fails are FAILED with its message.
// A ticket with an output of its own (not out.plain()): its first part sets — and so restarts — the slot's row of the worker's output stage,
// its pushes carry that row, its last part flushes it. The stage follows the samples that were DELIVERED: the put-back above resets
// the codec stream's row, never the stage's, so the ticket's listener hears neither a gap nor a repeat.
static void decoder_stream_job(q3_batcher* b, std::vector<StreamPart>& parts) {
    BatDecoder& d = *b->dec;
    const auto t_job = std::chrono::steady_clock::now();
    const q3_model* m = b->m;
    const int spf = samples_per_frame(m->cfg);
    q3_status st0 = hipSetDevice(m->device) == hipSuccess ? Q3_OK : set_err(Q3_HIP_ERROR, "hipSetDevice");
    if (st0 == Q3_OK && !d.stream && hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess) st0 = set_err(Q3_HIP_ERROR, "hipStreamCreateWithFlags");
    if (st0 == Q3_OK && !d.cs)
        st0 = codec_stream_create(b->m, b->stream_rows(), b->frame_budget + b->prompt_budget, d.stream, &d.cs, b->s_block_frames, b->s_max_blocks);
    auto fail = [&](BatTicket& t, q3_status st, const char* msg) {
        std::lock_guard<std::mutex> g(d.mu);
        if (!t.s_failed) { t.s_failed = true; t.s_st = st; t.s_err = msg; }
    };
    struct Out { StreamPart* p; int n_new; std::vector<float> pcm; std::vector<char> out; size_t n_out = 0; };
    auto flush_only = [&](const Out& o) { return o.n_new <= 0 && !o.p->t->out.plain() && o.p->last; };
    auto is_failed = [&](BatTicket& t) { std::lock_guard<std::mutex> g(d.mu); return t.s_failed; };
    // the samples of a served part land; a failed ticket's row and a finished one's give their blocks back
    auto land = [&](Out& o) {
        BatTicket& t = *o.p->t;
        t.s_deliv += o.n_new;
        float lm = 0.0f, lg = 1.0f; int lb = 0, lc = 0;
        const bool loud = t.out.loud != Q3_LOUD_OFF && q3_pcm_stage_loudness(d.ps, o.p->row, &lm, &lg, &lb, &lc) == Q3_OK;
        int64_t si[5] = {0, 0, 0, 0, 0};
        const bool sil = t.out.sil_mB != 0 && q3_pcm_stage_silence(d.ps, o.p->row, &si[0], &si[1], &si[2], &si[3], &si[4]) == Q3_OK;
        std::lock_guard<std::mutex> g(d.mu);
        if (loud) { t.lo_M = lm; t.lo_gain = lg; t.lo_blocks = lb; t.lo_gated = lc; }
        if (sil) memcpy(t.si, si, sizeof(si));
        if (!t.out.plain()) t.sout.insert(t.sout.end(), o.out.begin(), o.out.begin() + (long)(o.n_out * t.out.sample_bytes()));
        else t.spcm.insert(t.spcm.end(), o.pcm.begin(), o.pcm.end());
    };
    size_t i = 0;
    while (i < parts.size()) {
        // the next group: parts up to the first repeated row
        std::vector<Out> grp; std::vector<char> seen((size_t)b->stream_rows(), 0);
        for (; i < parts.size() && !seen[(size_t)parts[i].row]; ++i) {
            StreamPart& p = parts[i]; BatTicket& t = *p.t;
            seen[(size_t)p.row] = 1;
            if (st0 != Q3_OK) { fail(t, st0, q3_last_error()); continue; }
            if (p.first) { codec_stream_reset(d.cs, p.row); t.s_all = t.req.ref_codes; t.s_deliv = 0; }
            if (p.first && !t.out.plain()) {
                q3_status so = Q3_OK;
                if (!d.ps) so = q3_pcm_stage_create(m->device, b->stream_rows(), (size_t)std::min(b->frame_budget + b->prompt_budget, 100000) * spf, &d.ps);
                if (so == Q3_OK) so = pcm_stage_apply(d.ps, p.row, "q3_batcher_step", t.out);      // (whatever the row's last ticket had)
                if (so != Q3_OK) fail(t, so, q3_last_error());
            }
            if (is_failed(t)) continue;
            t.s_all.insert(t.s_all.end(), p.frames.begin(), p.frames.end());
            grp.push_back({&p, (int)(p.frames.size() / 16), {}});
        }
        auto push_of = [&](Out& o) {
            BatTicket& t = *o.p->t;
            const int n_ref = (int)(t.req.ref_codes.size() / 16), sp = codec_stream_pos(d.cs, o.p->row);
            if (t.out.plain()) {
                o.pcm.resize((size_t)o.n_new * spf);
                return CsPush{o.p->row, n_ref + t.s_deliv + o.n_new - sp, n_ref + t.s_deliv - sp, t.s_all.data() + (size_t)sp * 16, nullptr, o.pcm.data()};
            }
            o.out.resize(pcm_stage_count(d.ps, o.p->row, (size_t)o.n_new * spf, o.p->last) * t.out.sample_bytes());
            CsPush p{o.p->row, 0, 0, nullptr, nullptr, nullptr};      // (no new frames: only the stage row's tail)
            if (o.n_new > 0) { p.n = n_ref + t.s_deliv + o.n_new - sp; p.skip = n_ref + t.s_deliv - sp; p.host = t.s_all.data() + (size_t)sp * 16; }
            p.ps = d.ps; p.ps_row = o.p->row; p.last = o.p->last; p.out_host = o.out.data(); p.n_out = &o.n_out;
            return p;
        };
        std::vector<CsPush> P;
        for (Out& o : grp) if (o.n_new > 0 || flush_only(o)) P.push_back(push_of(o));
        bool joint_ok = true;
        if (!P.empty()) { joint_ok = codec_stream_push(d.cs, P) == Q3_OK; d.st_pushes++; for (const CsPush& p : P) d.st_frames += p.n; }
        // A refused joint push (Q3_OOM under max_blocks) is repeated row by row, the rows that need no new block first and then the
        // others by the blocks they already hold, fewest first: under a block limit the ticket that fails is the one whose row
        // holds the most — a long ticket does not starve a short one that arrived after it took the last free block.
        if (!joint_ok)
            std::stable_sort(grp.begin(), grp.end(), [&](const Out& x, const Out& y) {
                auto key = [&](const Out& o) {
                    if (o.n_new <= 0) return std::make_pair(0, 0);
                    int held = 0, need = 0;
                    codec_stream_blocks(d.cs, o.p->row, (int)(o.p->t->req.ref_codes.size() / 16) + o.p->t->s_deliv + o.n_new, &held, &need);
                    return std::make_pair(need > 0 ? 1 : 0, need > 0 ? held : 0);
                };
                return key(x) < key(y);
            });
        for (Out& o : grp) {
            BatTicket& t = *o.p->t;
            if (!joint_ok && (o.n_new > 0 || flush_only(o))) {            // alone: this row's own push decides about this ticket
                const q3_status st = codec_stream_push(d.cs, {push_of(o)});
                if (st != Q3_OK) { fail(t, st, q3_last_error()); codec_stream_reset(d.cs, o.p->row); continue; }
            }
            land(o);
            if (o.p->last) codec_stream_reset(d.cs, o.p->row);
        }
    }
    int bf = 0, tot = 0, use = 0, peak = 0; size_t bytes = 0;
    if (d.cs) (void)q3_codec_stream_info(d.cs, &bf, &bytes, &tot, &use, &peak);
    {
        std::lock_guard<std::mutex> g(d.mu);
        d.info_bf = bf; d.info_bytes = bytes; d.info_total = tot; d.info_use = use; d.info_peak = peak;
        for (StreamPart& p : parts) p.t->s_pending--;
        d.st_jobs++; d.st_busy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_job).count();
    }
    d.cv_done.notify_all();
}
static void decoder_main(q3_batcher* b) {
    BatDecoder& d = *b->dec;
    for (;;) {
        DecJob job;
        {
            std::unique_lock<std::mutex> lk(d.mu);
            d.cv.wait(lk, [&] { return d.stop || !d.q.empty(); });
            if (d.q.empty()) return;                 // stop, and nothing left to decode
            job = std::move(d.q.front()); d.q.pop_front();
        }
        if (!job.whole) { decoder_stream_job(b, job.parts); continue; }
        BatTicket* t = job.whole;
        const q3_status st = decoder_run(b, *t);
        t->dec_st = st;
        if (st != Q3_OK) t->dec_err = q3_last_error();
        {
            std::lock_guard<std::mutex> g(d.mu);
            t->dec_done.store(true);
        }
        d.cv_done.notify_all();
    }
}
static void stage_join(q3_batcher* b) { if (b->stage.thr.joinable()) b->stage.thr.join(); }
static void stage_drop(q3_batcher* b) {
    stage_join(b);
    if (b->stage.side) { q3_session_free(b->stage.side); b->stage.side = nullptr; }
    b->stage.id = -1; b->stage.st = Q3_OK; b->stage.err.clear();
}

// a row that has nothing to do: frozen on the device from its current frame on (rows of a freshly opened session that no
// request occupies yet)
static q3_status session_idle_row(q3_session* s, int b) {
    SeqInfo& q = s->seq[b];
    int ran = q.opened ? q.committed : s->frames_run - q.start_run;      // (a held row replayed frames it did not commit)
    if (ran < 0) ran = 0; if (ran > q.limit) ran = q.limit;
    q.limit = ran;
    HIPC(sync_frames(s));          // no frame in flight while the row's limit and pages change
    HIPC(q3_hipMemcpy(s->limit + b, &q.limit, sizeof(int), hipMemcpyHostToDevice));
    // A frozen row still runs through every frame (its results are dropped): it reads its keys and rewrites the K/V of its
    // frozen position, prefill_len + ran. It keeps the ONE page that position lies in and every table entry it can reach points
    // there, zero-filled (below); the other pages go back to the pool, and the row takes no
    // more (kv_reserve_frames skips it) — a finished row must not sit on pages the queue is waiting for.
    if (s->paged && !q.idle && !s->kv_rows[(size_t)b].empty()) {
        std::vector<float*>& row = s->kv_rows[(size_t)b];
        size_t keep = (size_t)(q.prefill_len + ran) / KV_PAGE_POS; if (keep >= row.size()) keep = row.size() - 1;
        float* kept = row[keep];
        std::vector<float*> back;
        for (size_t i = 0; i < row.size(); ++i) if (i != keep) back.push_back(row[i]);
        if (!back.empty()) (s->kv_in_bf16 ? s->m->kv_pool16 : s->m->kv_pool).give(back);
        row.assign(1, kept);
        // EVERY entry of the row's table names the kept page (none keeps the address of a page that went back to the pool), and the
        // page is zero-filled: the frozen row goes on reading positions 0 .. pos through it, i.e. also slots this row never wrote
        // (a previous owner's bits, possibly NaN / Inf, which would then run through the sampler and the embedding gather of a row
        // nobody reads); zeros are finite keys. One strided memset per K and V: n_layers runs of nkv * KV_PAGE_POS * HEAD_DIM elements.
        std::vector<unsigned long long> ent((size_t)KV_MAX_PAGES, (unsigned long long)kept);
        HIPC(q3_hipMemcpy(s->kv_table + (size_t)b * KV_MAX_PAGES, ent.data(), ent.size() * 8, hipMemcpyHostToDevice));
        const KvPool& pool = s->kv_in_bf16 ? s->m->kv_pool16 : s->m->kv_pool;
        const size_t run_bytes = pool.run_floats * pool.elem_bytes, pitch = pool.layer_stride() * pool.elem_bytes;
        HIPC(hipMemset2DAsync(kept, pitch, 0, run_bytes, (size_t)pool.n_layers, s->stream));
        HIPC(hipMemset2DAsync((char*)kept + pool.v_delta() * pool.elem_bytes, pitch, 0, run_bytes, (size_t)pool.n_layers, s->stream));
        HIPC(hipStreamSynchronize(s->stream));
    }
    q.idle = true;
    s->codes_host_valid = false;
    return Q3_OK;
}

extern "C" q3_status q3_batcher_create(q3_model* m, int slots, int frame_budget, int prompt_budget, q3_batcher** out) {
    if (!m || !out) return set_err(Q3_INVALID_ARG, "q3_batcher_create: null argument");
    if (!m->finalized) return set_err(Q3_INVALID_ARG, "model not finalized");
    if (slots < 1 || slots > Q3_MAX_BATCH) return set_err(Q3_UNSUPPORTED, "q3_batcher_create: %d rows unsupported (1..%d)", slots, Q3_MAX_BATCH);
    if (frame_budget < 1 || prompt_budget < 0) return set_err(Q3_INVALID_ARG, "q3_batcher_create: frame_budget must be >= 1, prompt_budget >= 0");
    {   // the session the first step opens: max_seq = max(prompt_budget, 16) + frame_budget + 1 positions of the RoPE table
        const long need = (long)(prompt_budget > 16 ? prompt_budget : 16) + frame_budget + 1;
        if (need > m->rope_len) return set_err(Q3_KV_OVERFLOW, "q3_batcher_create: prompt_budget + frame_budget = %ld positions exceed the RoPE table (%d)", need, m->rope_len);
    }
    std::unique_ptr<q3_batcher> b(new q3_batcher());
    b->m = m; b->slots = slots; b->frame_budget = frame_budget; b->prompt_budget = prompt_budget;
    b->owner.assign(slots, -1); b->commit.assign(slots, 0);
    b->dec.reset(new BatDecoder());
    // the streamed tickets' codec stream: frames per block (a multiple of 32, default 128) and the block limit (default none)
    if (const char* e = getenv("Q3_BAT_STREAM_BLOCK_FRAMES")) {
        const int v = atoi(e);
        if (v < 32 || v % 32 != 0) return set_err(Q3_INVALID_ARG, "Q3_BAT_STREAM_BLOCK_FRAMES=%s: not a positive multiple of 32", e);
        b->s_block_frames = v;
    }
    if (const char* e = getenv("Q3_BAT_STREAM_MAX_BLOCKS")) {
        const int v = atoi(e);
        if (v < 0) return set_err(Q3_INVALID_ARG, "Q3_BAT_STREAM_MAX_BLOCKS=%s: negative", e);
        b->s_max_blocks = v;
    }
    *out = b.release();
    return Q3_OK;
}
extern "C" void q3_batcher_free(q3_batcher* b) {
    if (!b) return;
    stage_drop(b);
    if (b->tx_steps > 0 && getenv("Q3_BAT_TEXT_STATS"))
        fprintf(stderr, "[q3 batcher text] %ld flushes in %ld steps, %ld tokens, %.3f ms in flushes (%.4f ms per step)\n", b->tx_flushes, b->tx_steps, b->tx_tokens,
                b->tx_ms, b->tx_ms / b->tx_steps);
    for (int64_t id : b->parked) { q3_parked_free(b->t[id]->rec); b->t[id]->rec = nullptr; }      // what is still parked gives its pages back
    b->parked.clear();
    if (b->dec) decoder_stop(b);                       // finishes what is queued (tickets nobody will fetch included), then ends the worker
    if (b->s) q3_session_free(b->s);
    delete b;
}
static void queue_enter(q3_batcher* b, int64_t id, bool fresh);
static q3_status batcher_submit(q3_batcher* b, const q3_request* req, int want_pcm, bool streamed, int64_t* ticket);
extern "C" q3_status q3_batcher_submit(q3_batcher* b, const q3_request* req, int want_pcm, int64_t* ticket) {
    if (!b || !req || !ticket) return set_err(Q3_INVALID_ARG, "q3_batcher_submit: null argument");
    return batcher_submit(b, req, want_pcm, false, ticket);
}
extern "C" q3_status q3_batcher_submit_streamed(q3_batcher* b, const q3_request* req, int64_t* ticket) {
    if (!b || !req || !ticket) return set_err(Q3_INVALID_ARG, "q3_batcher_submit_streamed: null argument");
    if (b->m->device < 0) return set_err(Q3_INVALID_ARG, "q3_batcher_submit_streamed: the model has no device (manifest-only): the vocoder runs on the GPU");
    if (req->n_ref > 0 && req->ref_codes && (long)req->n_ref + req->opts.max_length > (long)b->frame_budget + b->prompt_budget)
        return set_err(Q3_UNSUPPORTED, "q3_batcher_submit_streamed: %d reference frames + max_length %d exceed the stream's %d frames (frame_budget + prompt_budget)",
                       req->n_ref, req->opts.max_length, b->frame_budget + b->prompt_budget);
    return batcher_submit(b, req, 0, true, ticket);
}
static q3_status batcher_submit(q3_batcher* b, const q3_request* req, int want_pcm, bool streamed, int64_t* ticket) {
    if (req->opts.max_length < 1 || req->opts.max_length > b->frame_budget)
        return set_err(Q3_UNSUPPORTED, "q3_batcher_submit: max_length %d outside 1..%d (the batcher's frame budget)", req->opts.max_length, b->frame_budget);
    if (req->n_text < 0 || req->n_instruct < 0 || req->n_ref < 0 || req->n_ref_text < 0) return set_err(Q3_INVALID_ARG, "q3_batcher_submit: negative length");
    std::unique_ptr<BatTicket> t(new BatTicket());
    t->req.own(*req, b->m->cfg.hidden); t->want_pcm = want_pcm != 0; t->streamed = streamed; t->born = b->steps;
    if (streamed) b->n_streamed++;
    const int64_t id = b->next_id++;
    b->t[id] = std::move(t);
    queue_enter(b, id, true);
    *ticket = id;
    return Q3_OK;
}

// ---- open tickets: the text arrives in pieces ----
// trailing text rows of a text of n_text tokens: what the prefill does not consume
static int ticket_n_trail(const BatTicket& t, size_t n_text) { return prompt_shape(t.req.r, (int)n_text).n_trail; }
// the frame limit of an open ticket with the text it has: its max_length, once its text is closed under the ICL cap over that text
static int ticket_limit(const BatTicket& t) { return t.closed ? prompt_shape(t.req.r, (int)t.text_all.size()).limit : t.req.r.opts.max_length; }
// text rows a slot of the batcher's session takes from an open ticket (its last row holds tts_pad: transplant_row)
static int batcher_text_cap(const q3_batcher* b) { return (b->prompt_budget > 16 ? b->prompt_budget : 16) + 1024 - 1; }

extern "C" q3_status q3_batcher_submit_open(q3_batcher* b, const q3_request* req, int want, int64_t* ticket) {
    if (!b || !req || !ticket) return set_err(Q3_INVALID_ARG, "q3_batcher_submit_open: null argument");
    if (want != Q3_WANT_CODES && want != Q3_WANT_PCM && want != Q3_WANT_STREAM) return set_err(Q3_INVALID_ARG, "q3_batcher_submit_open: want %d is none of Q3_WANT_CODES / _PCM / _STREAM", want);
    if (b->m->device < 0) return set_err(Q3_INVALID_ARG, "q3_batcher_submit_open: the model has no device (manifest-only)");
    // what q3_session_open_text asks of the row (the side session is opened when the ticket reaches the head of the queue)
    if (req->n_text < 1 || !req->text_ids)
        return set_err(Q3_INVALID_ARG, "q3_session_open_text: the request has no text token (an open row needs one at creation: the prefill consumes it)");
    for (int i = 0; i < req->n_text; ++i) if (req->text_ids[i] >= (uint32_t)b->m->cfg.text_vocab) return set_err(Q3_INVALID_ARG, "text id %u out of range", req->text_ids[i]);
    const PromptShape sh = prompt_shape(*req);
    if (sh.icl) {
        const int need = sh.open_need;
        if (req->n_text < need)
            return set_err(Q3_INVALID_ARG, "q3_session_open_text: the ICL request needs at least %d target text tokens at creation (%d given), so that tts_eos falls after the ICL block", need, req->n_text);
        if (req->opts.max_length > b->frame_budget)
            return set_err(Q3_UNSUPPORTED, "q3_session_open_text: the ICL request asks for max_length %d beyond the frame budget %d (its length cap is resolved when the text closes)", req->opts.max_length, b->frame_budget);
    }
    int64_t id = 0;
    if (want == Q3_WANT_STREAM) Q3C(q3_batcher_submit_streamed(b, req, &id));
    else Q3C(batcher_submit(b, req, want == Q3_WANT_PCM, false, &id));
    BatTicket& t = *b->t[id];
    t.open = true; t.text_all = t.req.text;
    if (ticket_n_trail(t, t.text_all.size()) + 1 > batcher_text_cap(b)) {
        b->queue.erase(std::remove(b->queue.begin(), b->queue.end(), id), b->queue.end()); if (t.streamed) b->n_streamed--; b->t.erase(id);
        return set_err(Q3_UNSUPPORTED, "q3_batcher_submit_open: the text exceeds the row's slot (%d rows)", batcher_text_cap(b));
    }
    b->want_text = true;
    *ticket = id;
    return Q3_OK;
}

extern "C" q3_status q3_batcher_append_text(q3_batcher* b, int64_t ticket, const uint32_t* ids, int n, int last) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_append_text: null batcher");
    if (n < 0 || (n > 0 && !ids)) return set_err(Q3_INVALID_ARG, "q3_batcher_append_text: bad token id array");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_append_text: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    if (!t.open) return set_err(Q3_INVALID_ARG, "q3_batcher_append_text: ticket %lld was not submitted open (q3_batcher_submit_open)", (long long)ticket);
    if (t.closed) return set_err(Q3_INVALID_ARG, "q3_batcher_append_text: ticket %lld's text is already closed", (long long)ticket);
    for (int i = 0; i < n; ++i) if (ids[i] >= (uint32_t)b->m->cfg.text_vocab) return set_err(Q3_INVALID_ARG, "text id %u out of range", ids[i]);
    const int rows = ticket_n_trail(t, t.text_all.size() + (size_t)n) + 1;
    if (rows > batcher_text_cap(b)) return set_err(Q3_UNSUPPORTED, "q3_batcher_append_text: %d trailing text rows exceed the row's slot (%d)", rows, batcher_text_cap(b));
    // recorded only: the frames see it after the next flush (q3_batcher_step). A ticket that has ended takes it and ignores it.
    t.text_all.insert(t.text_all.end(), ids, ids + n);
    if (last) t.closed = true;
    return Q3_OK;
}

extern "C" q3_status q3_batcher_text_state(q3_batcher* b, int64_t ticket, int* n_text, int* frames_committed, int* frames_runnable, int* closed) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_text_state: null batcher");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_text_state: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    int committed = 0, runnable = 0;
    // what the text received so far allows (tokens the next flush will publish included), as q3_session_text_state counts
    const int lim = t.open ? ticket_limit(t) : 0;
    const int allowed = !t.open ? 0 : t.closed ? lim : std::min(lim, ticket_n_trail(t, t.text_all.size()));
    if (t.state == Q3_TICKET_QUEUED) runnable = t.open ? allowed : t.req.r.opts.max_length;
    else if (t.state == Q3_TICKET_PARKED) {
        committed = parked_committed(t.rec);
        runnable = parked_done(t.rec) ? 0 : std::max(0, (t.open ? allowed : parked_seq(t.rec).limit) - committed);
    } else if (t.row >= 0 && b->s) {
        int done = 0;
        Q3C(q3_session_frames(b->s, t.row, nullptr, &done));
        committed = session_row_committed(b->s, t.row);
        runnable = done ? 0 : (t.open ? allowed : b->s->seq[(size_t)t.row].limit) - committed;
        if (runnable < 0) runnable = 0;
    } else committed = t.n_frames;
    if (n_text) *n_text = (int)(t.open ? t.text_all.size() : t.req.text.size());
    if (frames_committed) *frames_committed = committed;
    if (frames_runnable) *frames_runnable = runnable;
    if (closed) *closed = (!t.open || t.closed) ? 1 : 0;
    return Q3_OK;
}

static void bat_fail(BatTicket& t, q3_status st) { t.state = Q3_TICKET_FAILED; t.st = st; t.err = q3_last_error(); t.row = -1; }

// frames [t.s_pushed, n_total) of a streamed ticket's row (frames = the row's codes from frame 0) join the parts of this step
static void stream_part(q3_batcher* b, BatTicket& t, int row, const uint32_t* frames, int n_total, bool last) {
    if (n_total < t.s_pushed) {
        // frames past the row's end would have gone to the worker (samples nobody should hear): a row's frame count never shrinks
        // (refresh_codes cuts at the EOS before a frame is handed over), so this is a broken invariant — the ticket fails, loudly
        std::lock_guard<std::mutex> g(b->dec->mu);
        if (!t.s_failed) {
            t.s_failed = true; t.s_st = Q3_INVALID_ARG;
            t.s_err = "streamed ticket: " + std::to_string(t.s_pushed) + " frames were handed to the vocoder, the row ended at " + std::to_string(n_total);
        }
        n_total = t.s_pushed;
    }
    if (!last && n_total == t.s_pushed) return;
    if (b->max_parked > 0) {
        // parking on: the stream row follows the ticket, not the slot — taken with its first part, returned with its last (jobs run
        // in order and a job is cut where a row repeats, so the row's next owner's first part is served after this last one)
        if (t.srow < 0) {
            // (slots + max_parked rows for at most that many tickets in rows or parked; should a row have been lost on an error path,
            // this ticket fails with a message instead)
            if (b->srow_free.empty()) {
                std::lock_guard<std::mutex> g(b->dec->mu);
                if (!t.s_failed) { t.s_failed = true; t.s_st = Q3_OOM; t.s_err = "streamed ticket: no free row of the decode worker's stream"; }
                return;
            }
            t.srow = b->srow_free.back(); b->srow_free.pop_back();
        }
        row = t.srow;
        if (last) { b->srow_free.push_back(t.srow); std::sort(b->srow_free.begin(), b->srow_free.end(), std::greater<int>()); t.srow = -1; }
    }
    StreamPart p{&t, row, {}, !t.s_started, last};
    if (n_total > t.s_pushed) p.frames.assign(frames + (size_t)t.s_pushed * 16, frames + (size_t)n_total * 16);
    t.s_started = true; t.s_pushed = n_total;
    b->sparts.push_back(std::move(p));
}
// a streamed ticket that leaves without a last part (the worker failed it) gives its stream row back
static void stream_row_release(q3_batcher* b, BatTicket& t) {
    if (t.srow < 0) return;
    b->srow_free.push_back(t.srow); std::sort(b->srow_free.begin(), b->srow_free.end(), std::greater<int>()); t.srow = -1;
}
// the row's sequence has ended: keep its codes (and PCM), free the row
static q3_status bat_collect(q3_batcher* b, int row) {
    BatTicket& t = *b->t[b->owner[row]];
    int n = 0;
    Q3C(q3_session_codes(b->s, row, nullptr, 0, &n));
    t.codes.resize((size_t)n * 16); t.n_frames = n;
    if (n > 0) Q3C(q3_session_codes(b->s, row, t.codes.data(), n, &n));
    bool async = false;
    if (t.streamed) {
        // its last part: the frames up to its end that no step has handed over yet; DONE once the worker has served it
        stream_part(b, t, row, t.codes.data(), n, true);
        t.s_ended = true; async = true;
    } else
    if (t.want_pcm && n > 0) {
        static const bool sync_decode = getenv("Q3_BAT_SYNC_DECODE") != nullptr;
        t.pcm.resize((size_t)n * samples_per_frame(b->m->cfg));
        if (!sync_decode && b->s->seq[(size_t)row].ref_codes.empty()) {
            // the worker vocodes it from the host copy of the codes while the row is refilled and the frames go on
            t.decoding = true; t.dec_done.store(false);
            try { decoder_push(b, &t); async = true; } catch (...) { t.decoding = false; }
        }
        if (!async) {
            size_t ns = 0;
            Q3C(q3_session_decode(b->s, row, 0, n, t.pcm.data(), t.pcm.size(), &ns));
            t.pcm.resize(ns);
        }
    }
    t.state = async ? Q3_TICKET_RUNNING : t.cancelled ? Q3_TICKET_CANCELLED : Q3_TICKET_DONE; t.row = -1;
    b->owner[row] = -1; b->commit[row] = 0;
    // the device freezes a row at its frame limit, not at EOS: idle it now so that it stops advancing — and taking pages — while
    // the queue is empty or waits for room; its pages but one go back to the pool
    return session_idle_row(b->s, row);
}

// ---- parked tickets (q3_batcher_set_parking) ----
// frames the text an open ticket has received allows (unflushed tokens included), as q3_batcher_text_state counts them
static int ticket_allowed(const BatTicket& t) {
    const int lim = ticket_limit(t);
    return t.closed ? lim : std::min(lim, ticket_n_trail(t, t.text_all.size()));
}
// an open ticket with `committed` frames can commit another one (or is closed: it runs to its end, or is collected)
static bool ticket_runnable(const BatTicket& t, int committed) { return !t.open || t.closed || ticket_allowed(t) > committed; }
// The one waiting order. fresh_first = 0: FIFO by arrival / park time. fresh_first != 0: a fresh ticket stands ahead of the parked
// ones, behind every earlier fresh one.
static void queue_enter(q3_batcher* b, int64_t id, bool fresh) {
    auto pos = b->queue.end();
    if (fresh && b->fresh_first)
        pos = std::find_if(b->queue.begin(), b->queue.end(), [&](int64_t q) { return b->t[q]->state == Q3_TICKET_PARKED; });
    b->queue.insert(pos, id);
    b->t[id]->in_queue = true;
}
// parked tickets that want a row again enter the waiting list, in park order, once a frame of theirs is runnable
static void parked_requeue(q3_batcher* b) {
    for (int64_t id : b->parked) {
        BatTicket& t = *b->t[id];
        if (t.want_in && !t.in_queue && ticket_runnable(t, parked_committed(t.rec))) queue_enter(b, id, false);
    }
}
static int parked_waiting(const q3_batcher* b) {      // want a row, not in the list yet (an open ticket without text)
    int n = 0;
    for (int64_t id : b->parked) { const BatTicket& t = *b->t.at(id); n += (t.want_in && !t.in_queue) ? 1 : 0; }
    return n;
}
static void stream_part(q3_batcher* b, BatTicket& t, int row, const uint32_t* frames, int n_total, bool last);
// row -> record: the ticket reads PARKED, its row is free. A streamed ticket's frames that no step has handed over yet go to the
// worker as a part with last = false. from_host: q3_batcher_park — the ticket then waits for q3_batcher_unpark.
static q3_status bat_park(q3_batcher* b, int row, bool from_host) {
    const int64_t id = b->owner[row];
    BatTicket& t = *b->t[id];
    q3_parked* rec = nullptr;
    Q3C(q3_session_park_row(b->s, row, &rec));
    if (t.streamed) {
        const uint32_t* codes = nullptr; const int n = parked_frames(rec, &codes);
        if (n > t.s_pushed) stream_part(b, t, row, codes, n, false);
        if (from_host) stream_flush(b);           // (inside a step: with the step's job)
    }
    t.rec = rec; t.state = Q3_TICKET_PARKED; t.last_row = row; t.row = -1; t.units = b->commit[row]; t.want_in = !from_host; t.in_queue = false;
    b->owner[row] = -1; b->commit[row] = 0;
    b->parked.push_back(id); b->n_parks++;
    return Q3_OK;
}
static void parked_forget(q3_batcher* b, int64_t id) {      // the ticket no longer holds a record
    b->parked.erase(std::remove(b->parked.begin(), b->parked.end(), id), b->parked.end());
    b->queue.erase(std::remove(b->queue.begin(), b->queue.end(), id), b->queue.end());
    BatTicket& t = *b->t[id];
    t.rec = nullptr; t.want_in = false; t.in_queue = false;
}

extern "C" q3_status q3_batcher_step(q3_batcher* b, int n_frames, int use_graph, int* n_running, int* n_queued, int* n_finished) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_step: null batcher");
    if (n_frames < 1) return set_err(Q3_INVALID_ARG, "q3_batcher_step: n_frames must be >= 1");
    b->steps++;
    int finished = 0;
    // Open the session on `slots` idle rows: copies of a one-token CustomVoice prompt with a one-frame limit (ten prefill
    // positions per row — opening on the first request itself would prefill, and size every row's KV extent for, `slots`
    // copies of what may be a 4k-token prompt), frozen before the first frame. Every request, the first included, then enters
    // through q3_session_replace, so prompt kinds mix freely.
    if (!b->s && !b->queue.empty()) {
        // The idle rows are built from fixed, known-valid values — never from a queued request: a malformed first request must
        // fail alone, at its own q3_session_replace below, not wedge the queue by failing the session every step.
        const q3_request& first = b->t[b->queue.front()]->req.r;
        b->chunk_frames = first.opts.chunk_frames >= 1 ? first.opts.chunk_frames : 10;       // the one option a session shares
        const q3_request d = idle_request(b->chunk_frames);
        std::vector<q3_request> reqs((size_t)b->slots, d);
        q3_session* s = nullptr;
        q3_status st = session_create(b->m, reqs.data(), b->slots, b->frame_budget, b->prompt_budget > 16 ? b->prompt_budget : 16, &s);
        if (st == Q3_OK) st = q3_session_prefill(s);
        if (st != Q3_OK) {
            // nothing a request could have caused (the budgets were checked at q3_batcher_create): a device failure. The head
            // ticket takes the error so that a serving loop sees it on a ticket and the queue moves on.
            if (s) q3_session_free(s);
            const int64_t id = b->queue.front(); b->queue.erase(b->queue.begin());
            bat_fail(*b->t[id], st);
            if (n_running) *n_running = 0; if (n_queued) *n_queued = (int)b->queue.size(); if (n_finished) *n_finished = 1;
            return st;
        }
        b->s = s;
        for (int r = 0; r < b->slots; ++r) Q3C(session_idle_row(s, r));
    }
    if (!b->s) { if (n_running) *n_running = 0; if (n_queued) *n_queued = 0; if (n_finished) *n_finished = finished; return Q3_OK; }
    // the first open ticket switches the hold path on: text_ready and the append scratch; a frame captured before is captured
    // again by the next q3_session_generate (nothing is in flight between two steps). Never for a batcher without open tickets.
    if (b->want_text && !b->s->text_ready) Q3C(session_text_enable(b->s));
    if (b->want_text) b->tx_steps++;
    // Admission under a page limit (q3_model_kv_pool_limit): a request enters a row only if its WORST CASE (prompt + max_length
    // positions; row_worst_units) fits beside what the running rows may still come to hold and what everything else on the model
    // holds now — so a page shortage shows up here, as a request that waits in the queue (rows are running: room will come) or
    // fails on its ticket (it cannot fit even alone), never in the middle of a generation where it would stop every row.
    auto held_units = [&](int r) -> long { return (long)b->s->kv_rows[(size_t)r].size() * (b->s->kv_in_bf16 ? 1 : 2); };
    auto admit = [&](const q3_request& rq, bool open, long* units_out, bool* wait, long extra = 0) -> bool {
        *wait = false; *units_out = 0;
        if (!b->s->paged) return true;
        const PromptShape sh = prompt_shape(rq);
        const int lim = open ? rq.opts.max_length : sh.limit;          // an open ICL ticket's length cap is not known before its text closes
        const long units = row_worst_units(sh.prefill_len, lim, b->s->kv_bf16);
        *units_out = units;
        long mine = 0, claimed = 0; int running = 0;
        for (int r = 0; r < b->slots; ++r) {
            const long h = held_units(r);
            mine += h;
            if (b->owner[r] >= 0) { claimed += std::max(b->commit[r], h); running++; } else claimed += h;
        }
        // a parked ticket counts exactly as if it still sat in a row: the pages its record holds, and its worst case
        for (int64_t pid : b->parked) {
            const BatTicket& pt = *b->t[pid];
            const long h = (long)parked_pages(pt.rec) * (b->s->kv_in_bf16 ? 1 : 2);
            mine += h; claimed += std::max(pt.units, h);
            // (only a ticket that wants a row again makes a request WAIT for it: one the host holds parked may stay so for ever,
            // and a request that cannot fit beside it fails on its ticket, as it does when nothing runs)
            if (pt.want_in) running++;
        }
        // pages only the prefix cache holds are reclaimable (kv_take evicts them before a row's request fails): they do not stand
        // in a request's way. A request is never discounted for the pages it hopes to find cached.
        const long reclaim = 2L * prefix_reclaimable(b->m);
        std::lock_guard<std::mutex> g(b->m->kv_budget.mu);
        if (b->m->kv_budget.limit <= 0) return true;
        const long others = std::max(0L, b->m->kv_budget.used - mine - reclaim);
        if (others + claimed + units + extra <= b->m->kv_budget.limit) return true;      // (extra: the page a row vacated by a park will hold)
        *wait = running > 0;
        return false;
    };
    auto fill = [&]() -> q3_status {               // free rows <- waiting requests
        for (int r = 0; r < b->slots && !b->queue.empty(); ++r) {
            if (b->owner[r] >= 0) continue;
            while (!b->queue.empty()) {
                const int64_t id = b->queue.front();
                BatTicket& t = *b->t[id];
                long units = 0; bool wait = false;
                if (t.state == Q3_TICKET_PARKED) {
                    // a parked ticket enters by q3_session_resume_row, into whichever row is free; its admission claim never left
                    q3_parked* rec = t.rec; const int committed = parked_committed(rec); const long claim = t.units;
                    const q3_status st = q3_session_resume_row(b->s, r, rec);
                    parked_forget(b, id);
                    if (st != Q3_OK) { q3_parked_free(rec); stream_row_release(b, t); bat_fail(t, st); finished++; continue; }
                    t.state = Q3_TICKET_RUNNING; t.row = r; t.entered = committed; b->owner[r] = id; b->commit[r] = claim;
                    b->n_resumes++; if (r != t.last_row) b->n_moved++;
                    break;
                }
                if (!admit(t.req.r, t.open, &units, &wait)) {
                    if (wait) {
                        // FIFO: the head of the queue waits for running rows to end — and for parked tickets, whose claims stand in
                        // its way like a running row's: the first parked ticket of the list goes ahead (it needs no admission)
                        auto pk = std::find_if(b->queue.begin(), b->queue.end(), [&](int64_t x) { return b->t[x]->state == Q3_TICKET_PARKED; });
                        if (pk == b->queue.end()) return Q3_OK;
                        std::rotate(b->queue.begin(), pk, pk + 1);
                        continue;
                    }
                    b->queue.erase(b->queue.begin());
                    if (b->stage.id == id) stage_drop(b);      // (a limit set after it was prefilled ahead) its side session goes with it
                    const PromptShape sh = prompt_shape(t.req.r);
                    bat_fail(t, set_err(Q3_KV_OVERFLOW, "KV page pool exhausted: the request's %d prompt positions + %d frames need %ld page(s) (f32 equivalents), more than the pool's limit leaves",
                                        sh.prefill_len, sh.limit, (units + 1) / 2));
                    finished++; continue;
                }
                b->queue.erase(b->queue.begin());
                t.req.r.opts.chunk_frames = b->chunk_frames;        // the one option a session shares
                q3_status st;
                if (b->stage.id == id) {
                    // prefilled ahead on the worker's stream: wait for it (normally long done), then only the state copy stands
                    // between two frames of the live rows
                    stage_join(b);
                    st = b->stage.st;
                    if (st != Q3_OK) set_err(st, "%s", b->stage.err.c_str());
                    else {
                        st = sync_frames(b->s) == hipSuccess ? Q3_OK : Q3_HIP_ERROR;      // no frame of the host session in flight while its row changes
                        if (st == Q3_OK) st = transplant_row(b->s, r, b->stage.side, 0, b->stage.limit);
                    }
                    stage_drop(b);
                } else if (t.open) {
                    // with the text it has at this moment; what arrives later goes in with the flushes
                    q3_request rq = t.req.r;
                    rq.text_ids = t.text_all.data(); rq.n_text = (int32_t)t.text_all.size();
                    t.n_taken = t.text_all.size(); t.close_taken = t.closed;
                    st = session_replace(b->s, r, &rq, true, t.closed);
                } else
                    st = q3_session_replace(b->s, r, &t.req.r);
                if (st != Q3_OK) { bat_fail(t, st); finished++; continue; }     // does not fit: the ticket carries the reason; try the next one
                t.state = Q3_TICKET_RUNNING; t.row = r; t.entered = 0; t.in_queue = false; b->owner[r] = id; b->commit[r] = units;
                break;
            }
        }
        return Q3_OK;
    };
    // the head of the queue starts its prefill on the worker (see q3_batcher::Stage); called with frames about to be queued
    auto stage_begin = [&]() {
        const bool off = getenv("Q3_BAT_NO_STAGE") != nullptr;      // (read per step: a test flips it between two batchers)
        if (off || b->stage.id >= 0 || b->queue.empty() || b->s->debug || b->s->profile) return;
        // not while this thread may still CAPTURE the host session's frame (the first graph step): one thing less to go wrong
        // (captures are in relaxed mode and repeated when invalidated: q3_session.hip frame_capture)
        if (use_graph ? b->s->graph == nullptr : false) return;
        { std::lock_guard<std::mutex> g(b->m->kv_budget.mu); if (b->m->kv_budget.limit > 0) return; }
        bool any_free = false;
        for (int r = 0; r < b->slots; ++r) any_free = any_free || b->owner[r] < 0;
        if (any_free) return;                        // a free row takes the head at once (fill): nothing to run ahead of
        const int64_t id = b->queue.front();
        BatTicket& t = *b->t[id];
        if (t.state == Q3_TICKET_PARKED) return;     // the worker serves fresh tickets only: a parked one enters by a state copy
        q3_request rq = t.req.r;                     // (arrays owned by the ticket, which lives until it is fetched)
        rq.opts.chunk_frames = b->chunk_frames;
        // an open ticket is staged with a copy of the text it has now (q3_batcher_append_text may grow the ticket's own while the
        // worker reads); what arrives later is applied by the first flush after the transplant
        const bool open = t.open, closed = t.closed;
        std::vector<uint32_t> text_now;
        if (open) { text_now = t.text_all; t.n_taken = text_now.size(); t.close_taken = closed; }
        const int limit_req = rq.opts.max_length;
        if (limit_req < 1 || limit_req > b->s->max_frames) return;      // the synchronous path reports it on the ticket
        b->stage.id = id; b->stage.st = Q3_OK; b->stage.err.clear(); b->stage.side = nullptr; b->stage.limit = 0;
        q3_batcher* bp = b;
        try {
        b->stage.thr = std::thread([bp, rq, limit_req, open, closed, text_now]() {
            q3_batcher::Stage& g = bp->stage;
            std::unique_ptr<q3_session> side;
            q3_request rw = rq;
            if (open) { rw.text_ids = text_now.data(); rw.n_text = (int32_t)text_now.size(); }
            q3_status st = hipSetDevice(bp->m->device) == hipSuccess ? Q3_OK : set_err(Q3_HIP_ERROR, "hipSetDevice");
            if (st == Q3_OK) st = side_prefill(bp->s, &rw, &limit_req, 1, open, closed, false, nullptr, &side, &g.limit);      // a stream of its own: runs beside the frames
            g.side = side.release(); g.st = st;
            if (st != Q3_OK) g.err = q3_last_error();
        });
        } catch (...) { b->stage.id = -1; }          // no thread to be had: the swap prefills synchronously, as before
    };
    // Run in pieces that end where the next row reaches its frame limit: that row is collected and refilled at once instead of
    // idling to the end of the step (a row that ends on EOS is noticed at q3_session_generate's 32-frame check or at the
    // end of the piece)
    // The text flush, at the start of every piece (nothing is in flight): what q3_batcher_append_text recorded for the running
    // open tickets since their last flush — tickets that were queued or staged meanwhile included — goes to the device in one
    // session_append_many: projected together, published together, one synchronisation.
    auto flush_text = [&]() -> q3_status {
        if (!b->want_text) return Q3_OK;
        std::vector<TextPiece> pieces;
        for (int r = 0; r < b->slots; ++r) {
            if (b->owner[r] < 0) continue;
            BatTicket& t = *b->t[b->owner[r]];
            if (!t.open || (t.n_taken == t.text_all.size() && t.close_taken == t.closed)) continue;
            pieces.push_back({r, t.text_all.data() + t.n_taken, (int)(t.text_all.size() - t.n_taken), t.closed});
        }
        if (pieces.empty()) return Q3_OK;
        const auto t0 = std::chrono::steady_clock::now();
        Q3C(session_append_many(b->s, pieces));
        for (const TextPiece& p : pieces) {
            BatTicket& t = *b->t[b->owner[p.b]];
            b->tx_tokens += p.n; t.n_taken = t.text_all.size(); t.close_taken = t.closed;
        }
        b->tx_flushes++; b->tx_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return Q3_OK;
    };
    // The time slice (quantum_frames > 0), at the start of every piece: while something waits, no row is free and fewer than
    // max_parked tickets are parked, ONE running ticket is parked — a HELD one first (it counts as having used its quantum), else
    // the one that has committed the most frames since it entered its row if that is at least the quantum; ties go to the lowest
    // row — and the list's head takes its row (fill). Reads no clock: a function of submissions, steps and frames.
    auto used_of = [&](int r) { return session_row_committed(b->s, r) - b->t[b->owner[r]]->entered; };
    auto slice = [&]() -> q3_status {
        std::vector<int64_t> mine;                   // parked by this call: the list is served until one of them is its head
        for (;;) {
            parked_requeue(b);
            if (!b->queue.empty() && std::find(mine.begin(), mine.end(), b->queue.front()) != mine.end()) return Q3_OK;
            if (b->quantum <= 0 || b->queue.empty() || (int)b->parked.size() >= b->max_parked) return Q3_OK;
            for (int r = 0; r < b->slots; ++r) if (b->owner[r] < 0) return Q3_OK;
            {   // a fresh head that admission would keep waiting gains nothing from a free row (a parked ticket keeps its claim)
                BatTicket& h = *b->t[b->queue.front()];
                long units = 0; bool wait = false;
                if (h.state != Q3_TICKET_PARKED && !admit(h.req.r, h.open, &units, &wait, b->s->kv_in_bf16 ? 1 : 2)) return Q3_OK;
            }
            int victim = -1, most = -1;
            for (int r = 0; r < b->slots && victim < 0; ++r) {
                const BatTicket& t = *b->t[b->owner[r]];
                if (t.open && !ticket_runnable(t, session_row_committed(b->s, r))) victim = r;      // HELD
            }
            if (victim < 0) {
                for (int r = 0; r < b->slots; ++r) { const int u = used_of(r); if (u > most) { most = u; victim = r; } }
                if (most < b->quantum) return Q3_OK;
            }
            const int64_t vid = b->owner[victim];
            const q3_status st = bat_park(b, victim, false);
            if (st == Q3_KV_OVERFLOW) return Q3_OK;      // no page for the vacated row under the limit: nothing changed, no slice now
            Q3C(st);
            mine.push_back(vid);
            Q3C(fill());
        }
    };
    for (int left = n_frames; left > 0;) {
        Q3C(fill());
        if (b->max_parked > 0) Q3C(slice());
        Q3C(flush_text());
        int piece = left, busy = 0;
        for (int r = 0; r < b->slots; ++r) {
            if (b->owner[r] < 0) continue;
            // (an open row's progress is what it has COMMITTED, not frames_run - start_run: it may have been held; a held row —
            // nothing runnable with the text it has — does not make the piece busy)
            const int rem = session_row_remaining(b->s, r);
            if (rem > 0) { busy++; if (rem < piece) piece = rem; }
            // something waits: the piece also ends where this row's quantum does
            if (b->quantum > 0 && rem > 0 && !b->queue.empty()) { const int u = used_of(r); if (u < b->quantum && b->quantum - u < piece) piece = b->quantum - u; }
        }
        if (busy > 0) {
            stage_begin();
            const q3_status gst = q3_session_generate(b->s, piece, use_graph);
            if (gst == Q3_KV_OVERFLOW && b->s->kv_overflow_row >= 0 && b->owner[b->s->kv_overflow_row] >= 0) {
                // (only reachable when something outside this batcher took the pages its admission counted on) nothing ran: the
                // row that needs the page fails alone and is frozen; the others go on
                const int row = b->s->kv_overflow_row;
                bat_fail(*b->t[b->owner[row]], gst);
                stream_row_release(b, *b->t[b->owner[row]]);
                b->owner[row] = -1; b->commit[row] = 0;
                Q3C(session_idle_row(b->s, row));
                finished++;
                continue;
            }
            Q3C(gst);
            left -= piece;
        }
        int collected = 0;
        for (int r = 0; r < b->slots; ++r) {
            if (b->owner[r] < 0) continue;
            {   // a row without a live EOS id ends exactly at its frame limit, which the host knows: no device read-back (a
                // synchronisation and nine blocking copies per step) while no row can have ended
                const SeqInfo& q = b->s->seq[r];
                if (q.req.opts.eos_token_id < 0 && session_row_committed(b->s, r) < q.limit) continue;
            }
            int n = 0, done = 0;
            Q3C(q3_session_frames(b->s, r, &n, &done));
            if (done) { Q3C(bat_collect(b, r)); finished++; collected++; }
        }
        if (busy == 0 && collected == 0) break;          // nothing runs and nothing is waiting for a row
    }
    // Streamed tickets: the frames of this step come to the host and go to the decode worker as ONE job over every streamed row
    // (a row that ended inside the step has its part already, up to its end: bat_collect). The step does not wait for the job.
    // A ticket the worker could not serve (a refused or failed push) gives up its row here.
    if (b->n_streamed > 0) {
        for (int r = 0; r < b->slots; ++r) {
            if (b->owner[r] < 0) continue;
            BatTicket& t = *b->t[b->owner[r]];
            if (!t.streamed) continue;
            bool failed; { std::lock_guard<std::mutex> g(b->dec->mu); failed = t.s_failed; }
            if (failed) {
                t.state = Q3_TICKET_FAILED; t.st = t.s_st; t.err = t.s_err; t.row = -1;
                stream_row_release(b, t);
                b->owner[r] = -1; b->commit[r] = 0;
                Q3C(session_idle_row(b->s, r));
                finished++;
                continue;
            }
            int n = 0, done = 0;
            Q3C(q3_session_frames(b->s, r, &n, &done));        // (one read-back serves every row: the session's host copy of the codes)
            if (n > t.s_pushed) stream_part(b, t, r, &b->s->codes_host[(size_t)r * b->s->max_frames * 16], n, false);
        }
        stream_flush(b);
    }
    Q3C(fill());                                   // the next step starts with full rows
    int running = 0;
    for (int r = 0; r < b->slots; ++r) running += b->owner[r] >= 0 ? 1 : 0;
    // Nothing runs and nothing waits: the rows that just ended may still be with the decode worker. Their samples are waited for
    // HERE, so that a host loop that stops on "running == 0 && queued == 0" finds every ticket DONE, as it always did.
    parked_requeue(b);
    const int queued = (int)b->queue.size() + parked_waiting(b);      // (parked tickets that want a row count as queued: a host loop must not stop on them)
    if (running == 0 && queued == 0)
        for (auto& kv : b->t) { ticket_wait_decode(b, *kv.second); stream_settle(b, *kv.second, true); }
    if (n_running) *n_running = running;
    if (n_queued) *n_queued = queued;
    if (n_finished) *n_finished = finished;
    return Q3_OK;
}

// the samples of a ticket's host codes on the session's stream and workspace, as q3_session_decode gives them for a whole row:
// an ICL ticket's reference frames go in front (vocode_enqueue cuts their samples)
static q3_status decode_host_codes(q3_batcher* b, BatTicket& t) {
    q3_session* s = b->s;
    HIPC(hipSetDevice(b->m->device));
    HIPC(sync_frames(s));
    const bool icl = t.req.r.mode == Q3_MODE_VOICE_CLONE && !t.req.ref_codes.empty();
    VocodePcm pcm;
    Q3C(vocode_enqueue(b->m, s->cws, s->stream, VocodeSrc{icl ? t.req.ref_codes.data() : nullptr, (int)(t.req.ref_codes.size() / 16), t.codes.data(), true},
                       0, t.n_frames, 0, 0, &pcm));
    HIPC(sync_frames(s));
    t.pcm.resize(pcm.n);
    return vocode_copy_out(pcm, t.pcm.data(), t.pcm.size(), nullptr, nullptr);
}
// A ticket whose client went away gives its place back. Synchronous: between two steps nothing of the session is in flight.
// Queued: it leaves the queue (a side session staged for it is dropped with its pages). Running: its row is collected with the
// frames it has committed — the codes, and their samples: every layer of the vocoder is causal, so they are the first n * 1920
// samples of what the full run would have given; a streamed ticket's last part goes to the worker with last = true, which gives
// the slot's blocks back —, idled, and free for the next fill. The samples are waited for here, so the ticket reads CANCELLED on return.
extern "C" q3_status q3_batcher_cancel(q3_batcher* b, int64_t ticket) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_cancel: null batcher");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_cancel: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    if (t.state == Q3_TICKET_QUEUED) {
        b->queue.erase(std::remove(b->queue.begin(), b->queue.end(), ticket), b->queue.end());
        if (b->stage.id == ticket) stage_drop(b);
        t.cancelled = true; t.state = Q3_TICKET_CANCELLED; t.n_frames = 0; t.s_ended = true;
        return Q3_OK;
    }
    if (t.state == Q3_TICKET_PARKED) {
        // out of the record: the codes it has committed, their decode for want_pcm (the session's own decode path over the host
        // copy, reference frames of an ICL ticket included), the last part of a streamed ticket; the record's pages go back
        q3_parked* rec = t.rec;
        const uint32_t* codes = nullptr; const int n = parked_frames(rec, &codes);
        t.cancelled = true; t.codes.assign(codes, codes + (size_t)n * 16); t.n_frames = n;
        parked_forget(b, ticket);
        q3_parked_free(rec);
        q3_status st = Q3_OK;
        if (t.streamed) { stream_part(b, t, -1, t.codes.data(), n, true); t.s_ended = true; t.state = Q3_TICKET_RUNNING; stream_settle(b, t, true); }
        else {
            if (t.want_pcm && n > 0) st = decode_host_codes(b, t);
            if (st != Q3_OK) { bat_fail(t, st); return set_err(st, "%s", t.err.c_str()); }
            t.state = Q3_TICKET_CANCELLED;
        }
        return Q3_OK;
    }
    if (t.state != Q3_TICKET_RUNNING || t.row < 0) return Q3_OK;      // DONE / FAILED / CANCELLED, or ended and with the decode worker: nothing to take back
    const int row = t.row;
    t.cancelled = true;
    const q3_status st = bat_collect(b, row);
    if (st != Q3_OK) {           // the row could not be read: the ticket fails, the row is given up all the same
        bat_fail(t, st); t.decoding = false;
        stream_row_release(b, t);
        b->owner[row] = -1; b->commit[row] = 0;
        (void)session_idle_row(b->s, row);
        return set_err(st, "%s", t.err.c_str());
    }
    ticket_wait_decode(b, t);
    stream_settle(b, t, true);
    return Q3_OK;
}

extern "C" q3_status q3_batcher_poll(q3_batcher* b, int64_t ticket, int* state, int* n_frames, size_t* n_samples) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_poll: null batcher");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_poll: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    if (t.decoding && t.dec_done.load()) ticket_wait_decode(b, t);      // its samples have landed: DONE (or FAILED) from here on
    stream_settle(b, t, false);
    if (state) *state = t.state;                                         // a ticket still being vocoded reads RUNNING
    int nf = t.n_frames;
    if (t.state == Q3_TICKET_RUNNING && b->s && t.row >= 0) {       // frames run so far (an EOS inside them is only looked at when the row is collected)
        nf = session_row_committed(b->s, t.row);      // (an open row: the frames it committed — it may have been held)
    }
    if (t.state == Q3_TICKET_PARKED) nf = parked_committed(t.rec);      // the frames it had committed when it left its row
    if (n_frames) *n_frames = nf;
    if (n_samples) *n_samples = t.pcm.size();         // (of a ticket still being vocoded: the samples it WILL hold — the size q3_batcher_fetch wants)
    if (n_samples && t.streamed) { std::lock_guard<std::mutex> g(b->dec->mu); *n_samples = t.out.plain() ? t.spcm.size() : t.sout.size() / t.out.sample_bytes(); }      // streamed: the samples that have landed
    return Q3_OK;
}

extern "C" q3_status q3_batcher_fetch(q3_batcher* b, int64_t ticket, uint32_t* codes_host, int cap_frames, float* pcm_host, size_t cap_samples) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_fetch: null batcher");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_fetch: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    ticket_wait_decode(b, t);                         // a row that ended but is still being vocoded: wait for its samples
    if (t.streamed) {
        // a ticket the worker may still hold parts of is not released under it: a finished (or failed) one waits for them
        if (t.row < 0) stream_settle(b, t, true);      // (a FAILED one too: the queue may still hold parts that name it)
        if ((t.state == Q3_TICKET_DONE || t.state == Q3_TICKET_CANCELLED) && pcm_host)
            return set_err(Q3_INVALID_ARG, "q3_batcher_fetch: ticket %lld is streamed: its samples go through q3_batcher_read", (long long)ticket);
    }
    if (t.state == Q3_TICKET_FAILED) {
        const q3_status st = t.st; const std::string err = t.err;
        if (t.streamed) b->n_streamed--;
        b->t.erase(it);
        return set_err(st, "%s", err.c_str());
    }
    if (t.state != Q3_TICKET_DONE && t.state != Q3_TICKET_CANCELLED) return set_err(Q3_INVALID_ARG, "q3_batcher_fetch: ticket %lld has not finished", (long long)ticket);
    if (codes_host) {
        if (cap_frames < t.n_frames) return set_err(Q3_INVALID_ARG, "codes buffer too small (%d < %d frames)", cap_frames, t.n_frames);
        memcpy(codes_host, t.codes.data(), t.codes.size() * 4);
    }
    if (pcm_host) {
        if (cap_samples < t.pcm.size()) return set_err(Q3_INVALID_ARG, "pcm buffer too small");
        memcpy(pcm_host, t.pcm.data(), t.pcm.size() * 4);
    }
    if (t.streamed) b->n_streamed--;
    b->t.erase(it);
    return Q3_OK;
}


extern "C" q3_status q3_batcher_read(q3_batcher* b, int64_t ticket, float* pcm_host, size_t cap_samples, size_t* n_samples, int* done) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_read: null batcher");
    if (!n_samples || !done || (cap_samples > 0 && !pcm_host)) return set_err(Q3_INVALID_ARG, "q3_batcher_read: null argument");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_read: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    if (!t.streamed) return set_err(Q3_INVALID_ARG, "q3_batcher_read: ticket %lld was not submitted as streamed (its samples come with q3_batcher_fetch)", (long long)ticket);
    if (!t.out.plain())
        return set_err(Q3_INVALID_ARG, "q3_batcher_read: ticket %lld has an output of its own (%u Hz, %s): its samples come with q3_batcher_read_out", (long long)ticket,
                       t.out.rate, t.out.fmt == Q3_PCM_S16 ? "s16" : t.out.fmt == Q3_PCM_ULAW ? "ulaw" : t.out.fmt == Q3_PCM_ALAW ? "alaw" : "f32");
    *n_samples = 0; *done = 0;
    stream_settle(b, t, false);
    if (t.state == Q3_TICKET_FAILED) return set_err(t.st, "%s", t.err.c_str());
    std::lock_guard<std::mutex> g(b->dec->mu);
    size_t n = t.spcm.size() - t.s_read;
    if (n > cap_samples) n = cap_samples;
    if (n > 0) memcpy(pcm_host, t.spcm.data() + t.s_read, n * 4);
    t.s_read += n;
    *n_samples = n;
    *done = ((t.state == Q3_TICKET_DONE || t.state == Q3_TICKET_CANCELLED) && t.s_read == t.spcm.size()) ? 1 : 0;
    return Q3_OK;
}

// The ticket setters: `edit` on the ticket's setting, legal for a streamed ticket between its submission and the next step. what: the
// setting's name in the window's refusal.
template <class Edit>
static q3_status ticket_set(q3_batcher* b, int64_t ticket, const char* who, const char* what, Edit edit) {
    if (!b) return set_err(Q3_INVALID_ARG, "%s: null batcher", who);
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "%s: unknown ticket %lld", who, (long long)ticket);
    BatTicket& t = *it->second;
    if (!t.streamed) return set_err(Q3_INVALID_ARG, "%s: ticket %lld was not submitted as streamed", who, (long long)ticket);
    OutSettings o = t.out;
    Q3C(edit(who, o));
    if (t.born != b->steps || t.state != Q3_TICKET_QUEUED)
        return set_err(Q3_INVALID_ARG, "%s: ticket %lld has been through a step: its %s is set between its submission and the next q3_batcher_step", who,
                       (long long)ticket, what);
    t.out = o;
    return Q3_OK;
}
extern "C" q3_status q3_batcher_ticket_output(q3_batcher* b, int64_t ticket, uint32_t sample_rate, int format) {
    return ticket_set(b, ticket, "q3_batcher_ticket_output", "output", [&](const char* who, OutSettings& o) { return out_set_output(who, o, sample_rate, format); });
}
extern "C" q3_status q3_batcher_ticket_tempo(q3_batcher* b, int64_t ticket, int tempo_permille) {
    return ticket_set(b, ticket, "q3_batcher_ticket_tempo", "tempo", [&](const char* who, OutSettings& o) { return out_set_tempo(who, o, tempo_permille); });
}
extern "C" q3_status q3_batcher_ticket_pitch(q3_batcher* b, int64_t ticket, int cents) {
    return ticket_set(b, ticket, "q3_batcher_ticket_pitch", "pitch", [&](const char* who, OutSettings& o) { return out_set_pitch(who, o, cents); });
}
extern "C" q3_status q3_batcher_ticket_level(q3_batcher* b, int64_t ticket, int gain_mB, int ceiling_mB) {
    return ticket_set(b, ticket, "q3_batcher_ticket_level", "level", [&](const char* who, OutSettings& o) { return out_set_level(who, o, gain_mB, ceiling_mB); });
}
extern "C" q3_status q3_batcher_ticket_loudness(q3_batcher* b, int64_t ticket, int mode, int target_mB, int prior_mB) {
    Q3C(ticket_set(b, ticket, "q3_batcher_ticket_loudness", "loudness step",
                   [&](const char* who, OutSettings& o) { return out_set_loudness(who, o, mode, target_mB, prior_mB); }));
    BatTicket& t = *b->t.find(ticket)->second;
    out_loudness_at_rest(t.out, &t.lo_M, &t.lo_gain, &t.lo_blocks, &t.lo_gated);      // (until a part lands)
    return Q3_OK;
}
extern "C" q3_status q3_batcher_ticket_mark(q3_batcher* b, int64_t ticket, uint64_t key, int strength_mB) {
    return ticket_set(b, ticket, "q3_batcher_ticket_mark", "mark", [&](const char* who, OutSettings& o) { return out_set_mark(who, o, key, strength_mB); });
}
extern "C" q3_status q3_batcher_ticket_silence(q3_batcher* b, int64_t ticket, int threshold_mB, int edge_ms, int pause_ms) {
    Q3C(ticket_set(b, ticket, "q3_batcher_ticket_silence", "silence step",
                   [&](const char* who, OutSettings& o) { return out_set_silence(who, o, threshold_mB, edge_ms, pause_ms); }));
    BatTicket& t = *b->t.find(ticket)->second;
    out_silence_at_rest(&t.si[0], &t.si[1], &t.si[2], &t.si[3], &t.si[4]);      // (until a part lands)
    return Q3_OK;
}

extern "C" q3_status q3_batcher_ticket_loudness_read(q3_batcher* b, int64_t ticket, float* mean_square, float* gain, int* blocks, int* gated) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_ticket_loudness_read: null batcher");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_ticket_loudness_read: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    if (t.out.loud == Q3_LOUD_OFF) return set_err(Q3_INVALID_ARG, "q3_batcher_ticket_loudness_read: ticket %lld has no loudness step (q3_batcher_ticket_loudness)", (long long)ticket);
    std::lock_guard<std::mutex> g(b->dec->mu);
    if (mean_square) *mean_square = t.lo_M;
    if (gain) *gain = t.lo_gain;
    if (blocks) *blocks = t.lo_blocks;
    if (gated) *gated = t.lo_gated;
    return Q3_OK;
}

extern "C" q3_status q3_batcher_ticket_silence_read(q3_batcher* b, int64_t ticket, int64_t* n_in, int64_t* n_out, int64_t* lead_cut, int64_t* pause_cut, int64_t* trail_cut) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_ticket_silence_read: null batcher");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_ticket_silence_read: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    if (t.out.sil_mB == 0) return set_err(Q3_INVALID_ARG, "q3_batcher_ticket_silence_read: ticket %lld has no silence step (q3_batcher_ticket_silence)", (long long)ticket);
    std::lock_guard<std::mutex> g(b->dec->mu);
    if (n_in) *n_in = t.si[0];
    if (n_out) *n_out = t.si[1];
    if (lead_cut) *lead_cut = t.si[2];
    if (pause_cut) *pause_cut = t.si[3];
    if (trail_cut) *trail_cut = t.si[4];
    return Q3_OK;
}

extern "C" q3_status q3_batcher_read_out(q3_batcher* b, int64_t ticket, void* out_host, size_t cap_samples, size_t* n_samples, int* done) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_read_out: null batcher");
    if (!n_samples || !done || (cap_samples > 0 && !out_host)) return set_err(Q3_INVALID_ARG, "q3_batcher_read_out: null argument");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_read_out: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    if (!t.streamed) return set_err(Q3_INVALID_ARG, "q3_batcher_read_out: ticket %lld was not submitted as streamed (its samples come with q3_batcher_fetch)", (long long)ticket);
    if (t.out.plain()) return q3_batcher_read(b, ticket, (float*)out_host, cap_samples, n_samples, done);      // 24 kHz f32: the samples as they are
    *n_samples = 0; *done = 0;
    stream_settle(b, t, false);
    if (t.state == Q3_TICKET_FAILED) return set_err(t.st, "%s", t.err.c_str());
    std::lock_guard<std::mutex> g(b->dec->mu);
    const size_t sb = t.out.sample_bytes();
    size_t n = (t.sout.size() - t.o_read) / sb;
    if (n > cap_samples) n = cap_samples;
    if (n > 0) memcpy(out_host, t.sout.data() + t.o_read, n * sb);
    t.o_read += n * sb;
    *n_samples = n;
    *done = ((t.state == Q3_TICKET_DONE || t.state == Q3_TICKET_CANCELLED) && t.o_read == t.sout.size()) ? 1 : 0;
    return Q3_OK;
}

extern "C" q3_status q3_batcher_stream_info(q3_batcher* b, int* block_frames, size_t* block_bytes, int* blocks_total, int* blocks_in_use, int* blocks_peak) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_stream_info: null batcher");
    BatDecoder& d = *b->dec;
    std::lock_guard<std::mutex> g(d.mu);
    // the stream's own figures (q3_codec_stream_info after the last job); before the first stream job there is no stream: the
    // block size the batcher will ask for, and zeros
    if (block_frames) *block_frames = d.info_bf ? d.info_bf : b->s_block_frames;
    if (block_bytes) *block_bytes = d.info_bytes;
    if (blocks_total) *blocks_total = d.info_total;
    if (blocks_in_use) *blocks_in_use = d.info_use;
    if (blocks_peak) *blocks_peak = d.info_peak;
    return Q3_OK;
}


// ---- parking: the public calls (include/q3tts.h) ----
extern "C" q3_status q3_batcher_set_parking(q3_batcher* b, int max_parked, int quantum_frames, int fresh_first) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_set_parking: null batcher");
    if (b->steps > 0) return set_err(Q3_INVALID_ARG, "q3_batcher_set_parking: after the first q3_batcher_step (the decode worker's stream is sized for slots + max_parked rows)");
    if (max_parked < 0 || max_parked > 4096 || quantum_frames < 0) return set_err(Q3_INVALID_ARG, "q3_batcher_set_parking: max_parked must be 0..4096, quantum_frames >= 0");
    b->max_parked = max_parked; b->quantum = max_parked > 0 ? quantum_frames : 0; b->fresh_first = fresh_first != 0;
    b->srow_free.clear();
    for (int r = b->stream_rows() - 1; r >= 0; --r) b->srow_free.push_back(r);      // lowest row first (taken from the back)
    return Q3_OK;
}
extern "C" q3_status q3_batcher_park(q3_batcher* b, int64_t ticket) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_park: null batcher");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_park: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    if (t.state == Q3_TICKET_QUEUED) return set_err(Q3_INVALID_ARG, "q3_batcher_park: ticket %lld has not entered a row yet", (long long)ticket);
    if (t.state == Q3_TICKET_PARKED) { t.want_in = false; if (t.in_queue) { b->queue.erase(std::remove(b->queue.begin(), b->queue.end(), ticket), b->queue.end()); t.in_queue = false; } return Q3_OK; }      // the scheduler's park becomes the host's
    if (t.state != Q3_TICKET_RUNNING || t.row < 0) return Q3_OK;      // ended, or with the decode worker: nothing happens
    if ((int)b->parked.size() >= b->max_parked)
        return set_err(Q3_UNSUPPORTED, "q3_batcher_park: %d ticket(s) are parked already (max_parked, q3_batcher_set_parking)", (int)b->parked.size());
    return bat_park(b, t.row, true);
}
extern "C" q3_status q3_batcher_unpark(q3_batcher* b, int64_t ticket) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_unpark: null batcher");
    auto it = b->t.find(ticket);
    if (it == b->t.end()) return set_err(Q3_INVALID_ARG, "q3_batcher_unpark: unknown ticket %lld", (long long)ticket);
    BatTicket& t = *it->second;
    if (t.state != Q3_TICKET_PARKED) return Q3_OK;      // not parked (any more): nothing happens
    t.want_in = true;
    parked_requeue(b);
    return Q3_OK;
}
extern "C" q3_status q3_batcher_park_info(q3_batcher* b, int* n_parked, int* max_parked, long long* parks, long long* resumes, long long* moved, int* pages_parked) {
    if (!b) return set_err(Q3_INVALID_ARG, "q3_batcher_park_info: null batcher");
    if (n_parked) *n_parked = (int)b->parked.size();
    if (max_parked) *max_parked = b->max_parked;
    if (parks) *parks = b->n_parks;
    if (resumes) *resumes = b->n_resumes;
    if (moved) *moved = b->n_moved;
    if (pages_parked) { int n = 0; for (int64_t id : b->parked) n += parked_pages(b->t[id]->rec); *pages_parked = n; }
    return Q3_OK;
}
