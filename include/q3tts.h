/*
 * q3tts.h — C ABI of the MI355X-native Qwen3-TTS hot path (libq3tts.so, gfx950).
 *
 * This is the drop-in boundary for the reference's generation/session API: each entry point
 * names the reference interface (file:line, relative to the TrevorS/qwen3-tts-rs repo root) it
 * replaces. A Rust shim (`extern "C"` block) re-exposes the reference's
 * `Qwen3TTS` / `SynthesisOptions` / `StreamingSession` names on top of these symbols; the Python
 * mirror in qwen3_tts_rs_amd/api.py does the same over ctypes.
 *
 * Conventions: plain pointers and sizes only; every function returns q3_status (0 = OK) and
 * never throws/aborts across the ABI; `q3_last_error()` returns the thread-local message
 * (the reference's anyhow::Error text). All `*_host` pointers are host memory; device memory is
 * owned by the library (model arena, per-session KV pages) except where a function says
 * "device pointer". One process drives one GPU; the model handle is immutable after
 * q3_model_finalize and may be shared by any number of sessions on that GPU.
 */
#ifndef Q3TTS_H
#define Q3TTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Q3_ABI_VERSION 1
#define Q3_MAX_BATCH 64      /* sequences per session (rows of the decode GEMVs: 16-column MFMA tiles x 4) */

typedef enum q3_status {
    Q3_OK = 0,
    Q3_INVALID_ARG = 1,
    Q3_IO = 2,
    Q3_MISSING_WEIGHT = 3,   /* lib.rs:226-231, decoder_12hz.rs:176-181 ("Missing weight: ...") */
    Q3_KV_OVERFLOW = 4,      /* kv_cache.rs:293-300 */
    Q3_HIP_ERROR = 5,
    Q3_RCCL_ERROR = 6,
    Q3_UNSUPPORTED = 7,
    Q3_OOM = 8
} q3_status;

/* Shape constants parsed from config.json by the reference (config.rs:238-336 →
 * talker.rs:176-290 TalkerConfig, code_predictor.rs:48-113, decoder_12hz.rs:14-67). */
typedef struct q3_config {
    int32_t text_vocab;   /* 151936 */
    int32_t text_dim;     /* 2048 */
    int32_t hidden;       /* 2048 (1.7B) / 1024 (0.6B) */
    int32_t inter;        /* 6144 / 3072 */
    int32_t n_layers;     /* 28 */
    int32_t n_heads;      /* 16 */
    int32_t n_kv_heads;   /* 8 */
    int32_t head_dim;     /* 128 (only value supported by the gfx950 kernels) */
    int32_t codec_vocab;  /* 3072 */
    int32_t cp_hidden;    /* 1024 */
    int32_t cp_inter;     /* 3072 */
    int32_t cp_layers;    /* 5 */
    int32_t cp_heads;     /* 16 */
    int32_t cp_kv_heads;  /* 8 */
    int32_t cp_vocab;     /* 2048 */
    int32_t n_groups;     /* 16 */
    float   rms_eps;      /* 1e-6 */
    float   rope_theta;   /* 1e6 */
    int32_t dec_cb_dim;   /* 256 */
    int32_t dec_q_dim;    /* 512 */
    int32_t dec_latent;   /* 1024 */
    int32_t dec_hidden;   /* 512 */
    int32_t dec_layers;   /* 8 */
    int32_t dec_heads;    /* 16 */
    int32_t dec_head_dim; /* 64 */
    int32_t dec_inter;    /* 1024 */
    int32_t dec_cb_size;  /* 2048 */
    int32_t dec_dim;      /* 1536 */
    int32_t dec_up_ratios[2]; /* 2,2 */
    int32_t dec_up_rates[4];  /* 8,5,4,3 */
    float   dec_eps;      /* 1e-5 */
    float   dec_theta;    /* 1e4 */
} q3_config;

/* SynthesisOptions (lib.rs:1786-1836); f64 fields are f64 in the reference too. */
typedef struct q3_options {
    double   temperature;        /* 0.9 */
    double   top_p;              /* 0.9 */
    double   repetition_penalty; /* 1.05 */
    uint64_t seed;               /* used when has_seed != 0 */
    int32_t  max_length;         /* 2048  (max_new_tokens) */
    int32_t  top_k;              /* 50 */
    int32_t  eos_token_id;       /* 2150 (CODEC_EOS_TOKEN_ID, lib.rs:1466); -1 = None */
    int32_t  chunk_frames;       /* 10 */
    int32_t  min_new_tokens;     /* 2 */
    int32_t  has_seed;           /* 0 = None: seeded from the wall clock (sampling.rs:66-82) */
} q3_options;

enum { Q3_MODE_CUSTOM_VOICE = 0, Q3_MODE_VOICE_CLONE = 1, Q3_MODE_VOICE_DESIGN = 2 };
enum { Q3_DTYPE_F32 = 0, Q3_DTYPE_BF16 = 1 };

/* One utterance. Replaces the argument lists of synthesize_with_voice (lib.rs:718-724),
 * synthesize_voice_design (lib.rs:802-808) and the x-vector-only branch of
 * synthesize_voice_clone (lib.rs:897-951); token ids come from the caller's tokenizer
 * (text.rs:210-217 stays on the Rust side). */
typedef struct q3_request {
    int32_t mode;
    const uint32_t* text_ids;     int32_t n_text;
    const uint32_t* instruct_ids; int32_t n_instruct;  /* voice design: ChatML-framed instruct */
    uint32_t speaker_id;          /* Speaker::token_id (talker.rs:145-157) */
    uint32_t language_id;         /* Language::token_id (talker.rs:94-107) */
    const float* xvector;         /* [hidden] speaker embedding (voice clone) or NULL */
    q3_options opts;
    /* ICL voice clone (VoiceClonePrompt.ref_codes / ref_text_ids, lib.rs:127-134, 897-1046): reference codec
     * frames [n_ref][16] (from the caller's speech encoder) and the reference transcript's token ids. With
     * both present (mode = voice clone) the talker prefill is extended by the ICL block of
     * build_icl_prompt (talker.rs:646-710, streaming overlay), repetition_penalty is floored at 1.5 and
     * max_length capped at max(75, 6·n_text) (lib.rs:913-929).
     * ref_codes ALONE (with or without the transcript) already makes the full-utterance decode of a prefilled session
     * (q3_session_decode(b, 0, n_frames), q3_session_run) prepend the reference frames and cut their share of the samples
     * off again, as lib.rs:1022-1041 does for any prompt that carries codes; before q3_session_prefill (no frames, the
     * reference frames not yet on the device) the call decodes the empty range. */
    const uint32_t* ref_codes;    int32_t n_ref;
    const uint32_t* ref_text_ids; int32_t n_ref_text;
} q3_request;

/* SynthesisTiming (lib.rs:138-147) */
typedef struct q3_timing {
    double prefill_ms, generation_ms, decode_ms;
    int32_t generation_frames;
} q3_timing;

typedef struct q3_model q3_model;
typedef struct q3_session q3_session;

int         q3_abi_version(void);
const char* q3_last_error(void);
/* number of visible HIP devices, or -1 (replaces auto_device / parse_device, lib.rs:1854-1926) */
int         q3_device_count(void);

/* ---------------- model (Qwen3TTS::from_weights, lib.rs:267-368) ---------------- */
/* device = HIP device index; device = -1 creates a manifest-only handle (tensor names/shapes, no GPU) */
q3_status q3_model_create(const q3_config* cfg, int device, q3_model** out);
void      q3_model_free(q3_model* m);
/* Upload one checkpoint tensor under its safetensors name. `dtype` is the
 * SOURCE dtype; talker/code-predictor matrices are stored bf16 in HBM (the checkpoint's native
 * dtype, lib.rs:1394-1396), norms/biases and all decoder tensors f32 (lib.rs:344-353). */
q3_status q3_model_set_tensor(q3_model* m, const char* name, int dtype, const void* data_host, int64_t n);
/* the shape constants the handle was built with (talker.config(), talker.rs:843-846) */
q3_status q3_model_config(const q3_model* m, q3_config* out);
/* Names the model expects: i in [0, q3_model_n_tensors); returns name, element count, stored dtype */
int       q3_model_n_tensors(const q3_model* m);
q3_status q3_model_tensor_info(const q3_model* m, int i, const char** name, int64_t* n, int* stored_dtype);
/* Weight arena for the one data-parallel collective (RCCL broadcast from rank 0): device pointer
 * + size; after the broadcast non-root ranks call q3_model_mark_loaded then q3_model_finalize. */
q3_status q3_model_arena(q3_model* m, void** dev_ptr, size_t* bytes);
q3_status q3_model_mark_loaded(q3_model* m);
/* Paged talker KV. The reference allocates one cache per call, max_new_tokens + 256 positions long, and bails when it
 * overflows (kv_cache.rs:234-310, overflow :293-300; sized at lib.rs:450). Here every session of a model draws PAGES
 * (128 positions x every layer and KV head, K and V) from one pool per model as its rows grow, and returns them when a
 * row is replaced or the session ends: a 4k-position prompt and a ten-position prompt share the memory, and
 * q3_session_replace relinks the prefilled pages into the row instead of copying them.
 * q3_model_kv_pool_limit: the most pages the model's sessions may hold at once (0 = no limit but HBM); a session that
 * needs a page beyond it fails with Q3_KV_OVERFLOW before it runs (the reference's overflow bail). ONE budget covers f32 and
 * bf16 sessions (q3_session_set_kv_dtype): pages are counted in f32 equivalents, a bf16 page is half of one — the f32 pages a
 * bf16 session's prompt is prefilled into count in full until they are converted. The native batcher (q3_batcher_*) admits a
 * request only when its worst case (prompt + max_length) fits beside what the running rows may still take, so under a limit a
 * request waits in the queue instead of failing mid-generation; a request that cannot fit even alone fails on its ticket.
 * q3_model_kv_pool_info: page geometry and occupancy in f32-equivalent pages (any pointer may be NULL).
 * q3_model_kv_pool_trim: slabs (32 pages, ~1 GB at 28 layers x 8 KV heads) none of whose pages is held go back to the device;
 * the first f32 slab is allocated by q3_model_finalize so that it is not on the first request's time to first audio. */
q3_status q3_model_kv_pool_limit(q3_model* m, int max_pages);
q3_status q3_model_kv_pool_trim(q3_model* m, size_t* bytes_freed);
/* Vocoder arithmetic. The codec decoder's convs (decoder_block.rs:81-92, 240-247; F32 in the reference on every device)
 * run on the bf16 matrix cores with each f32 operand split into bf16 planes. planes = 3 (default): hi + mid + lo, six
 * products per multiply-accumulate — every f32 product exact, PCM within 2.5e-5 RMS of the reference CPU path.
 * planes = 2: hi + mid, three products — operands carry 16-17 mantissa bits (more than TF32's 11), PCM within 1e-4 RMS
 * (the path's tolerance is 1e-3), the 640-frame decode 20.6 -> 14.4 ms. Codec token ids never depend on it. Applies to
 * decodes started after the call; anything but 2 or 3 is Q3_INVALID_ARG. */
q3_status q3_model_set_codec_planes(q3_model* m, int planes);
q3_status q3_model_kv_pool_info(q3_model* m, int* page_positions, size_t* page_bytes, int* pages_total, int* pages_in_use, int* pages_peak);
/* Prefix cache (opt-in, off by default; no reference counterpart: the reference builds its KV cache per call, kv_cache.rs:234-310,
 * and prefills the whole VoiceDesign prompt [instruct N][role 3][codec 5][first text 1] every time, talker.rs:585-627). Under
 * causal attention the K/V of the instruct positions depend on the instruct tokens only, so the pages a prefill filled for them
 * are kept and LINKED into the rows of later requests with the same instruction: the prefill then starts at the first position
 * that is not cached. Blocks of 128 positions (one KV page), keyed by a chain hash over the token ids (ids stored and compared);
 * a lookup is a longest-prefix match in pages. A hit is invisible except in time: first logits, codes and PCM are bit for bit
 * those of the same request in the same session shape with the cache off.
 * q3_model_prefix_cache: capacity in pages; 0 = off, which also drops every cached page (one a running row holds stays that
 * row's). Cached pages are f32 pages of the model's pool and count against q3_model_kv_pool_limit once, however many rows share
 * them; loading weights again (q3_model_set_tensor, q3_model_mark_loaded, q3_model_finalize) drops every cached page; pages only the cache holds are given up (least recently used first) before a request fails with Q3_KV_OVERFLOW, and the
 * batcher's admission treats them as free. They pin their slabs against q3_model_kv_pool_trim until the cache is cleared.
 * Not used by debug / profiling sessions, with Q3_KV_CONTIGUOUS=1, for instructions shorter than one page, or for prompts that
 * are not VoiceDesign (ICL, x-vector, CustomVoice).
 * q3_model_prefix_cache_info: capacity, pages cached, how many of those a row holds too, and counters since the model was created
 * (lookups = eligible rows prefilled, hit_positions = prompt positions not computed again); any pointer may be NULL.
 * q3_session_prefix_info: positions of row b's prompt that came from the cache (after prefill; rows that entered through
 * q3_session_replace or the batcher report their own). */
q3_status q3_model_prefix_cache(q3_model* m, int max_pages);
q3_status q3_model_prefix_cache_info(q3_model* m, int* max_pages, int* pages_cached, int* pages_shared, long long* lookups,
                                     long long* hit_positions, long long* evictions);
q3_status q3_session_prefix_info(q3_session* s, int b, int* reused_positions);
/* Verify every tensor is present ("Missing weight: <name>"), derive codebooks
 * (decoder_12hz.rs:189-225) and RoPE tables. */
q3_status q3_model_finalize(q3_model* m);
/* Deterministic synthetic tensor generator (SURVEY.md Appendix B rules; host side, no GPU):
 * value_i = offset + scale * z_i, z ~ approx N(0,1) from a counter hash of (seed, name, i);
 * dtype BF16 writes uint16 (round-to-nearest-even), F32 writes float. */
q3_status q3_synth_fill(uint64_t seed, const char* name, int dtype, float scale, float offset,
                        int64_t n, void* out_host);

/* ---------------- session = one batch of utterances on one GPU ----------------
 * Owns KV pages, RNG streams, penalty masks (the fields of StreamingSession, lib.rs:1484-1508).
 * batch > 1 has no reference counterpart (reference batch = 1): every sequence behaves exactly
 * as its own batch-1 run. The sequences may be of ANY mix of prompt kinds and lengths (CustomVoice lib.rs:718-784,
 * VoiceDesign 802-870, x-vector / ICL voice clone 897-1046): rows of one prefill length are prefilled together (the text
 * length is free — it rides along as trailing text — so all CustomVoice requests share one batched prefill); a RAGGED
 * batch is prefilled in groups of equal prefill length by q3_session_prefill, each group on the side, and every row is then
 * moved into the session the way q3_session_replace does — decode runs in one captured frame graph over all rows. A
 * malformed request of a ragged batch is reported by q3_session_prefill (equal-length batches: by q3_session_create);
 * debug / profiling sessions (q3_session_set_debug) need rows of one prefill length.
 * Every request keeps its own q3_options — temperature, top-k / top-p, repetition penalty, min_new_tokens, EOS id, seed,
 * max_length: one sampler row per sequence on the device; only chunk_frames must be the same for all of them. */
q3_status q3_session_create(q3_model* m, const q3_request* reqs, int batch, q3_session** out);
/* The same with capacity for later arrivals (q3_session_replace): code buffers and the pre-drawn PCG streams are sized for
 * max(frame_budget, the largest max_length of `reqs`) frames per row, the KV extent of a row for
 * max(prompt_budget, the batch's prefill length) prompt positions + those frames. The rows of `reqs` behave exactly as
 * under q3_session_create (each ends at its own max_length). No reference counterpart (one utterance per call). */
q3_status q3_session_create_reserved(q3_model* m, const q3_request* reqs, int batch, int frame_budget, int prompt_budget,
                                     q3_session** out);
void      q3_session_free(q3_session* s);
/* prefill_custom_voice / _voice_clone / _voice_design + run_prefill_layers (talker.rs:451-627,
 * 823-841), build_trailing_text (lib.rs:508-519) and the first sampling decision
 * (lib.rs:558-571). */
q3_status q3_session_prefill(q3_session* s);
/* generate_codes frame loop (lib.rs:580-652): run up to n_frames more frames for every live
 * sequence; returns when they are done on the device. use_graph != 0: the frame is captured once
 * (hipGraph) and replayed per frame — as packets on the library's own AQL queue (the default;
 * q3_session_submit_info) or through hipGraphLaunch; 0: eager launches. Same kernels, same bits. */
q3_status q3_session_generate(q3_session* s, int n_frames, int use_graph);
/* frames emitted so far for sequence b (stops at the frame whose semantic token is EOS,
 * lib.rs:581-585) and whether it hit EOS / max_length */
q3_status q3_session_frames(q3_session* s, int b, int* n_frames, int* done);
/* gpu_frames_to_frame_codes (lib.rs:676-690): [n][16] u32, frame-major */
q3_status q3_session_codes(q3_session* s, int b, uint32_t* codes_host, int cap_frames, int* n_frames);
/* decode_codes over frames [f0, f1) of sequence b (lib.rs:881-890; streaming decodes each chunk
 * context-free, lib.rs:1755-1758): writes (f1-f0)*1920 f32 samples */
q3_status q3_session_decode(q3_session* s, int b, int f0, int f1, float* pcm_host, size_t cap, size_t* n_samples);
/* synthesize_with_timing (lib.rs:425-501) for the whole batch: prefill → generate → decode.
 * pcm_host[b] receives up to cap[b] samples (NULL = skip copy-out); n_samples[b] is set. */
q3_status q3_session_run(q3_session* s, int use_graph, float** pcm_host, const size_t* cap, size_t* n_samples,
                         q3_timing* timing);
/* StreamingSession::next_chunk (lib.rs:1650-1759) for sequence 0 of a batch-1 session: generates
 * up to chunk_frames frames, decodes them as an independent utterance; *done=1 with
 * *n_samples=0 when finished. */
q3_status q3_session_next_chunk(q3_session* s, float* pcm_host, size_t cap, size_t* n_samples, int* done);
/* The same for sequence b of a session with several sequences (one StreamingSession per row, lib.rs:1484-1541): the rows
 * advance in lockstep, so the first row asked generates the chunk's frames for all of them and the others only run their
 * vocoder. An error leaves the row's position untouched: the call can be repeated (lib.rs:1775-1781).
 * A row has ONE streaming position (frames already handed out), and every streaming entry follows it: q3_session_next_chunk,
 * q3_session_next_chunk_row, q3_session_next_chunks and q3_session_next_chunks_out may be mixed on a row, each continuing
 * where the last one stopped. q3_session_replace and q3_session_resume_row set the row's position back to frame 0. */
q3_status q3_session_next_chunk_row(q3_session* s, int b, float* pcm_host, size_t cap, size_t* n_samples, int* done);
/* q3_session_next_chunk_row for every row in one call: generates until every live row has a chunk (or ends, or is held by
 * open text), then decodes all rows' chunks together. pcm_host / cap / n_samples / done are arrays of one entry per row.
 * n_samples[b] = 0 with done[b] = 0 means "nothing yet" (held row), with done[b] = 1 "finished". Chunk boundaries and
 * samples are those of q3_session_next_chunk_row; in stream mode 1 the rows that are not ICL share one pass of a codec stream
 * the session owns (below), so a chunk costs O(chunk) and the launch count does not grow with the rows. */
q3_status q3_session_next_chunks(q3_session* s, float* const* pcm_host, const size_t* cap, size_t* n_samples, int* done);
/* Continuous batching: replace row b of a PREFILLED session — normally one whose sequence has ended (q3_session_frames:
 * done; fetch its codes / PCM first) — by a new request, which then starts at its frame 0 while the other rows go on. The
 * reference keeps all per-utterance state per call (KV caches, SamplingContext, penalty mask, trailing text:
 * lib.rs:743-756; StreamingSession lib.rs:1484-1541); here it is row b's slice of the session's device state, refilled
 * from a one-row prefill of `req`. The request carries its own q3_options — sampler settings, seed, EOS id, max_length
 * (SynthesisOptions is per call in the reference, lib.rs:1786-1836; only chunk_frames must equal the session's); it must
 * fit the row (max_length <= the session's largest; text rows <= max(1024, the longest of the original batch); prompt +
 * max_length within the row's KV extent). Any mode fits any session (an ICL request's repetition-penalty floor of 1.5,
 * lib.rs:1154-1160, is resolved into its own row). Each row of a session stops at its own opts.max_length;
 * q3_session_generate returns early once every row is done. Other rows are bit-for-bit unaffected. */
q3_status q3_session_replace(q3_session* s, int b, const q3_request* req);
/* Park and resume: a RUNNING row's state as an object (no reference counterpart: the reference runs one utterance per call to
 * its end). q3_session_park_row takes row b out of a prefilled session between two frames: the row's K/V pages (relinked, never
 * copied), its slice of every device array a frame reads before it writes (last hidden state, current token, penalty mask,
 * counters, pre-drawn PCG stream, frame limit, text state and trailing text rows, sampler record), its latest logits, the codes it
 * has committed and its host bookkeeping move into a record. The row is left idle — frozen, holding one zero-filled page of its
 * own — and may take a q3_session_replace or a record. The row may be live, held by open text or already ended; an idle row is
 * Q3_INVALID_ARG; a Q3_KV_CONTIGUOUS=1 session, a debug / profiling session and a row that has delivered chunks through
 * q3_session_next_chunk* are Q3_UNSUPPORTED; Q3_KV_OVERFLOW when the pool cannot give the vacated row its page, Q3_OOM when the
 * device refuses the record's block. Nothing changes when the call is REFUSED with one of these; a device error in the middle
 * (Q3_HIP_ERROR) leaves the session as unusable as any other failed launch does. The record's device state lives in one block
 * (a power of two from 64 KB on) from the session's own shelf of such blocks: a block is asked of the device only while the
 * session has never had as many records of that size parked at once, and goes back to the shelf at the resume or free.
 * q3_session_resume_row puts a record into row b of THE SAME session (another session's record: Q3_INVALID_ARG), any row that is
 * idle or has ended (a live row: Q3_INVALID_ARG). The row's own pages go back to the pool, the record's are linked, its text
 * moves to row b's slot. It consumes the record on success only; on failure the record is intact and the session unchanged.
 * For any schedule of parks and resumes, into any rows, a row's codes and PCM are those of the same session run without them,
 * and no other row's bits change. A row that sampled its EOS before it was parked resumes as ended: q3_session_frames reports
 * the same frame count and done = 1 (q3_parked_info: done), and the record's codes are the utterance's.
 * A record holds a reference on the model and may outlive its session; its pages stay charged to q3_model_kv_pool_limit until
 * q3_parked_free (which gives them back) or the resume. q3_parked_info: frames committed, the row's frame limit, whether it
 * had ended, pages held, bytes of device state (any pointer may be NULL). */
typedef struct q3_parked q3_parked;
q3_status q3_session_park_row(q3_session* s, int b, q3_parked** out);
q3_status q3_session_resume_row(q3_session* s, int b, q3_parked* p);
void      q3_parked_free(q3_parked* p);
q3_status q3_parked_info(const q3_parked* p, int* frames_committed, int* limit, int* done, int* kv_pages, size_t* state_bytes);
/* ---------------- continuous batcher: a queue of requests through the rows of one session ----------------
 * The serving loop around q3_session_replace, native: requests of any prompt kind, length and options are queued; a step
 * fills free rows from the queue, runs up to n_frames frames of the shared frame graph and collects the rows that ended.
 * No thread of its own — the host calls q3_batcher_step from its loop; calls may interleave freely, one thread at a time.
 * Each request's codes / PCM are those of its own batch-1 run (per-call state of the reference: lib.rs:743-756). No
 * reference counterpart (one utterance per call). */
typedef struct q3_batcher q3_batcher;
enum { Q3_TICKET_QUEUED = 0, Q3_TICKET_RUNNING = 1, Q3_TICKET_DONE = 2, Q3_TICKET_FAILED = 3 };
/* slots = rows of the session (1..64); frame_budget = largest max_length a request may ask for; prompt_budget = prefill
 * positions a row can hold (at least 16, which covers CustomVoice and x-vector prompts — their text rides along as trailing
 * text; VoiceDesign needs its instruct length + 16, ICL its reference frames + 16): see q3_session_create_reserved. The
 * session is opened lazily, on idle rows, when the first request arrives. */
q3_status q3_batcher_create(q3_model* m, int slots, int frame_budget, int prompt_budget, q3_batcher** out);
void      q3_batcher_free(q3_batcher* b);
/* Queue a request (deep copy: the caller's arrays may go away). want_pcm != 0: the finished row is vocoded
 * (the samples of q3_session_decode, ICL prompts included); else only its codes are kept. Since round 6 the vocoder of a
 * finished row runs on a worker thread and stream of the batcher while its row is refilled and the frames go on: the ticket
 * reads RUNNING until its samples have landed (q3_batcher_poll), and q3_batcher_fetch waits for them. */
q3_status q3_batcher_submit(q3_batcher* b, const q3_request* req, int want_pcm, int64_t* ticket);
/* One scheduling round. A request that cannot be placed (prompt or text longer than a row holds) fails alone: its ticket
 * carries the status and message. n_finished counts tickets whose generation ended (or that failed) in this call; with
 * want_pcm the samples of such a ticket may still be with the decode worker (it polls RUNNING until they land). A call
 * that returns n_running == 0 and n_queued == 0 has waited for the worker: every such ticket polls DONE afterwards. */
q3_status q3_batcher_step(q3_batcher* b, int n_frames, int use_graph, int* n_running, int* n_queued, int* n_finished);
/* state (Q3_TICKET_*); n_frames: frames of a finished ticket, frames run so far of a running one; n_samples: PCM samples held */
q3_status q3_batcher_poll(q3_batcher* b, int64_t ticket, int* state, int* n_frames, size_t* n_samples);
/* Copy a finished ticket's results out ([n_frames][16] u32; n_samples f32) and release it. A FAILED ticket returns its
 * status (message in q3_last_error) and is released too. */
q3_status q3_batcher_fetch(q3_batcher* b, int64_t ticket, uint32_t* codes_host, int cap_frames, float* pcm_host, size_t cap_samples);
/* Streamed tickets: the audio is delivered while the request runs. q3_batcher_submit_streamed queues like q3_batcher_submit
 * (rows of any prompt kind; an ICL request whose n_ref + max_length exceeds frame_budget + prompt_budget is Q3_UNSUPPORTED).
 * At the end of every q3_batcher_step the frames of that step go to the batcher's decode worker as ONE job over every streamed
 * row, which pushes them through a block-allocated codec stream (one stream row per slot, q3_codec_stream_create_blocked;
 * Q3_BAT_STREAM_BLOCK_FRAMES, default 128, and Q3_BAT_STREAM_MAX_BLOCKS, default 0 = no limit, are read by q3_batcher_create);
 * the step does not wait for it. The concatenation of what q3_batcher_read returns for a ticket is, bit for bit, the PCM the
 * same request gives with want_pcm = 1; its codes are the same too.
 * q3_batcher_read never blocks: it copies up to cap_samples (any count) of the ticket's samples that have landed and were not
 * read yet; *done = 1 once the ticket has finished and its last sample has been read (0 samples, done 0 before the first step).
 * An unknown ticket or one not submitted as streamed is Q3_INVALID_ARG; a FAILED ticket returns its status — a push the
 * stream refused (Q3_OOM under the block limit) or that failed fails the tickets it could not serve, each with its message,
 * and the others neither lose nor repeat a sample.
 * q3_batcher_fetch on a streamed ticket waits for its outstanding jobs, returns the codes and releases it (unread samples are
 * dropped); a non-null pcm_host is Q3_INVALID_ARG. q3_batcher_poll reports the samples that have landed.
 * q3_batcher_stream_info: the block figures of that stream as of the last job (q3_codec_stream_info). */
q3_status q3_batcher_submit_streamed(q3_batcher* b, const q3_request* req, int64_t* ticket);
q3_status q3_batcher_read(q3_batcher* b, int64_t ticket, float* pcm_host, size_t cap_samples, size_t* n_samples, int* done);
q3_status q3_batcher_stream_info(q3_batcher* b, int* block_frames, size_t* block_bytes, int* blocks_total, int* blocks_in_use, int* blocks_peak);
/* Open tickets: the text arrives in pieces while the request waits or speaks (streamed text in, beside the streamed audio out).
 * q3_batcher_submit_open queues like q3_batcher_submit / _submit_streamed, chosen by `want`, with the ticket's text open. The
 * request carries what q3_session_open_text asks for — at least one text token; an ICL request at least n_ref + 1 - n_ref_text
 * target tokens and a max_length within frame_budget —, else Q3_INVALID_ARG / Q3_UNSUPPORTED here. Admission under a page limit
 * counts prompt + max_length; an ICL ticket's length cap max(75, 6 n_text) is resolved when its text closes.
 * q3_batcher_append_text is host-only: it validates and records and never touches the device. The tokens become visible to the
 * frames, in arrival order, at the next FLUSH: at the start of every piece of q3_batcher_step, with no frame in flight, the
 * pending tokens of all running open tickets are projected together (groups of eight across rows, each through the one path of
 * q3_session_append_text: a token's row has the same bits) and published together, with one synchronisation. It works in every
 * state of the ticket: queued (the tokens are part of the request when its side session is created), staged on the prefill
 * worker (applied by the first flush after the row is entered) and running. last != 0 closes the text. After a close, or for a
 * ticket not submitted open: Q3_INVALID_ARG; text beyond the row's slot (prompt_budget + 1024 rows, one of them taken):
 * Q3_UNSUPPORTED, nothing of that call is taken and the ticket goes on; for a ticket that has ended: accepted and ignored.
 * A row whose text is exhausted is HELD: it keeps its slot, counts in n_running, and a step in which every row is
 * held replays no frame. For any feeding schedule a ticket's codes and PCM equal those of the closed request.
 * q3_batcher_text_state: the fields of q3_session_text_state (tokens the next flush will publish included); for a queued ticket
 * frames_committed is 0 and frames_runnable what its text allows.
 * q3_batcher_cancel gives a ticket's place back, synchronously (call it between steps). Queued: it leaves the queue. Running: its
 * row is collected with the frames it has committed and is free for the next step. The ticket reads Q3_TICKET_CANCELLED;
 * q3_batcher_fetch returns its [n][16] codes — with want_pcm their decode, the first n * 1920 samples of the full run — and
 * releases it; a streamed ticket's q3_batcher_read delivers every sample of the committed frames, then done = 1. DONE / FAILED /
 * CANCELLED tickets: Q3_OK, nothing happens; an unknown ticket: Q3_INVALID_ARG. The other rows keep their bits. */
enum { Q3_TICKET_CANCELLED = 4 };
enum { Q3_WANT_CODES = 0, Q3_WANT_PCM = 1, Q3_WANT_STREAM = 2 };
q3_status q3_batcher_submit_open(q3_batcher* b, const q3_request* req, int want, int64_t* ticket);
q3_status q3_batcher_append_text(q3_batcher* b, int64_t ticket, const uint32_t* ids, int n, int last);
q3_status q3_batcher_text_state(q3_batcher* b, int64_t ticket, int* n_text, int* frames_committed, int* frames_runnable, int* closed);
q3_status q3_batcher_cancel(q3_batcher* b, int64_t ticket);
/* Parked tickets (opt-in; no reference counterpart): more requests in flight than rows. A running ticket's row goes into a record
 * (q3_session_park_row) and the row is free for another ticket; the parked ticket re-enters ANY free row later by
 * q3_session_resume_row and goes on where it stopped. For any schedule a ticket's codes, PCM and streamed bytes are those of the
 * same request run to completion in one row.
 * q3_batcher_set_parking, before the first q3_batcher_step (Q3_INVALID_ARG after): max_parked = 0 (the default) is the batcher
 * without parking — no entry point changes its behaviour, bits or timing. quantum_frames = 0: only explicit parks.
 * quantum_frames > 0, the TIME SLICE: at the start of every piece of a step, while something waits, no row is free and fewer than
 * max_parked tickets are parked, the running ticket that has committed the most frames since it entered its row is parked if
 * that is at least quantum_frames (ties: the lowest row; a row HELD by open text counts as having used its quantum and goes
 * first), and the head of the waiting list takes its row; a ticket parked by one such round is not resumed by the same round.
 * Pieces are also cut where the next quantum ends while something waits. The policy reads no clock: it is a function of
 * submissions, steps and frames. ONE waiting list holds fresh tickets and parked tickets that want a row: with fresh_first = 0
 * in order of arrival / park time; with fresh_first != 0 a fresh ticket stands ahead of the parked ones, behind earlier fresh
 * ones. A ticket the scheduler parked waits at once; a parked OPEN ticket waits only while its text allows another frame or is
 * closed (text appended meanwhile is recorded and published by the first flush after it re-enters).
 * q3_batcher_park (between steps, like q3_batcher_cancel): a ticket RUNNING in a row reads Q3_TICKET_PARKED and stays parked
 * until q3_batcher_unpark, which puts it on the waiting list. A ticket that has ended or is with the decode worker: Q3_OK,
 * nothing happens; a queued one: Q3_INVALID_ARG; with max_parked tickets parked already: Q3_UNSUPPORTED, nothing changes.
 * q3_batcher_poll reports a parked ticket's committed frames; q3_batcher_cancel gives its codes (their decode with want_pcm, the
 * last part of a streamed ticket) out of the record and frees it; q3_batcher_free frees what is still parked. A streamed
 * ticket's row of the decode worker's codec stream and output stage follows the ticket (slots + max_parked rows; blocks are
 * taken on demand). Under a page limit a parked ticket keeps its admission claim, exactly as if it still sat in its row, and the
 * row it left holds one page like any idle row. A request that does not fit beside the claims WAITS while a row runs or a parked
 * ticket wants a row (a parked ticket passes it: it needs no admission); beside tickets the host holds parked and nothing else
 * it fails on its ticket with Q3_KV_OVERFLOW, as a request that cannot fit does today — unpark first, or raise the limit.
 * n_running of q3_batcher_step keeps counting rows; parked tickets that want a row count in n_queued (a host loop that stops on
 * running == 0 && queued == 0 does not stop while they wait); q3_batcher_park_info gives the parked count, the limit, parks,
 * resumes, resumes into another row than the one left, and the K/V pages the records hold (any pointer may be NULL). */
enum { Q3_TICKET_PARKED = 5 };
q3_status q3_batcher_set_parking(q3_batcher* b, int max_parked, int quantum_frames, int fresh_first);
q3_status q3_batcher_park(q3_batcher* b, int64_t ticket);
q3_status q3_batcher_unpark(q3_batcher* b, int64_t ticket);
q3_status q3_batcher_park_info(q3_batcher* b, int* n_parked, int* max_parked, long long* parks, long long* resumes, long long* moved,
                               int* pages_parked);

/* Chunk decode mode of q3_session_next_chunk. 0 (default) = each chunk decoded as an independent utterance, exactly
 * as the reference does (lib.rs:1755-1758: audible seams, every chunk restarts from zero padding). 1 = continuous:
 * the vocoder's front runs over all frames so far and its convolutional stack over the chunk plus 12 frames of left
 * context, so the concatenated chunks are sample-identical to the non-streaming decode (SURVEY.md §8(f) rank 1,
 * "improved overlap mode"). */
q3_status q3_session_set_stream_mode(q3_session* s, int mode);

/* ---------------- streaming text input: a row's text arrives while it speaks ----------------
 * Qwen3-TTS reads its text one token per frame after the prefill ("trailing text", lib.rs:508-519, 613-619): frame f of a row
 * depends on the text only through trailing token f. A row OPENED before q3_session_prefill takes the rest of its text in pieces
 * (q3_session_append_text); a frame whose trailing token has not arrived yet is not committed — the row is HELD in it (no
 * token, counter or state of the row moves) while the other rows go on — and runs as if it had never waited once the token is
 * there. tts_eos, then tts_pad follow the append that closes the text (last != 0). For any feeding schedule an open row's codes
 * and PCM equal those of the same request with its whole text. q3_session_generate never replays a frame in which
 * no row can commit; q3_session_next_chunk / _row return *n_samples = 0, *done = 0 while a whole chunk is not possible yet;
 * q3_session_run refuses a session with an open row. q3_session_prefill_len / Q3_GET_TRAILING report the trailing rows present.
 * No reference counterpart (the reference takes the whole text per call). */
/* Open row b: before q3_session_prefill, not in a ragged first batch nor a debug / profiling session. The request must carry at
 * least one text token (the prefill consumes it); an ICL request at least n_ref + 1 - n_ref_text, and a max_length within the
 * session's frame budget (its length cap max(75, 6 n_text) is resolved when the text closes). */
q3_status q3_session_open_text(q3_session* s, int b);
/* Append n text tokens to open row b; last != 0 closes its text. Waits for the session's frames in flight, projects the tokens on
 * the session stream (one fixed path: a token's row does not depend on how it was fed) and publishes them. Text beyond the row's
 * slot (1024 rows, or the session's prompt budget + 1024) is refused with Q3_UNSUPPORTED; an append after the close with
 * Q3_INVALID_ARG; appends to a row that has ended (EOS / max_length) are accepted and ignored. */
q3_status q3_session_append_text(q3_session* s, int b, const uint32_t* ids, int n, int last);
/* Row b: text tokens received (n_text), frames committed, frames it can still commit with the text it has (0 when held or
 * done), whether its text is closed; frames_replayed = frames the session has replayed, all rows. Any pointer may be NULL. */
q3_status q3_session_text_state(q3_session* s, int b, int* n_text, int* frames_committed, int* frames_runnable, int* closed,
                                int* frames_replayed);

/* ---------------- stage-level entry points (parity tests; the reference's
 * tests/reference_validation.rs stages) ---------------- */
enum {
    Q3_GET_PREFILL_EMBEDS = 0,  /* [prefill_len][hidden] f32 */
    Q3_GET_LAST_HIDDEN = 1,     /* [hidden] normed last hidden (talker.rs:729-735) */
    Q3_GET_LOGITS = 2,          /* [codec_vocab] raw logits of the latest talker step */
    Q3_GET_TRAILING = 3,        /* [T_tr][hidden] */
    Q3_GET_PAD_EMBED = 4,       /* [hidden] */
    Q3_GET_LOGITS_HIST = 5,     /* [frames+1][codec_vocab] (session created with debug capture) */
    Q3_GET_CP_LOGITS = 6,       /* [15][cp_vocab] of the latest code-predictor run */
    Q3_GET_TOKEN = 7,           /* u32 current semantic token */
    Q3_GET_CP_LOGITS_HIST = 8   /* [frames][15][cp_vocab] (debug capture) */
};
/* K/V dtype of the talker cache, before q3_session_prefill: Q3_DTYPE_F32 (default — the parity contract is the reference's CPU
 * F32 path) or Q3_DTYPE_BF16, the dtype of the reference GPU path's cache (kv_cache.rs:234-310; KVCache::new(..., dtype) at
 * lib.rs:450): the prompt is prefilled in f32 and converted once, decode steps append and read bf16 — half the K/V bytes per
 * frame; results are no longer bit-comparable with the F32 oracle. Needs the paged cache. */
q3_status q3_session_set_kv_dtype(q3_session* s, int dtype);
q3_status q3_session_set_debug(q3_session* s, int capture_logits);
q3_status q3_session_prefill_len(q3_session* s, int b, int* prefill_len, int* trailing_len);
q3_status q3_session_get(q3_session* s, int what, int b, void* out_host, size_t bytes);
/* generate_step_with_embed (talker.rs:716-736), teacher-forced: embeds_host [batch][hidden] */
q3_status q3_talker_step(q3_session* s, const float* embeds_host, float* hidden_host, float* logits_host);
/* generate_acoustic_codes (code_predictor.rs:320-416), teacher-forced: inputs [batch][hidden] */
q3_status q3_cp_generate(q3_session* s, const float* last_hidden_host, const float* sem_embed_host,
                         uint32_t* codes15_host, float* cp_logits_host /*[batch][15][cp_vocab] or NULL*/);
/* lib.rs:612-622 frame glue: sem + ((e0+e1)+..+e14) + text_add → [hidden] */
q3_status q3_frame_embed(q3_model* m, uint32_t sem_token, const uint32_t* codes15, const float* text_add_host,
                         float* out_host);
/* apply_generation_penalties_gpu + sample (lib.rs:1271-1322; sampling.rs:140-319) on device for
 * `rows` independent rows: logits_host [rows][vocab], seen_host [rows][vocab] u8 (may be NULL),
 * u_host [rows] uniform draws (SamplingContext::rand_f32) → tokens_host [rows] */
q3_status q3_sample(int device, const float* logits_host, const uint8_t* seen_host, const float* u_host,
                    int rows, int vocab, const q3_options* opts, int token_count, uint32_t* tokens_host);
/* PCG-XSH-RR stream of SamplingContext (sampling.rs:32-51, 84-94); host side */
void      q3_rng_seed(uint64_t seed, uint64_t* state);
float     q3_rng_next(uint64_t* state);
/* FusedRmsNorm::forward_residual (fused_ops.rs:49-96; kernels/fused_residual_rmsnorm.cu:39-90):
 * returns (rms_norm(x+res)*w, x+res); dtype F32 or BF16 (storage), f32 math */
q3_status q3_fused_residual_rmsnorm(int device, int dtype, const void* x_host, const void* res_host,
                                    const void* w_host, int rows, int cols, float eps,
                                    void* normed_host, void* sum_host);
/* y = x·Wᵀ (+b) with bf16 weights / f32 activations — the GEMV family used by every projection
 * (candle Linear, transformer.rs:224-227): x [M][K] f32, w [N][K] bf16 */
q3_status q3_linear(int device, const float* x_host, const uint16_t* w_bf16_host, const float* bias_host,
                    int M, int N, int K, float* y_host);
/* Test API: ONE launch of the GEMV family with every argument of the engine's dispatcher spelled out. All arrays are host
 * arrays. x [M][ldx] (ldx >= K, ldx % 4 == 0); w / w2 row-major bf16 [N][K] (w2: the SwiGLU "up" matrix, else NULL);
 * bias [N], norm_w [K] (fused input RMSNorm with eps) and resid [M][ldr] may be NULL; epi 0 none / 1 + resid / 2 SiLU /
 * 3 SwiGLU; tiled -1 = the engine's choice, 1 = 16-row tiles, 2 = 4-row tiles, 0 = row-major first-generation kernel;
 * ksplit 1, or 2 = the K range over two workgroups (the entry zeroes the M x N result first); use_ws != 0 and M > 16: the
 * wide-session GEMM's workspace is passed. y [M_alloc][ldy] (M_alloc >= M, ldy >= N) is uploaded whole before the launch and
 * copied back whole after it, so the caller sees what lies around the result. zero_n > 0 (% 4 == 0): zero_buf
 * [zero_n + zero_guard] is uploaded, its first zero_n floats are the launch's clearing side job, and it is copied back.
 * A launch the dispatcher refuses returns Q3_UNSUPPORTED (never another kernel) and leaves y / zero_buf as they were. */
typedef struct q3_linear_ex_args {
    int M, N, K, ldx, ldy, ldr, M_alloc;
    int epi, tiled, ksplit, use_ws, zero_n, zero_guard;
    float eps;
    const float* x; const uint16_t* w; const uint16_t* w2;
    const float* bias; const float* norm_w; const float* resid;
    float* y; float* zero_buf;
} q3_linear_ex_args;
q3_status q3_linear_ex(int device, const q3_linear_ex_args* args);
/* Test API: one decode-attention step (per-head q/k RMSNorm, rotate-half RoPE at pos, K/V append, GQA attention) over a
 * contiguous cache. variant 0 = the one-launch kernel (+ the split merge when n_splits > 1), 1 = the three-launch path,
 * 2 = the code predictor's kernel (every pos equal, < 16; n_splits 1; Q3_UNSUPPORTED otherwise). pos [B]; qkv
 * [B][(nh + 2 nkv) * 128]; q_norm_w / k_norm_w [128]; rope_cos / rope_sin [max_seq][64]; kcache / vcache
 * [B][nkv][max_seq][128] in and out; out [B][nh * 128]. nh / nkv is 1, 2 or 4; n_splits <= 64. */
typedef struct q3_attn_step_args {
    int variant, B, nh, nkv, n_splits, max_seq;
    float eps; int reserved;
    const int* pos; const float* qkv; const float* q_norm_w; const float* k_norm_w;
    const float* rope_cos; const float* rope_sin;
    float* kcache; float* vcache; float* out;
} q3_attn_step_args;
q3_status q3_attn_step(int device, const q3_attn_step_args* args);
/* Test API: one decode-attention step in the forms a session runs (tests/test_gpu_attention_forms.py). variant 0 =
 * launch_attn_fused (+ launch_attn_merge when n_splits > 1), 1 = launch_qknorm_rope_kv + launch_attn_decode + launch_attn_merge,
 * 2 = launch_attn_cp, 3 = launch_attn_first2. layout 0 = one contiguous f32 cache, 1 = f32 pages, 2 = bf16 pages (variant 0 only;
 * every cache value must be exact in bf16). The caller always passes and receives the LOGICAL cache of the selected layer,
 * kcache / vcache [n_seq][nkv][max_seq][128] f32. For a paged layout the entry builds n_slabs (1, 2) slabs of KvPool's geometry
 * for n_layers (1..4) layers, fills all of them with a pattern, scatters the cache into the pages page_slots [n_seq][ceil(max_seq
 * / 128)] names (slots 0 .. 32 n_slabs - 1, each at most once) under each page's row rotation, runs the step on layer `layer`
 * with kv_row_pages as given (1..8 and >= the pages of max_seq: the scalar table form; 0 or 9..64: one entry per lane), gathers
 * the cache back and reports in stray[0] how many elements outside the gathered rows no longer hold the pattern, in stray[1] the
 * offset of the first (-1: none); rot_used [n_seq][pages][nkv] receives the rotations. B counts rows, n_seq = B / rows_per_seq
 * sequences; pos [n_seq] is a sequence's base position. rows_per_seq 1..8 with variant 1, exactly 2 (pos 0) with variant 3, else 1.
 * Sources of q|k|v: qkv [B][(nh + 2 nkv) * 128]; or (variants 0, 2) the K-slice sums qkv_part [qkv_S][B][ld_qkv] with qkv_ssq
 * [qkv_S][B], qkv_S 1..8, qkv_K, qkv_eps; or the folded gather: g_logits [B][g_vocab] (variants 0, 2: the row is the first
 * maximum) or g_tok [n_seq] (variant 3: row 1 of a sequence) naming a row of g_qkv_tab [g_vocab][ld_qkv] and g_proj_tab
 * [g_vocab][g_proj_dim], which is copied to g_x [B or n_seq][g_ldx] (in and out); variants 0 and 2 record the row in g_codes
 * [B][g_max_frames][16] (in and out) at [g_frame_idx[b]][g_code_slot] while g_frame_idx[b] < g_max_frames. qkv may be NULL where
 * no row is read from it. zero_buf [zero_n + zero_guard] (in and out, zero_n % 4 == 0; variants 0, 2, 3): the zero side job.
 * Everything the kernels cannot address is refused before a device is touched (Q3_INVALID_ARG / Q3_UNSUPPORTED). */
typedef struct q3_attn_step_ex_args {
    int variant, layout, B, nh, nkv, n_splits, max_seq, rows_per_seq;
    int n_layers, layer, n_slabs, kv_row_pages;
    int qkv_S, qkv_K, g_vocab, g_proj_dim, g_ldx, g_max_frames, g_code_slot, zero_n, zero_guard;
    float eps, qkv_eps; int reserved;
    const int* pos; const float* qkv; const float* q_norm_w; const float* k_norm_w;
    const float* rope_cos; const float* rope_sin;
    float* kcache; float* vcache; float* out;
    const int* page_slots; int* rot_used; long long* stray;
    const float* qkv_part; const float* qkv_ssq;
    const float* g_logits; const uint32_t* g_tok; const float* g_qkv_tab; const float* g_proj_tab;
    float* g_x; uint32_t* g_codes; const int* g_frame_idx;
    float* zero_buf;
} q3_attn_step_ex_args;
q3_status q3_attn_step_ex(int device, const q3_attn_step_ex_args* args);
/* Test API: launch_kv_pages_to_bf16 over n_pages (1..32) pages of n_layers (1..4) layers and nkv kv heads: src [n_pages]
 * [n_layers][2 (K, V)][nkv][128][128] f32 is scattered into slots src_slots [n_pages] of a pattern-filled f32 slab, converted
 * into slots dst_slots [n_pages] of a pattern-filled bf16 slab (both of KvPool's geometry; slots 0..31, each at most once per
 * list) and gathered into dst (uint16, the same shape). stray as in q3_attn_step_ex, over the destination slab; rot_used
 * [2 (src, dst)][n_pages][nkv]. */
q3_status q3_kv_pages_to_bf16_ex(int device, int n_layers, int nkv, int n_pages, const int* src_slots, const int* dst_slots,
                                 const float* src, uint16_t* dst, int* rot_used, long long* stray);
/* Test API: which kernel instance the vocoder conv family runs for a shape — the launchers' own decision function, no GPU
 * needed. Returns a ConvPath code: low 5 bits the kernel (0 refused, 1 k_conv_out1, 2 k_conv_out1_v4, 3 / 4 k_lin_small_bf16x3
 * <4 | 8>, 5..11 the k_conv_bf16x3 geometries 96x128 T_M=4 / 4 waves x 32x128 / 4 waves x 32x256 / 64x128 / 64x64 / 128x128 /
 * 96x128 six waves, 12 / 13 k_conv1d_mfma<CO_W = 2 | 1>, 14 k_conv1d, 15 / 16 k_resunit_bf16x3<3 | 6>), then flags 32 PRE, 64 SEG,
 * 128 CIS = 128, 256 NP = 2. phases > 1: the polyphase transposed conv (k = taps, dil = 1). q3_conv_path_name: the code as text
 * (thread-local buffer). q3_resunit_path: launch_resunit's acceptance rule (0 = refused: the caller runs the two convs). Both
 * answer 0 for L above 2^30, q3_conv_path also for a dilation beyond +-2^16. */
int         q3_conv_path(int cout, int cin, int L, int k, int dil, int phases, int packed, int has_resid, int planes, int aligned16);
int         q3_resunit_path(int C, int L, int dil, int packed, int ya_is_xa, int planes);
const char* q3_conv_path_name(int code);
/* Test API: ONE launch of the vocoder conv family over host arrays ([C][L] f32, time contiguous).
 * kind 0 = launch_conv1d (causal, left zero padding): x [cin][L], w [cout][cin][k], optional b [cout], snake_a / snake_b [cin]
 *   (SnakeBeta on load), resid [cout][L] (or resid_in_place != 0: the residual is y itself, as the residual units use it), scale
 *   [cout], act 0..6, post_a / post_ib [cout] (SnakeBeta on the output), y2 (raw in y, activated in y2).
 * kind 1 = launch_transconv1d_taps: w in the checkpoint layout [cin][cout][k], k = stride * taps; output [cout][L * stride].
 * kind 2 = launch_resunit: y += conv1x1(snake_mid(conv7_dil(x) + b)) + b2 in place, y2 = snake_post(y); w [C][C][7], w2 [C][C],
 *   mid_a / mid_ib [C]; cin = cout = C; y2_is_x != 0 passes the operand as the activated output (refused).
 * packed != 0: the entry packs the weights (launch_pack_conv_w, per phase for kind 1) and passes them; else the f32 kernels run.
 * snake_raw != 0: the snake pairs are (alpha, beta) and the entry builds each (a, 1/b) table with launch_snake_tables first.
 * y and y2 are host buffers of y_elems floats whose result starts y_front floats in (y_front % 4 == 0): both are uploaded whole
 * before the launch and copied back whole after it, guards included. *path (optional) receives the ConvPath code of the launch.
 * A launch the dispatcher refuses returns Q3_UNSUPPORTED (never another kernel) and leaves y / y2 as they were. */
typedef struct q3_conv_ex_args {
    int kind, cin, cout, L, k, dil, stride;
    int act, planes, packed, resid_in_place, snake_raw, y2_is_x;
    int y_front, y_elems;
    int* path;
    const float* x; const float* w; const float* b;
    const float* snake_a; const float* snake_b; const float* resid; const float* scale;
    const float* post_a; const float* post_ib;
    const float* w2; const float* b2; const float* mid_a; const float* mid_ib;
    float* y; float* y2;
} q3_conv_ex_args;
q3_status q3_conv_ex(int device, const q3_conv_ex_args* args);
/* Test API: q3_conv_ex under a residency cap — at most `resident` workgroups of the launch per CU (0 = none: q3_conv_ex itself),
 * the cap the session's overlapped decode puts on the vocoder launches that run beside the frame loop (Q3_DECODE_RESIDENT). The cap
 * is padding of the launch's dynamic LDS; the kernels and their results are the same. *lds_bytes (optional) receives the dynamic
 * LDS the launch asked for. Q3_UNSUPPORTED for a shape whose kernel has only static LDS (nothing to cap). */
q3_status q3_test_conv_resident(int device, const q3_conv_ex_args* args, int resident, int* lds_bytes);
/* Test API: which geometry launch_lm_gemm (the long-prompt prefill GEMM) picks for a shape — the launcher's own decision function,
 * no GPU needed. norm / w2 / planes != 0: a fused input RMSNorm, a second (SwiGLU "up") matrix, pre-split activation planes with
 * the split-K workspace q3_gemm_ex passes. Returns the geometry (0 = geometry 1 with the split in the kernel, 1 = geometry 1 over
 * planes, 2 = k_lm_gemm2, 3 = k_lm_gemm3) or -1 for arguments the launcher refuses (and for M, N or K above 2^24); path (optional) [4] =
 * geometry, k_ranges, k_split, n_split. */
int q3_gemm_path(int M, int N, int K, int epi, int norm, int w2, int planes, int* path);
/* Test API: ONE launch_lm_gemm call over host arrays. x [M][ldx]; w / w2 row-major bf16 [N][K] (retiled as the loader does);
 * bias [N], norm_w [K] (the entry runs launch_row_den first) and resid [M][ldr] may be NULL; epi as in q3_linear_ex. geometry -1 =
 * the engine's pick over planes, 0 = geometry 1 with the split in the kernel (no planes), 1 / 2 / 3 = that geometry over planes
 * (launch_split_rows into a NaN-filled buffer of whole 128-row tiles). k_split 0 = the engine's, else forced (geometry 3; the
 * split-K workspace is NaN-filled); sup_m, sup_n 0 = the engine's, else the forced super-tile. y [M_alloc][ldy] is uploaded whole
 * before the launch and copied back whole after it. path (optional) [4] = what ran: geometry, k_ranges, k_split, n_split.
 * A launch the dispatcher refuses returns Q3_UNSUPPORTED (never another geometry) and leaves y as it was. */
typedef struct q3_gemm_ex_args {
    int M, N, K, ldx, ldy, ldr, M_alloc;
    int epi, geometry, k_split, sup_m, sup_n;
    float eps;
    int* path;
    const float* x; const uint16_t* w; const uint16_t* w2;
    const float* bias; const float* norm_w; const float* resid;
    float* y;
} q3_gemm_ex_args;
q3_status q3_gemm_ex(int device, const q3_gemm_ex_args* args);
/* Test API: which prefill attention kernel launch_attn_prefill picks (0 = VALU, 8 query rows per workgroup; 1 = S = Q.K^T on the
 * f32 matrix cores; 2 = the transposed product; 3 = bf16x3 planes) for heads / kv heads, with or without K/V planes, over 1 or 2
 * key halves. No GPU needed. Returns the kernel or -1 (refused); path (optional) [2] = kernel, halves. */
int q3_attn_prefill_path(int nh, int nkv, int use_planes, int halves, int* path);
/* Test API: one prefill attention step over a contiguous cache: n_seq sequences of rps rows at positions base_pos .. base_pos +
 * rps - 1. launch_qknorm_rope_kv, launch_kv_planes (bf16x3 kernel only; NaN-filled buffer, more tiles allocated than used), ONE
 * launch_attn_prefill, launch_attn_merge for two halves. qkv [n_seq * rps][ld_qkv]; q_norm_w / k_norm_w [128]; rope_cos / rope_sin
 * [max_seq][64]; kcache / vcache [n_seq][nkv][max_seq][128] in and out; out [n_seq * rps][ld_out] is uploaded whole and copied
 * back whole. kernel -1 = the engine's pick (use_planes != 0: with K/V planes), 0..3 as q3_attn_prefill_path; halves 1 or 2.
 * path (optional) [2] = kernel, halves that ran. A refused launch returns Q3_UNSUPPORTED and leaves the caches and out alone.
 * max_seq <= 2^20 and base_pos + rps <= max_seq, else Q3_INVALID_ARG.
 * The trailing fields select the cache layout; all zero = the contiguous form above. layout 1 = f32 pages (what prefill_gemm runs
 * on by default): kcache / vcache stay the LOGICAL cache of the selected layer, and the entry builds n_slabs (1, 2) slabs of
 * KvPool's geometry for n_layers (1..4) layers as q3_attn_step_ex does — pattern-filled, the cache scattered into the pages
 * page_slots [n_seq][ceil(max_seq / 128)] names under each page's row rotation, the page table between two slabs, table entries
 * beyond a row's pages naming its first — runs the same launches on layer `layer`, gathers the cache back and reports stray /
 * rot_used [n_seq][pages][nkv] as there. max_seq <= 64 * 128. Slots are 0 .. 32 n_slabs - 1 and distinct, except that page i of
 * several sequences may name ONE slot (a shared prefix page) when (i + 1) * 128 <= base_pos and those sequences' cache rows of
 * the page are bit-equal. layout 2 (bf16 pages) is Q3_UNSUPPORTED: prefill never runs on them. Every argument, the slots and the
 * sharing rule included, is checked before a device is touched (Q3_INVALID_ARG). */
typedef struct q3_attn_prefill_ex_args {
    int n_seq, rps, base_pos, nh, nkv, max_seq, ld_qkv, ld_out;
    int kernel, halves, use_planes;
    float eps;
    int* path;
    const float* qkv; const float* q_norm_w; const float* k_norm_w;
    const float* rope_cos; const float* rope_sin;
    float* kcache; float* vcache; float* out;
    int layout, n_layers, layer, n_slabs;
    const int* page_slots; int* rot_used; long long* stray;
} q3_attn_prefill_ex_args;
q3_status q3_attn_prefill_ex(int device, const q3_attn_prefill_ex_args* args);
/* Test API: the PACKED sibling of q3_attn_prefill_ex (a ragged first batch's packed prefill pass): n_seq sequences of seq_len[i]
 * rows (1 .. 8192 each, at most 16384 together), every one from position 0, laid end to end: qkv [sum(seq_len)][ld_qkv] and out
 * [sum(seq_len)][ld_out] in pack order. It runs the packed q/k-norm + RoPE + K/V-append launch, the packed K/V plane split where a
 * sequence takes the bf16x3 kernel (NaN-filled buffer, two spare tiles behind the last), and ONE packed attention launch per
 * kernel present — nothing else. kernel -1 = per sequence the kernel its length selects when prefilled alone (below 256 rows the
 * transposed f32-MFMA kernel, else bf16x3: possibly two launches), 2 = the transposed f32-MFMA kernel for all, 3 = bf16x3 for all.
 * No key halves. kcache / vcache [n_seq][nkv][max_seq][128] (max_seq >= every seq_len), rope tables [max_seq][64], layouts 0 and 1,
 * page_slots / rot_used / stray as q3_attn_prefill_ex (no slot may be shared: every sequence starts at 0). path (optional) [2] =
 * launches of the f32-MFMA kernel, of the bf16x3 kernel (0 / 1 each). plane_tail (optional) [2] = bytes of the plane buffer behind
 * the last sequence's tiles that are still NaN fill, bytes there in all. Every argument is checked before a device is touched. */
typedef struct q3_attn_prefill_packed_ex_args {
    int n_seq, nh, nkv, max_seq, ld_qkv, ld_out;
    int kernel;
    float eps;
    const int* seq_len;
    int* path; long long* plane_tail;
    const float* qkv; const float* q_norm_w; const float* k_norm_w;
    const float* rope_cos; const float* rope_sin;
    float* kcache; float* vcache; float* out;
    int layout, n_layers, layer, n_slabs;
    const int* page_slots; int* rot_used; long long* stray;
} q3_attn_prefill_packed_ex_args;
q3_status q3_attn_prefill_packed_ex(int device, const q3_attn_prefill_packed_ex_args* args);
/* Which rows of a ragged first batch share a packed prefill pass (host arithmetic, no GPU). lengths [n] = prefill
 * positions per row (>= 1), hit_pages [n] = prefix-cache pages each row plans to link (>= 0; NULL = none), row_budget = most
 * activation rows of a pass (>= 128), gemm_ok = the GEMM prefill path may run (model geometry, no debug / profile / no_chunk
 * session, no attention A/B aid). A row packs when gemm_ok, 48 <= length < 1024 and it plans no hit; packs
 * form in row order and close when the next row would pass the budget; a pack of one row is no pack. pass [n] = the row's pass or
 * -1 (it stays in the equal-length groups), row0 [n] = its first activation row inside the pass (0 for -1), *n_passes (optional). */
q3_status q3_prefill_pack_plan(const int32_t* lengths, const int32_t* hit_pages, int32_t n, int32_t row_budget, int32_t gemm_ok,
                               int32_t* pass, int32_t* row0, int32_t* n_passes);
/* What the last q3_session_prefill of a ragged first batch ran: info[0] = layer passes, [1] = of those packed passes, [2] = rows
 * that went through packed passes, [3] = activation rows of the largest pack, [4] = rows that went through equal-length groups,
 * [5..7] = 0. All zeros for a session whose rows have one prefill length (one batched prefill), before the prefill and after a
 * failed one. Q3_PREFILL_PACK=0 (read per call) keeps every row in the groups. */
q3_status q3_session_prefill_info(const q3_session* s, int32_t info[8]);
/* Test API: the kernels that build the prompt rows, exactly ONE launch over host arrays (tests/test_gpu_prompt_rows.py). Every
 * destination (out; trail_len / text_ready / limit) is a host buffer with 64 guard elements in front of and behind its payload; it
 * is uploaded whole and copied back whole, and the kernel is given the payload. What a kernel could not address is Q3_INVALID_ARG
 * before a device is touched. cols 1..65536, n 1..65535.
 * mode 0 = launch_gather_rows_bf16: out [n][cols] = f32(table [n_table][cols] bf16 row ids[r]); ids < n_table.
 * mode 1 = launch_assemble_rows: out [n][cols] from src = rows [n_rows][cols], text_row / codec_id [n], table = codec_emb
 *   [n_table][cols], xvec [cols] (needed by a codec_id of -2), ref_codes [n_ref][16] and cp_embs [15][cp_vocab][cols] bf16 (needed by
 *   a codec_id <= -3: frame -3 - codec_id < n_ref, its code 0 < n_table, codes 1..15 < cp_vocab). text_row < n_rows (negative: none);
 *   codec_id < n_table.
 * mode 2 = launch_copy_rows: out [n][ldd] <- src [n][lds], cols <= lds, ldd (the payload is n * ldd floats).
 * mode 3 = launch_scatter_rows: out = rows [n_rows][cols], row dst_row[r] <- src [n][cols] row r; dst_row < n_rows, the non-negative
 *   ones distinct (negative: skipped).
 * mode 4 = launch_publish_text: ent [n][4] = (b, trail_len, text_ready, limit) into trail_len / text_ready / limit [n_rows]; b inside
 *   [0, n_rows) and distinct. */
typedef struct q3_prompt_rows_ex_args {
    int mode, n, cols, n_table, n_rows, n_ref, cp_vocab, lds, ldd, reserved;
    const uint16_t* table; const uint32_t* ids; const float* src;
    const int* text_row; const int* codec_id; const float* xvec;
    const uint32_t* ref_codes; const uint16_t* cp_embs;
    const int* dst_row; const int* ent;
    float* out; int* trail_len; int* text_ready; int* limit;
} q3_prompt_rows_ex_args;
q3_status q3_prompt_rows_ex(int device, const q3_prompt_rows_ex_args* args);
/* Test API: which kernel launch_attn_c (the codec transformer's whole-utterance attention) runs: kernel -1 = the engine's pick
 * (k_attn_c_mfma unless the Q3_ATTN_C_VALU aid is set), 0 = k_attn_c (VALU), 1 = k_attn_c_mfma. Returns the kernel, or -1 for what
 * the launcher refuses (hd != 64, any other kernel value). No GPU needed. */
int q3_attn_c_path(int hd, int kernel);
/* Test API: ONE launch of the codec transformer / speech encoder attention family over host arrays ([nh*hd][columns] f32, hd = 64,
 * softmax(q.K^T * scale).V per head over keys j <= i).
 * mode 0 = launch_attn_c (whole utterance): q, k, v, o [nh*hd][L]; kernel as in q3_attn_c_path.
 * mode 1 = launch_attn_cs (codec stream): q, o [nh*hd][N]; row r = rows[3r ..] = (a0, e, qcol): its new frames [a0, e) are columns
 *   qcol .. of q / o, its keys and values frames [0, e) of its cache caches[r] = [layers][K | V][nh*hd][cap]; the launch is on
 *   `layer`. max_tiles as the codec stream computes it: the largest tile count ((e - 1) >> 5) - (a0 >> 5) + 1 of a row.
 * mode 2 = launch_attn_cb (block-allocated stream): as mode 1, caches being a pool of n_blocks blocks [layers][K | V][nh*hd][bf]
 *   (bf = cap, a multiple of 32); row r's frames [b * bf, (b + 1) * bf) live in block tabs[tab0[r] + b], b < tab_n[r].
 * mode 3 = launch_mimi_attn (sliding window): as mode 0 over keys i - window < j <= i.
 * o is uploaded whole before the launch and copied back whole after it; the caches are uploaded as given. A bad shape (hd != 64,
 * bf % 32 != 0, e <= a0, e > cap, a row's columns outside [0, N), a block list shorter than ceil(e / bf) or naming a block outside
 * the pool, kernel outside -1..1, window < 1) is Q3_INVALID_ARG and nothing is launched. */
typedef struct q3_attn_c_ex_args {
    int mode, nh, hd, L, kernel, window;
    int N, n_rows, layers, layer, cap, n_blocks, n_tabs;
    float scale;
    const float* q; const float* k; const float* v;
    const int* rows; const float* caches;
    const int* tabs; const int* tab0; const int* tab_n;
    float* o;
} q3_attn_c_ex_args;
q3_status q3_attn_c_ex(int device, const q3_attn_c_ex_args* args);
/* Test API: launch_rope_c (pos NULL: column t at position t) or launch_rope_c_pos (column t at position pos[t]) on q and k
 * [nh*hd][L] in place; cs / sn [n_pos][hd / 2]. hd even; every position must lie inside [0, n_pos). */
q3_status q3_rope_c_ex(int device, float* q, float* k, const float* cs, const float* sn, const int* pos, int nh, int hd, int L, int n_pos);
/* Test API: the codec stream's descriptor-driven movers, one launch each over host buffers that are uploaded whole and copied back
 * whole (guards included). Offsets are in elements; a descriptor that leaves its buffer is Q3_INVALID_ARG before anything runs.
 * q3_copy_cols_ex (launch_copy_cols): column j < n: dst[dst_off + d_off[j] + c * dp[j]] = src[src_off + s_off[j] + c * sp[j]] for
 *   c < C, or 0 when s_off[j] < 0 (a null source).
 * q3_copy_segs_ex (launch_copy_segs): segment s = segs[3s ..] = (src, dst, n): dst[dst + i] = src[src + i], i < n; max_n is the
 *   largest n of the list.
 * q3_gather_frames_ex (launch_gather_frames): dst[j][16] = src[s_off[j] .. + 16] for j < n (u32 codes). */
q3_status q3_copy_cols_ex(int device, const float* src, size_t src_elems, float* dst, size_t dst_elems, int n, int C, const long long* s_off,
                          const long long* d_off, const int* sp, const int* dp, size_t src_off, size_t dst_off);
q3_status q3_copy_segs_ex(int device, const float* src, size_t src_elems, float* dst, size_t dst_elems, int n_segs, const unsigned long long* segs);
q3_status q3_gather_frames_ex(int device, const uint32_t* src, size_t src_elems, const long long* s_off, int n, uint32_t* dst, size_t dst_elems);
/* Test API: launch_rvq_embed: frames [n_frames][16] u32, first_cb [cb_size][cb_dim], rest_cbs [15][cb_size][cb_dim];
 * first_out / rest_out: host buffers of out_elems floats with the [cb_dim][n_frames] result at out_front, uploaded and copied back
 * whole. cb_dim 1..256. Code 0 is taken modulo cb_size; a rest code at or above cb_size reads the last entry. */
q3_status q3_rvq_embed_ex(int device, const uint32_t* frames, int n_frames, const float* first_cb, const float* rest_cbs, int cb_dim, int cb_size,
                          float* first_out, float* rest_out, int out_front, int out_elems);
/* Test API: launch_silu_mul: y[i] = silu(g[i]) * u[i], i < n; y: host buffer of y_elems >= n floats, uploaded and copied back whole. */
q3_status q3_silu_mul_ex(int device, const float* g, const float* u, float* y, long long n, long long y_elems);
/* Test API: the voice-clone encoders' own kernels, ONE launch each over host arrays (tests/test_gpu_clone_ops.py). Everything a kernel
 * would address is checked against the host buffers before the device is touched: a bad shape is Q3_INVALID_ARG, never a launch.
 * `out` is a host buffer of out_elems floats with the result at out_front; it is uploaded whole and copied back whole.
 * q3_spk_op_ex, by op (a / b / result):
 *   0 PAD (launch_spk_pad): a [C][T], b NULL or [C][T] -> [C][Tp] = reflect-padded a (+ b), pl columns on the left, Tp - T - pl on
 *     the right; 0 <= pl <= T - 1, 0 <= Tp - T - pl <= T - 1.
 *   1 COLS (launch_spk_cols): a [C][ld] -> [C][T] = a[c][off + t]; 0 <= off, off + T <= ld.
 *   2 MEAN (launch_spk_mean): a [C][T] -> [C].
 *   3 SE_APPLY (launch_spk_se_apply): a = o [C][T], b = g [C], the result region holds h [C][T] going in: h = o * g[c] + h.
 *   4 ASP_IN (launch_spk_asp_in): a [C][T] -> [3C][T] = [a ; mean ; sqrt(var + 1e-5)].
 *   5 ASP_POOL (launch_spk_asp_pool): a = logits [C][T], b = m [C][T] -> [2C] = softmax-weighted [mean ; sqrt(var + 1e-5)] of m.
 * a_elems / b_elems: floats behind a / b (b_elems 0 with b NULL). C 1..65535, T, Tp, ld 1..2^20. */
typedef struct q3_spk_op_ex_args {
    int op, C, T, pl, Tp, ld, off, reserved;
    long long a_elems, b_elems, out_front, out_elems;
    const float* a; const float* b; float* out;
} q3_spk_op_ex_args;
q3_status q3_spk_op_ex(int device, const q3_spk_op_ex_args* args);
/* q3_mimi_op_ex, by op:
 *   0 ELU (launch_mimi_elu): a [L] -> [L] (C, r, Lf unused).
 *   1 FOLD (launch_mimi_fold): a [C][L] -> [C*r][Lf + lead]; replicate == 0: lead 0, zeros beyond L, (Lf - 1) * r < L; replicate != 0:
 *     lead 1, column 0 = a[c][0], a[c][L - 1] beyond L. elu != 0: ELU on the way. r 1..64, C * r <= 65535.
 *   2 CODEBOOK (launch_mimi_codebook): a = embed_sum [C][L], b = cluster_usage [C] -> [C][L] = a / max(b, 1e-5) (C entries of L floats).
 * L, Lf 1..2^24. */
typedef struct q3_mimi_op_ex_args {
    int op, C, L, r, Lf, elu, replicate, reserved;
    long long a_elems, b_elems, out_front, out_elems;
    const float* a; const float* b; float* out;
} q3_mimi_op_ex_args;
q3_status q3_mimi_op_ex(int device, const q3_mimi_op_ex_args* args);
/* q3_mimi_rvq_ex (launch_mimi_rvq): proj [CD][T], books [n_layers][CB][CD]; codes [T][n_q] u32 is uploaded whole and copied back
 * whole: columns q0 .. q0 + n_layers - 1 of every frame are written, the rest keep what they held. 1 <= CD <= 256, CB 1..65536,
 * T 1..65536, n_layers >= 1, q0 >= 0, q0 + n_layers <= n_q <= 64. */
q3_status q3_mimi_rvq_ex(int device, const float* proj, int T, const float* books, int n_layers, int CB, int CD, uint32_t* codes, int n_q,
                         int q0);
/* Test API: the sampler and the frame-seam kernels in the forms a session launches them, ONE launch each over host arrays (op-level
 * tests). Arguments are checked before any device call: a null pointer, a token / code / row index that would make the kernel read
 * outside a table, a draw outside `u`, a sampler vocab outside 2..4096 are Q3_INVALID_ARG. Every buffer a kernel may write holds
 * `guard` extra elements in front of and behind its payload; it is uploaded whole before the launch and copied back whole after it.
 *
 * q3_sample_row: the per-row sampler record a session derives from a request's options (host only; `pad` is 0). */
typedef struct q3_sample_rec {
    float inv_temp; int apply_temp, greedy;
    int top_k; float top_p; int use_top_p;
    float rep_pen, rep_inv; int use_rep;
    int eos_id, min_new_tokens, pad;
} q3_sample_rec;
q3_status q3_sample_row(const q3_options* opts, q3_sample_rec* out);
/* q3_prompt_shape: the prompt layout a session derives from a request (host only: no device, no model; DESIGN "Prompt layout").
 * n_text: the text tokens counted — the request's own n_text, or the text an open row has received so far. Row indices are relative
 * to the row's first projected text row. The tables are optional (both or neither; cap_positions >= prefill_len): per prefill
 * position the projected text row (-1: none) and the codec embedding (a codec id; -1: none, -2: the x-vector, -3 - i: the summed
 * embeddings of reference frame i). A null request or record, a negative length and too small a table are Q3_INVALID_ARG. */
typedef struct q3_prompt_shape_rec {
    int32_t icl, n_ins, n_ref_text, n_icl, overlay;      /* ICL prompt; instruct / reference-text rows; ICL block and codec overlay positions */
    int32_t prefill_len, n_rows;                         /* prefill positions; projected text rows (tts_eos included) */
    int32_t trailing_len, n_trail;                       /* trailing text rows of the closed text (>= 1) / of an open text so far (no tts_eos) */
    int32_t limit, open_need, prefix_pages;              /* max_length under the ICL cap; fewest text tokens an open row needs; cacheable pages */
    int32_t r_role, r_pad, r_bos, r_text, r_eos, trail_base;
} q3_prompt_shape_rec;
q3_status q3_prompt_shape(const q3_request* req, int n_text, q3_prompt_shape_rec* out, int* text_row, int* codec_id, int cap_positions);
/* q3_sample_ex (launch_sample): row b samples logits[b * ld .. + vocab) with the draw u[b * u_stride + (draw_idx ? draw_idx[b] : 0)]
 * under rows[b] (or `scalar` when rows is NULL) and writes tok[b]. seen [B][vocab] u8: penalty mask, marked at the sampled id.
 * token_count: per-row counters (NULL: token_count_static for every row). advance != 0: frame_idx / pos are advanced, unless the row
 * is FROZEN (limit given, frame_idx >= limit: counters stay, tok / seen are still written) or HELD (text_ready given, frame_idx >=
 * text_ready: nothing is written). logits_hist [B][hist_stride_b]: the raw row is copied to index token_count while that is below
 * hist_cap. Guarded (in/out): tok, seen, token_count, frame_idx, pos, logits_hist. */
typedef struct q3_sample_ex_args {
    int B, vocab, ld, u_stride, u_elems, advance, token_count_static, hist_stride_b, hist_cap, codec_eos, use_suppress, guard;
    q3_sample_rec scalar;
    const float* logits; const float* u; const int* draw_idx; const q3_sample_rec* rows;
    const int* limit; const int* text_ready;
    uint32_t* tok; uint8_t* seen; int* token_count; int* frame_idx; int* pos; float* logits_hist;
} q3_sample_ex_args;
q3_status q3_sample_ex(int device, const q3_sample_ex_args* args);
/* q3_frame_embed_ex (launch_frame_embed): codec_emb [n_sem][H] bf16, cp_embs [15][cp_vocab][H] bf16, tok [B], cp_logits_last
 * [B][cp_vocab], frame_idx / trail_base / trail_len / pad_row / text_ready (nullable) [B], text_rows [n_text_rows][H] f32.
 * Guarded (in/out): codes [B][max_frames][16] u32, out [B][H] f32. frame_idx may equal max_frames (a frozen row). */
typedef struct q3_frame_embed_ex_args {
    int B, H, n_sem, cp_vocab, max_frames, n_text_rows, guard, reserved;
    const uint16_t* codec_emb; const uint16_t* cp_embs; const uint32_t* tok; const float* cp_logits_last;
    const int* frame_idx; const float* text_rows; const int* trail_base; const int* trail_len; const int* pad_row; const int* text_ready;
    uint32_t* codes; float* out;
} q3_frame_embed_ex_args;
q3_status q3_frame_embed_ex(int device, const q3_frame_embed_ex_args* args);
/* q3_cp_gather_ex (launch_cp_gather), one pass: 0 = last_hidden [B][H]; 1 = row tok[b] of codec_emb [n_sem][H] bf16; >= 2 = row
 * argmax(cp_logits[b]) of cp_emb [cp_vocab][H] bf16, recorded as codes[b][frame_idx[b]][pass - 1] while frame_idx[b] < max_frames.
 * proj_tab (nullable, [table rows][proj_dim] f32) replaces the bf16 table for pass >= 1; qkv_tab (nullable, [table rows][qkv_dim]
 * f32, qkv_dim % 4 == 0) is copied to qkv_out as well. Guarded (in/out): out [B][ld_out], qkv_out [B][ld_qkv_out], codes. */
typedef struct q3_cp_gather_ex_args {
    int pass, B, H, n_sem, cp_vocab, max_frames, proj_dim, qkv_dim, ld_out, ld_qkv_out, guard, reserved;
    const float* last_hidden; const uint16_t* codec_emb; const uint32_t* tok; const uint16_t* cp_emb; const float* cp_logits;
    const float* proj_tab; const float* qkv_tab; const int* frame_idx;
    uint32_t* codes; float* out; float* qkv_out;
} q3_cp_gather_ex_args;
q3_status q3_cp_gather_ex(int device, const q3_cp_gather_ex_args* args);
/* q3_rmsnorm_ex: launch_rmsnorm, or launch_rmsnorm_hold when frame_idx / text_ready [rows] are given (a row with frame_idx >=
 * text_ready keeps its old output): y[y_front + r * ldy + c] = x[x_off + r * ldx + c] / sqrt(mean(x_r^2) + eps) * w[c]. x / y are
 * host buffers of x_elems / y_elems floats; y is uploaded and copied back whole. */
q3_status q3_rmsnorm_ex(int device, const float* x, long long x_elems, long long x_off, int ldx, const float* w, float* y, long long y_elems,
                        long long y_front, int ldy, int rows, int cols, float eps, const int* frame_idx, const int* text_ready);
/* Test API: channel norm of x [C][L] over C (launch_layernorm_c / launch_rmsnorm_c): layernorm != 0 takes w and b [C], else w only.
 * y: host buffer of y_elems floats, result at y_front, uploaded and copied back whole. */
q3_status q3_norm_c(int device, int layernorm, const float* x, const float* w, const float* b, int C, int L, float eps,
                    float* y, int y_front, int y_elems);
/* Test API: depthwise causal conv, 7 taps (launch_dwconv7): x [C][L], w [C][7], b [C]; y as in q3_norm_c. */
q3_status q3_dwconv7(int device, const float* x, const float* w, const float* b, int C, int L, float* y, int y_front, int y_elems);
/* Test API: one launch of the row-state kernel (k_row_move, q3_session_park_row / _resume_row) over host buffers. Both buffers go
 * to the device, the n_segs segments — bytes seg_bytes[i] from src_off[i] of the source to dst_off[i] of the destination; mode 0
 * copies, mode 1 exchanges the two runs — run in ONE launch, both buffers come back. Any length and alignment; a segment that
 * leaves a buffer is Q3_INVALID_ARG before anything runs. Segments of one call must not overlap one another. */
q3_status q3_row_move(int device, void* src_host, size_t src_bytes, void* dst_host, size_t dst_bytes, int n_segs, const size_t* src_off,
                      const size_t* dst_off, const size_t* seg_bytes, const int* mode);
/* Qwen3TTS::decode_codes (lib.rs:881-890) / Decoder12Hz::decode (decoder_12hz.rs:411-505):
 * frames [n][16] u32 → n*1920 f32 samples. taps (optional, [Q3_DEC_N] host pointers or NULL)
 * receive stage outputs for the stage-by-stage validation the reference does in
 * tests/reference_validation.rs:1755-2400. */
enum { Q3_DEC_QUANT = 0, Q3_DEC_PRECONV = 1, Q3_DEC_PRETRANS = 2, Q3_DEC_UP0 = 3, Q3_DEC_UP1 = 4,
       Q3_DEC_INIT = 5, Q3_DEC_BLK0 = 6, Q3_DEC_BLK1 = 7, Q3_DEC_BLK2 = 8, Q3_DEC_BLK3 = 9, Q3_DEC_N = 10 };
q3_status q3_decode_codes(q3_model* m, const uint32_t* frames_host, int n_frames, float* pcm_host,
                          float** taps_host);
/* ---------------- codec stream: the vocoder with per-row state, many rows per decode pass ----------------
 * A codec stream keeps, for each of its `rows`, what the vocoder's front needs to go on from where the row stopped (the
 * pre-transformer's K / V, its output latent, two columns of pre_conv history): a push costs O(new frames), not O(frames so
 * far), and ONE pass of launches serves every row pushed in the call. Row state (about 68 KB per frame at the production
 * decoder shape) is allocated when a row is first pushed; Q3_OOM when the device refuses it. No reference counterpart. */
typedef struct q3_codec_stream q3_codec_stream;
q3_status q3_codec_stream_create(q3_model* m, int rows, int max_frames, q3_codec_stream** out);
void      q3_codec_stream_free(q3_codec_stream* cs);
q3_status q3_codec_stream_reset(q3_codec_stream* cs, int row);          /* row starts over at frame 0 */
q3_status q3_codec_stream_pos(q3_codec_stream* cs, int row, int* n_frames);
/* append n_frames[i] frames ([n][16] u32, host) to row rows[i] and decode them, all rows in one pass:
 * pcm_host[i] receives n_frames[i] * samples_per_frame f32 samples — the same bits as those frames in
 * q3_decode_codes over everything the row has been given so far. A row out of range or listed twice, a push past
 * max_frames, a null pointer or a cap[i] below the samples is Q3_INVALID_ARG and changes no row; n_frames[i] = 0 is a
 * no-op for that row. A push that fails on the device after those checks (Q3_HIP_ERROR) leaves the rows it carried at
 * frame 0: their state is not trusted half-written, push them again from their first frame. */
q3_status q3_codec_stream_push(q3_codec_stream* cs, int n_rows, const int* rows, const uint32_t* const* frames_host,
                               const int* n_frames, float* const* pcm_host, const size_t* cap);
/* Block-allocated state: a row's K / V and latent live in blocks of block_frames frames (a positive multiple of 32, otherwise
 * Q3_INVALID_ARG), taken from the stream's free list when a push reaches them and returned by q3_codec_stream_reset and the free of
 * the stream — a row holds what its frames need, not max_frames. max_blocks bounds the blocks in use (0 = no bound): a push that
 * would exceed it is refused as a whole with Q3_OOM before any row's state or position changes. Same samples, bit for bit. */
q3_status q3_codec_stream_create_blocked(q3_model* m, int rows, int max_frames, int block_frames, int max_blocks, q3_codec_stream** out);
/* block figures (any pointer may be NULL): frames and bytes per block, blocks allocated so far, in use now, and the most that
 * were ever in use at once. A stream of q3_codec_stream_create reports block_frames 0 (and zeros). */
q3_status q3_codec_stream_info(q3_codec_stream* cs, int* block_frames, size_t* block_bytes, int* blocks_total, int* blocks_in_use,
                               int* blocks_peak);
/* state-only frames: the front runs over n_frames frames of a row at frame 0 (any other position: Q3_INVALID_ARG) and fills its
 * caches; no stack runs, no samples. Later pushes to the row give the samples of q3_decode_codes(primed | pushed) with the
 * first n_frames * samples_per_frame cut — a voice-clone prompt's reference frames (lib.rs:1022-1041). */
q3_status q3_codec_stream_prime(q3_codec_stream* cs, int row, const uint32_t* frames_host, int n_frames);
/* ---------------- output stage: streamed audio at a requested sample rate, f32 or PCM16 ----------------
 * A stage has `rows` independent rows; each has an output rate, an output format, the last 128 input samples it still needs and a
 * count of what it has consumed. Its input is the engine's 24 kHz mono f32. ONE launch serves every row of a push, whatever their
 * rates, formats and positions. The filter is q3_resample's (the 128-tap Blackman-Harris²-windowed sinc of audio/resample.rs:83-97
 * at 0.95 x the lower Nyquist): with L / M = sample_rate / 24000 in lowest terms, output i sits at input time i M / L and is the
 * dot product of row (i M) mod L of a table taps[L][128] — q3_resample's weights in f64, rounded to f32 — with inputs c - 63 ..
 * c + 64, c = floor(i M / L); f32 products summed in an order that does not depend on how the input was cut into pushes.
 * Rates: 4000..96000 Hz with L <= 320 (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000 among them), else Q3_UNSUPPORTED
 * before the device is touched. 24000 Hz is a copy: no filter, nothing held back, the bits of the 24 kHz path.
 * Streaming rule: after n_in input samples in total a row has returned every output i with floor(i M / L) + 64 <= n_in - 1 (the
 * first push returns about 64 L / M samples fewer than it was given: 2.7 ms); a push with last != 0 returns the rest, up to
 * llround(n_in * sample_rate / 24000) samples in total, against zeros beyond the end — q3_resample's n_out and edge handling.
 * The row then takes no more samples until q3_pcm_stage_set / _reset restarts it (a further flush returns 0 samples).
 * Q3_PCM_S16: q3_pcm16_from_f32's rule on the device (clamp to +-1, x 32767.0f, truncation toward zero, NaN -> 0); the copy to
 * the host carries 2 bytes per sample. Q3_PCM_ULAW / Q3_PCM_ALAW: the ITU-T G.711 mu-law / A-law companding of that int16 value
 * (q3_g711_from_pcm16's bytes: what RTP PCMU / PCMA and telephony media streams carry), 1 byte per sample (uint8_t); a NaN gives
 * the byte of 0 (0xFF / 0xD5). No reference counterpart (nearest: audio::resample / save_wav, whole clips on the host). */
enum { Q3_PCM_F32 = 0, Q3_PCM_S16 = 1, Q3_PCM_ULAW = 2, Q3_PCM_ALAW = 3 };
typedef struct q3_pcm_stage q3_pcm_stage;
/* max_push_samples: the most 24 kHz samples one row takes in one push */
q3_status q3_pcm_stage_create(int device, int rows, size_t max_push_samples, q3_pcm_stage** out);
void      q3_pcm_stage_free(q3_pcm_stage* ps);
q3_status q3_pcm_stage_set(q3_pcm_stage* ps, int row, uint32_t sample_rate, int format);   /* also restarts the row */
q3_status q3_pcm_stage_reset(q3_pcm_stage* ps, int row);                                   /* row starts over at sample 0 */
/* n_in[i] samples (host) for row rows[i], all rows in one pass; last (may be NULL = none) flushes a row. out_host[i] receives
 * n_samples[i] samples in the row's format (float, int16_t or uint8_t), at most cap_samples[i]. A null argument, a row out of range or
 * listed twice, n_in[i] above max_push_samples, samples for a flushed row or a cap below what the push returns
 * (q3_pcm_stage_bound) is Q3_INVALID_ARG and changes no row; so does a push that fails on the device. */
q3_status q3_pcm_stage_push(q3_pcm_stage* ps, int n_rows, const int* rows, const float* const* in_host, const size_t* n_in,
                            const int* last, void* const* out_host, const size_t* cap_samples, size_t* n_samples);
q3_status q3_pcm_stage_bound(uint32_t sample_rate, size_t n_in, size_t* n_out_max);          /* host only: cap for a push of n_in */
/* host only: L, M and (taps_host != NULL) the table [L][128] the stage uploads for this rate */
q3_status q3_pcm_stage_taps(uint32_t sample_rate, float* taps_host, size_t cap_floats, int* L, int* M);
/* q3_codec_stream_push through a stage: the same decode pass, then the samples of row rows[i] go through stage row ps_rows[i]
 * on the stream's stream and the converted bytes are what is copied to the host (out_host[i], n_samples[i] of at most
 * cap_samples[i]; last may be NULL). n_frames[i] = 0 with last[i] != 0 only flushes. The checks of both calls apply, before
 * anything changes. The stage is the caller's: q3_codec_stream_reset does not restart a stage row — it follows the samples that
 * were delivered, so a row that is pushed again from its first frame after a failed push goes on where its listener stopped. */
q3_status q3_codec_stream_push_out(q3_codec_stream* cs, int n_rows, const int* rows, const uint32_t* const* frames_host, const int* n_frames,
                                   q3_pcm_stage* ps, const int* ps_rows, const int* last,
                                   void* const* out_host, const size_t* cap_samples, size_t* n_samples);
/* Sessions: the output of q3_session_next_chunks_out, for all rows; legal before the first streamed chunk (Q3_INVALID_ARG after).
 * q3_session_replace restarts the replaced row's stage row. q3_session_next_chunks_out is q3_session_next_chunks through the
 * session's stage: out_host[b] receives n_samples[b] samples at that rate and format; a row's tail is flushed in the call that
 * reports it done. q3_session_next_chunk* / _decode / _run ignore the setting. */
q3_status q3_session_set_output(q3_session* s, uint32_t sample_rate, int format);
q3_status q3_session_next_chunks_out(q3_session* s, void* const* out_host, const size_t* cap_samples, size_t* n_samples, int* done);
/* Batcher: a streamed ticket's own output (q3_batcher_submit_streamed, or _submit_open with Q3_WANT_STREAM), legal between its
 * submission and the next q3_batcher_step. Its samples then leave through q3_batcher_read_out (cap_samples / n_samples count
 * samples of the ticket's format; otherwise q3_batcher_read's contract) — q3_batcher_read refuses such a ticket and names
 * q3_batcher_read_out; q3_batcher_read_out serves every streamed ticket (24 kHz f32 by default). */
q3_status q3_batcher_ticket_output(q3_batcher* b, int64_t ticket, uint32_t sample_rate, int format);
q3_status q3_batcher_read_out(q3_batcher* b, int64_t ticket, void* out_host, size_t cap_samples, size_t* n_samples, int* done);
/* ---------------- output stage: a speaking rate per row (time-scale modification in front of the resampler) ----------------
 * tempo_permille in 500..2000 (1250: the speech runs 1.25 x as fast; else Q3_INVALID_ARG before the device is touched); 1000, the
 * default, is off: such a row takes the path above and returns its bits. Otherwise the row's 24 kHz input x goes through WSOLA
 * first: frames of W = 720 samples, one every Hs = 360 samples of the output y, frame k taken at p_k = a_k + lag_k with
 * a_k = floor(k Hs tempo / 1000), p_0 = 0 and lag_k in [max(-240, -a_k), 240] the lag whose frame correlates best, normalised by its
 * energy, with the continuation x[p_{k-1} + Hs ..] of the frame before (ties: the smallest |lag|, then the negative one; digital
 * silence gives 0). y[k Hs + j] = w[Hs + j] x[p_{k-1} + Hs + j] + w[j] x[p_k + j] for j < Hs with the periodic Hann window w of W
 * points, and y[j] = x[j] for j < Hs. f32 sums in an order that does not depend on how the input was cut into pushes.
 * Streaming rule: after n input samples in total, the frames k with need_k <= n are computed (need_0 = W, need_k =
 * max(a_k, a_{k-1} + Hs) + 240 + W) and frames x Hs samples of y are final; a push with `last` computes the frames up to
 * ceil(N_out / Hs), N_out = floor((n 1000 + tempo / 2) / tempo), against zeros beyond the end and y is N_out samples long. The
 * resampler takes y as its input stream: the counts and the edge rule above with N_out in the place of n_in. The stretcher's
 * state obeys the same commit rule: a push that is refused or fails leaves the row where it was. Its buffers are allocated by a
 * row's first tempo other than 1000. No reference counterpart (the reference returns whole clips at the model's own pace). */
q3_status q3_pcm_stage_set_tempo(q3_pcm_stage* ps, int row, int tempo_permille);            /* also restarts the row; kept by _set / _reset */
/* host only: the streaming rule — frames computed and samples of y final after n_in_total input samples (ended: after the flush) */
q3_status q3_pcm_stage_tempo_count(int tempo_permille, size_t n_in_total, int ended, size_t* frames, size_t* samples_24k);
/* host only: cap for a push of n_in new samples to a row at this rate and tempo, wherever the row stands and with `last` */
q3_status q3_pcm_stage_bound_tempo(uint32_t sample_rate, int tempo_permille, size_t n_in, size_t* n_out_max);
/* the lags of the frames k0 .. k0 + n - 1 the row's last successful push computed (n = 0: none; lags = NULL with
 * cap = 0: the count alone; any other cap < n: Q3_INVALID_ARG, *n set) */
q3_status q3_pcm_stage_tempo_lags(q3_pcm_stage* ps, int row, int64_t* k0, int* lags, size_t cap, size_t* n);
/* Sessions: the tempo of row b's stage row (b = -1: every row) in q3_session_next_chunks_out; legal while the row has delivered no
 * streamed sample since its start or its q3_session_replace (Q3_INVALID_ARG after, and then no row changes). The other chunk,
 * decode and run calls ignore it, as they ignore q3_session_set_output. */
q3_status q3_session_set_tempo(q3_session* s, int b, int tempo_permille);
/* Batcher: a streamed ticket's tempo; the window and the read of q3_batcher_ticket_output (q3_batcher_read_out). A parked streamed
 * ticket keeps its stage row. */
q3_status q3_batcher_ticket_tempo(q3_batcher* b, int64_t ticket, int tempo_permille);
/* ---------------- output stage: a level per row (gain and look-ahead peak limiter, between the stretcher and the resampler) --------
 * gain_mB in -6000..2400 and ceiling_mB in -2400..0, both in millibel (1/100 dB; else Q3_INVALID_ARG before the device is
 * touched); (0, 0), the default, is off: such a row takes the paths above and returns their bits and their launches. Otherwise,
 * with g = (float)pow(10, gain_mB / 2000) and c = (float)pow(10, ceiling_mB / 2000) (f64, rounded once), the row's 24 kHz
 * stream x (the stretcher's y where it has one) becomes y, all in f32 with every operation rounded once:
 *   u[i] = g x[i];  r[i] = c / |u[i]| where |u[i]| > c, else 1 (a NaN compares false), and 1 for i < 0 and beyond the end;
 *   m[j] = min(r[j] .. r[j + 127]);  a[n] = ((s0 + s1) + (s2 + s3)) / 128, s_q the sum in ascending k of m[n - 127 + k] over
 *   k = q (mod 4), k = 0..127;  y[n] = min(max(u[n] a[n], -c), c).
 * A peak limiter, not a compressor: the gain falls over the 5.3 ms (127 samples) before a peak and recovers over the 5.3 ms
 * after it; every window holds r[n], so |y| <= c at 24 kHz exactly (after a rate change up to the resampler's own overshoot; the
 * S16 / G.711 clamp is still behind it). y is a function of the sample index alone: the stream does not depend on its cuts.
 * Streaming rule: after n input samples the outputs [0, max(0, n - 127)) are final; a push with `last` returns the rest, up to
 * n. The resampler takes y as its input stream: its counts with this count in the place of n_in. The row keeps its last 254
 * inputs under the commit rule of the tails: a push that is refused or fails leaves the row where it was. The step's buffers are
 * allocated by a row's first level other than (0, 0). No reference counterpart. */
q3_status q3_pcm_stage_set_level(q3_pcm_stage* ps, int row, int gain_mB, int ceiling_mB);  /* also restarts the row; kept by _set / _reset / _set_tempo */
/* host only: g and c as the stage computes them (either may be NULL) */
q3_status q3_pcm_stage_level_coeffs(int gain_mB, int ceiling_mB, float* g, float* c);
/* host only: the streaming rule — outputs of the level step final after n_in_total inputs (ended: after the flush) */
q3_status q3_pcm_stage_level_count(size_t n_in_total, int ended, size_t* n_out);
/* host only: cap for a push of n_in new samples to a row with a level at this rate and tempo (1000: no stretcher), wherever the
 * row stands and with `last`: q3_pcm_stage_bound(sample_rate, Y + 127), Y = q3_pcm_stage_bound_tempo's 24 kHz bound or n_in */
q3_status q3_pcm_stage_bound_level(uint32_t sample_rate, int tempo_permille, size_t n_in, size_t* n_out_max);
/* Sessions: the level of row b's stage row (b = -1: every row) in q3_session_next_chunks_out; q3_session_set_tempo's window
 * (legal while the row has delivered no streamed sample since its start or its q3_session_replace) and its persistence (the
 * setting stays with the row across a replace until it is set again). The other chunk, decode and run calls ignore it. */
q3_status q3_session_set_level(q3_session* s, int b, int gain_mB, int ceiling_mB);
/* Batcher: a streamed ticket's level; the window and the read of q3_batcher_ticket_output (q3_batcher_read_out, also at 24 kHz
 * f32). A slot's next owner gets its own setting, off included; a parked streamed ticket keeps its stage row. */
q3_status q3_batcher_ticket_level(q3_batcher* b, int64_t ticket, int gain_mB, int ceiling_mB);
/* ---------------- output stage: a loudness meter and normaliser per row (ITU-R BS.1770-4, in front of the level) ----------------
 * Q3_LOUD_OFF, the default: the row takes the paths above and returns their bits and their launches. Q3_LOUD_METER measures and
 * passes the samples bit for bit; Q3_LOUD_NORMALIZE steers the row to target_mB (millibel of LUFS: -1900 = -19 LUFS, -4000..-500)
 * from the gain prior_mB (-6000..2400, 0 by default); anything else is Q3_INVALID_ARG before the device is touched.
 * The row's 24 kHz stream x (the stretcher's y where it has one) is K-weighted by two biquads (high shelf, high-pass:
 * q3_loudness_kweight(24000), rounded to f32) in transposed direct form II, a non-finite sample entering as 0; all f32, every
 * operation rounded once:  o = b0 v + s1;  s1 = (b1 v - a1 o) + s2;  s2 = b2 v - a2 o.
 * Hops of 2400 samples: e_h = the sum of the squares k^2 in 64 interleaved partial sums (sample j of the hop to partial j mod 64,
 * ascending; folded s_q += s_(q+d), d = 32 .. 1). Blocks of four hops: z_h = ((e_(h-3) + e_(h-2)) + (e_(h-1) + e_h)) (float)(1/9600)
 * for h >= 3. After every hop the gate runs over z_3 .. z_h in f64 (64 interleaved partials as above): Sa, ca over z > Ga =
 * (float)10^(-6.9309); none: no estimate; Gr = 0.1 Sa / ca; Sg, cg over z > Ga and z > Gr; M_h = (float)(Sg / cg). Integrated loudness
 * = -0.691 + 10 log10(M) LUFS, computed by the host. A_h = P = (float)10^(prior_mB / 2000) for h < 3, else
 * min(max(sqrt(T / M_h), A_lo), A_hi) with T = (float)10^((target_mB / 100 + 0.691) / 10), A_lo / A_hi = -+24 dB, else A_(h-1).
 * Sample j of hop h leaves as x (A_(h-2) + (A_(h-1) - A_(h-2)) (j / 2400)): a gain that depends on the hops that ended before hop h
 * began alone, so the step holds nothing back: n samples leave for n that enter, and no count or bound above changes. At most 4096
 * blocks (410 s) are kept; past them M and A are frozen. Not a compressor and not a true-peak limiter: with a gain above 1 set a
 * ceiling (q3_pcm_stage_set_level) behind it. The row's state (filter states, partials, three e, two A, M; the block values
 * append-only) follows the commit rule of the tails. The step's buffers are allocated by a row's first mode other than off.
 * No reference counterpart. */
enum { Q3_LOUD_OFF = 0, Q3_LOUD_METER = 1, Q3_LOUD_NORMALIZE = 2 };
/* host only: the K-weighting's two biquads at a rate of 8000..192000 Hz, each as b0 b1 b2 a0 a1 a2 in f64 (BS.1770's analogue
 * prototypes through the tangent pre-warped bilinear form; at 48000 the tables printed in BS.1770-4) */
q3_status q3_loudness_kweight(uint32_t sample_rate, double* shelf_ba, double* highpass_ba);
/* host only: T, P, the absolute gate and the gain's bounds as the stage computes them (any may be NULL) */
q3_status q3_pcm_stage_loudness_consts(int target_mB, int prior_mB, float* T, float* P, float* gate_abs, float* a_lo, float* a_hi);
q3_status q3_pcm_stage_set_loudness(q3_pcm_stage* ps, int row, int mode, int target_mB, int prior_mB);  /* also restarts the row; kept by _set / _reset / _set_tempo / _set_level */
/* after the row's last successful push: M (0 without an estimate), the last A, the blocks stored and cg (any may be NULL);
 * Q3_INVALID_ARG for a row whose step is off */
q3_status q3_pcm_stage_loudness(q3_pcm_stage* ps, int row, float* mean_square, float* gain, int* blocks, int* gated);
/* the stored block values z_3 ..; cap / n as in q3_pcm_stage_tempo_lags (no buffer and cap 0: the count alone) */
q3_status q3_pcm_stage_loudness_blocks(q3_pcm_stage* ps, int row, float* z, size_t cap, size_t* n);
/* Sessions: the loudness step of row b's stage row (b = -1: every row) in q3_session_next_chunks_out; q3_session_set_tempo's
 * window and persistence. q3_session_loudness: the row's reading (b = -1 is not a row). */
q3_status q3_session_set_loudness(q3_session* s, int b, int mode, int target_mB, int prior_mB);
q3_status q3_session_loudness(q3_session* s, int b, float* mean_square, float* gain, int* blocks, int* gated);
/* Batcher: a streamed ticket's loudness step; the window and the read of q3_batcher_ticket_output (q3_batcher_read_out, also at
 * 24 kHz f32). A slot's next owner gets its own setting, off included; a parked streamed ticket keeps its stage row, history
 * included. _read: the ticket's reading after the parts that have landed — final once q3_batcher_read_out has reported the
 * ticket done, valid until q3_batcher_fetch releases it. */
q3_status q3_batcher_ticket_loudness(q3_batcher* b, int64_t ticket, int mode, int target_mB, int prior_mB);
q3_status q3_batcher_ticket_loudness_read(q3_batcher* b, int64_t ticket, float* mean_square, float* gain, int* blocks, int* gated);
/* ---------------- output stage: a pitch per row in cents (a varispeed step behind the time stretcher) ----------------
 * cents in -1200..1200; 0, the default, is off: such a row takes the paths above and returns their bits and their launches. With the
 * row's tempo t (q3_pcm_stage_set_tempo; 1000 by default) and p = 2^(cents / 1200) in f64, te = llround(t / p) must lie in 500..2000,
 * else Q3_INVALID_ARG before the device is touched: whichever of _set_tempo / _set_pitch comes second refuses and changes nothing.
 * The stretcher then runs at te in the place of t (not at all when te = 1000; q3_pcm_stage_tempo_lags reports the lags of te), and
 * where te != t its output y is resampled by te / t, which brings the duration back to t's and moves the pitch by t / te — within
 * 1.8 cents of the request. Varispeed compensated by time stretching: formants move with the pitch; +-300 cents is the useful
 * range for natural speech, +-1200 is accepted; a formant-preserving shifter is out of scope.
 * The step is q3_resample's filter at sr_in = t, sr_out = te: output j sits at input time j t / te, cj = floor(j t / te),
 * r = (j t) mod te, taps over the inputs cj + k, k = -63 .. 64, at tau = r / te - k: h = fc sinc(fc tau) w^2(tau / 64),
 * fc = 0.95 min(1, te / t), w the Blackman-Harris window (0 from |tau| = 64 on). The taps come from two tables, f64 rounded to
 * f32: Sc[m] = sinc(m / S1), m = 0 .. 61 S1 + 1, and W2[m] = w^2(m / (64 S2)), m = 0 .. 64 S2 + 1, S1 = 512, S2 = 64. With
 * q = |r - k te| the sinc is read at 19 q S1 / (20 max(t, te)) and the window at q S2 / te, each split in integers into an index m
 * and a remainder, f = (float)rem / (float)den correctly rounded; then, every operation rounded once,
 *   s = fma(f1, Sc[m1 + 1] - Sc[m1], Sc[m1]);  w = fma(f2, W2[m2 + 1] - W2[m2], W2[m2]);  a[k mod 4] = fma(s w, x[cj + k], a[k mod 4])
 * in ascending k, and v[j] = (float)fc ((a0 + a1) + (a2 + a3)). Inputs outside [0, N_y) are zeros.
 * Streaming rule, the resampler's with y in the place of its input: after F final samples of y every j with
 * floor(j t / te) + 64 <= F - 1 is out; a push with `last` returns the rest, up to floor((2 N_y te + t) / (2 t)) in total (within 2
 * samples of the row's count without a pitch). The steps behind (loudness, level, resampler) take v as their input stream. The row
 * keeps its last 128 samples of y under the commit rule of the tails. The tables (138 KB, one pair per stage) and a row's tail are
 * allocated by the first pitch that moves a tempo. No reference counterpart (Qwen3-TTS has no pitch input). */
q3_status q3_pcm_stage_set_pitch(q3_pcm_stage* ps, int row, int cents);                    /* also restarts the row; kept by _set / _reset / every _set_* */
/* host only: te and the pitch the row then has, 1200 log2(t / te) cents (either may be NULL) */
q3_status q3_pcm_stage_pitch_plan(int tempo_permille, int cents, int* tempo_eff, double* cents_realized);
/* host only (test hook): S1, S2 and the two tables as the stage uploads them: 61 S1 + 2 and 64 S2 + 2 floats (either buffer may
 * be NULL; both NULL: S1 / S2 alone) */
q3_status q3_pcm_stage_pitch_tables(float* sinc, size_t cap1, float* win, size_t cap2, int* S1, int* S2);
/* host only: the streaming rule — 24 kHz samples behind the stretcher and the pitch step after n_in_total input samples */
q3_status q3_pcm_stage_pitch_count(int tempo_permille, int cents, size_t n_in_total, int ended, size_t* samples_24k);
/* host only: cap for a push of n_in new samples to a row at this rate, tempo and pitch (with_level: and a level), wherever the
 * row stands and with `last`; at 0 cents q3_pcm_stage_bound_tempo's / _bound_level's value */
q3_status q3_pcm_stage_bound_pitch(uint32_t sample_rate, int tempo_permille, int cents, int with_level, size_t n_in, size_t* n_out_max);
/* Sessions: the pitch of row b's stage row (b = -1: every row) in q3_session_next_chunks_out; q3_session_set_tempo's window and
 * persistence; a pitch the row's tempo does not admit (or, in q3_session_set_tempo, a tempo its pitch does not admit) is
 * Q3_INVALID_ARG and then no row changes. */
q3_status q3_session_set_pitch(q3_session* s, int b, int cents);
/* Batcher: a streamed ticket's pitch; the window and the read of q3_batcher_ticket_tempo. A slot's next owner gets its own setting,
 * off included; a parked streamed ticket keeps its stage row. */
q3_status q3_batcher_ticket_pitch(q3_batcher* b, int64_t ticket, int cents);
/* ---------------- output stage: a silence trim and pause cap per row (at the very front of the row, before the stretcher) ----------------
 * threshold_mB: 0, the default, is off: such a row takes the paths above and returns their bits and their launches, and a push
 * without such a row has no launch, copy or wait it did not have. Otherwise -9000..-2000, millibel re full scale of a hop's mean
 * square; edge_ms 0..1000 and pause_ms 20..2000, both multiples of 10; anything else is Q3_INVALID_ARG before the device is touched.
 * E = edge_ms / 10 and P = pause_ms / 10 are hops, P1 = P - P / 2, P2 = P / 2 (integer division).
 * A hop is H = 240 samples (10 ms) of the row's 24 kHz input x; hop h covers x[h H .. h H + H); with N samples in all there are
 * NH = ceil(N / H) hops, samples past N being zeros for the energy and never emitted. e_h is the sum of squares of the hop in 64
 * interleaved f32 partial sums as in the loudness step: sample j goes to partial j mod 64 in ascending j, product and sum each
 * rounded once (no fma), the partials folded s_q += s_(q + d), d = 32 .. 1. A non-finite sample enters the energy as 0 and, where it
 * is kept, leaves unchanged. loud_h = e_h > theta, theta = (float)(240 10^(threshold_mB / 1000)) (f64, rounded once; a NaN compares
 * false). active_h = some loud_g with |g - h| <= G, 0 <= g < NH, G = 2: a guard of 20 ms around onsets and decays. A run is a maximal
 * stretch [s, s + S) of non-active hops. Per run:
 *   leading (s = 0, also when it is the whole stream): hops [0, S - min(S, E)) are dropped;
 *   trailing (s > 0, s + S = NH): hops [s + min(S, E), NH) are dropped;
 *   inner, S <= P: kept whole;
 *   inner, S > P: hops [s + P1, s + S - P2) are dropped, and the seam hop a = s + P1 - 1 leaves crossfaded with hop b = s + S - P2 - 1:
 *     y = add_rn(mul_rn(x[a H + j], w1[j]), mul_rn(x[b H + j], w0[j])), w0[j] = (float)((j + 0.5) / 240), w1[j] = (float)(1 - (j + 0.5) / 240)
 *     (f64, rounded once).
 * Every other kept sample leaves bit for bit; y is the kept hops in order, a function of x alone: it does not depend on how the
 * stream was cut into pushes.
 * Streaming rule: a hop is classified once hops <= h + G are complete, or at the flush. A kept hop leaves in the first push after
 * which its fate no longer depends on samples that have not arrived: an active hop when it is classified; hop i of a later run
 * (s > 0) at once for i < min(E, P1 - 1); a leading run's last min(S, E) hops and everything else a run keeps when the run ends (at
 * the flush for a trailing one). What a row retains is bounded whatever a run's length: of a later run the hops
 * [min(E, P1 - 1), max(E, P1)) and the last P2 + 1, of a leading run the last E, and G complete hops and the partial one:
 * hold(edge_ms, pause_ms) = (max(E, P1) + P2 + G + 2) 240 samples, at most 48 960. The steps behind take y as the row's 24 kHz input
 * stream; their definitions, counts and bounds hold with the kept samples in the place of n_in.
 * The count a push returns depends on the data. A push in which some row has the step on runs in two passes: the samples go up,
 * k_trim runs for those rows, their kept counts come back (one small copy and one wait), then the plan and the launches of the
 * steps behind. max_push_samples applies to what enters the step. For such a row cap_samples must cover
 * q3_pcm_stage_bound_silence(...), checked before the device is touched; n_samples reports what came. The state (two copies under
 * the commit rule of the tails: a push that is refused or fails leaves the row where it was) is allocated by a row's first setting
 * other than off. No reference counterpart. */
q3_status q3_pcm_stage_set_silence(q3_pcm_stage* ps, int row, int threshold_mB, int edge_ms, int pause_ms);  /* also restarts the row; kept by _set / _reset / every other _set_* */
/* the 24 kHz sample counts after the row's last successful push: what entered the step, what left it, and what was cut at the front,
 * in pauses and at the end (a run's cut counts when the run ends; lead_cut is the input index of the first sample that was kept);
 * after the flush n_in - lead_cut - pause_cut - trail_cut == n_out. Any pointer may be NULL; Q3_INVALID_ARG for a row whose step
 * is off */
q3_status q3_pcm_stage_silence(q3_pcm_stage* ps, int row, int64_t* n_in, int64_t* n_out, int64_t* lead_cut, int64_t* pause_cut, int64_t* trail_cut);
/* host only: hold(edge_ms, pause_ms) in samples */
q3_status q3_pcm_stage_silence_hold(int edge_ms, int pause_ms, size_t* samples);
/* host only: cap for a push of n_in new samples to a row with the step on: q3_pcm_stage_bound_pitch(..., n_in + hold) */
q3_status q3_pcm_stage_bound_silence(uint32_t sample_rate, int tempo_permille, int cents, int with_level, int edge_ms, int pause_ms, size_t n_in,
                                     size_t* n_out_max);
/* host only: the whole definition for one clip on the CPU, the same f32 operations in the same order — for the whole-utterance
 * paths, whose callers convert on the host. y receives *n_y <= n samples (y NULL and cap 0: the counts alone); counts (may be NULL)
 * receives n_in, n_out, lead_cut, pause_cut, trail_cut. threshold_mB 0 (off) is Q3_INVALID_ARG here. */
q3_status q3_silence_trim(const float* x, size_t n, int threshold_mB, int edge_ms, int pause_ms, float* y, size_t cap, size_t* n_y, int64_t* counts);
/* Sessions: the silence step of row b's stage row (b = -1: every row) in q3_session_next_chunks_out; q3_session_set_tempo's window
 * and persistence. q3_session_silence: the row's counts (b = -1 is not a row; zeros before the first streamed chunk). */
q3_status q3_session_set_silence(q3_session* s, int b, int threshold_mB, int edge_ms, int pause_ms);
q3_status q3_session_silence(q3_session* s, int b, int64_t* n_in, int64_t* n_out, int64_t* lead_cut, int64_t* pause_cut, int64_t* trail_cut);
/* Batcher: a streamed ticket's silence step; the window and the read of q3_batcher_ticket_output (q3_batcher_read_out, whose counts
 * are then what the step handed on). A slot's next owner gets its own setting, off included; a parked streamed ticket keeps its
 * stage row and the step's state. _read: the counts after the parts that have landed, final once the ticket is done. */
q3_status q3_batcher_ticket_silence(q3_batcher* b, int64_t ticket, int threshold_mB, int edge_ms, int pause_ms);
q3_status q3_batcher_ticket_silence_read(q3_batcher* b, int64_t ticket, int64_t* n_in, int64_t* n_out, int64_t* lead_cut, int64_t* pause_cut, int64_t* trail_cut);
/* ---------------- output stage: a keyed watermark per row (between the loudness step and the level step), and its detector ----------------
 * key: 0, the default, is off: such a row takes the paths above and returns their bits and their launches, and a push without such
 * a row has no launch, copy or wait it did not have. strength_mB: -4000..-1000, millibel re the local signal level (the default of
 * every layer is Q3_MARK_STRENGTH_DEFAULT); anything else is Q3_INVALID_ARG before the device is touched. s = (float)10^(strength_mB / 2000).
 * The carrier c of a key has a period of P = 4096 samples at 24 kHz: a spectrum of unit magnitude in the bins 86..512 of the
 * period (500..3000 Hz: what the stage's own 8 kHz and G.711 outputs keep) with phases 2 pi u_k, u_k = (z_k >> 11) 2^-53,
 * z_k = mix(mix(key ^ fnv1a64("q3.mark.carrier")) + k 0x9E3779B97F4A7C15) with q3_synth_fill's splitmix64 finaliser `mix`, zero
 * elsewhere; the inverse real DFT in f64, scaled to unit RMS, rounded once to f32.
 * A hop is H = 240 samples (10 ms) of the row's 24 kHz stream x at that point of the chain. e_h is the sum of squares of hop h in
 * 64 interleaved f32 partial sums folded d = 32 .. 1, the silence step's rule (no fma; a non-finite sample enters as 0);
 * r_h = sqrt_rn(mul_rn(e_h, (float)(1 / 240))), r_(-1) = r_(-2) = 0. Sample j of hop h, stream index n = 240 h + j, leaves as
 *   g = add_rn(r_(h-2), mul_rn(sub_rn(r_(h-1), r_(h-2)), (float)(j / 240.0)))
 *   y = add_rn(x, mul_rn(mul_rn(s, g), c[n mod 4096]))
 * each operation rounded once. The gain depends on hops that ended before hop h began alone, so the step holds nothing back: n
 * samples out for n in, no count or bound changes, and y is a function of x and the sample index alone: it does not depend on
 * how the stream was cut into pushes. The mark trails the envelope by 10..20 ms: no pre-echo, and a decay is covered by
 * post-masking. A ceiling of the level step holds behind it. The row keeps the partials of its open hop and two roots (two copies
 * under the commit rule of the tails: a push that is refused or fails leaves the row where it was) and its carrier; the row's
 * first key other than 0 allocates them. No payload. No reference counterpart. */
#define Q3_MARK_STRENGTH_DEFAULT (-2600)
q3_status q3_pcm_stage_set_mark(q3_pcm_stage* ps, int row, uint64_t key, int strength_mB);  /* also restarts the row; kept by _set / _reset / every other _set_* */
/* host only: the carrier of a key, c[4096]. key 0 is Q3_INVALID_ARG. */
q3_status q3_mark_carrier(uint64_t key, float* c);
/* host only: the whole definition for one clip on the CPU, the same f32 operations in the same order: the bit reference of the
 * step and the path of the whole-utterance callers (q3_session_run / _decode, q3_batcher_fetch), which convert on the host.
 * y receives n samples (y == x is allowed). key 0 (off) is Q3_INVALID_ARG here. */
q3_status q3_mark_embed(const float* x, size_t n, uint64_t key, int strength_mB, float* y);
/* host only, f64 throughout: the detector for a 24 kHz mono clip z of n >= 2 P samples (shorter: Q3_INVALID_ARG). Hop-wise
 * normalised zn[i] = z[i] / max(r_h, 1e-4) with the hop's own root mean square r_h (a non-finite sample as 0; the clip's last,
 * partial hop against zeros), folded F[m] = sum_k zn[k P + m], correlated cyclically rho[d] = sum_m F[m] c[(m + d) mod P], d in 0..P-1;
 * score = (max_d rho - mean_d rho) / std_d rho, offset = the first argmax: the carrier index of the clip's first sample, so a
 * marked stream cut t samples from its front gives t mod P. A clip carries the key's mark when score >= Q3_MARK_SCORE_DETECT,
 * the one decision threshold (DESIGN 4.12f says how it was measured; q3_mark_score_detect returns it to a binding). Either of
 * score / offset may be NULL. */
#define Q3_MARK_SCORE_DETECT 9.0
double    q3_mark_score_detect(void);
q3_status q3_mark_detect(const float* z, size_t n, uint64_t key, double* score, int* offset);
/* Sessions: the mark of row b's stage row (b = -1: every row) in q3_session_next_chunks_out; q3_session_set_tempo's window and
 * persistence. */
q3_status q3_session_set_mark(q3_session* s, int b, uint64_t key, int strength_mB);
/* Batcher: a streamed ticket's mark; the window and the read of q3_batcher_ticket_output. A slot's next owner gets its own
 * setting, off included; a parked streamed ticket keeps its stage row and the step's state. */
q3_status q3_batcher_ticket_mark(q3_batcher* b, int64_t ticket, uint64_t key, int strength_mB);
/* codes_to_tensor (lib.rs:1417-1431): [n][16] u32 → [16][n] i64 (host helper) */
void      q3_codes_to_tensor(const uint32_t* frames, int n_frames, int64_t* out);

/* ---------------- measurement hooks (bench.py) ---------------- */
/* per-kernel-class accumulated GPU time since the last reset, measured with hipEvents on the
 * session stream when profiling is enabled (q3_session_set_profile) */
q3_status q3_session_set_profile(q3_session* s, int enable);
/* accumulated since the last reset: GPU milliseconds, algorithmic weight bytes and launch count of
 * the bf16 GEMV family (the dominant kernel) */
q3_status q3_session_profile_read(q3_session* s, double* ms, double* bytes, long* launches, int reset);
/* the distinct GEMV launches of the frame loop since profiling was enabled (bench.py's roofline inventory): rows of 8 ints
 * {M, N, K, epilogue, fused input RMSNorm 0/1, reserved (0), tiling, count} — exactly the arguments q3_bench_linear
 * replays; rows == NULL: only *n_rows */
q3_status q3_session_profile_shapes(q3_session* s, int* rows, int cap_rows, int* n_rows, int reset);
/* µs per launch of one GEMV shape: `iters` launches over `n_copies` distinct weight buffers (HBM-resident
 * stream, not Infinity-Cache hits) replayed from one hipGraph and timed with HIP events on that stream.
 * tiled (the inventory's tiling column): 1 = 16-row tiles, 2 = 4-row tiles, 3 = 16-row tiles with the K range split over
 * two workgroups (order-independent atomic reduction), 0 = first-generation row-major kernel, -1 = the engine's
 * choice among the unsplit kernels. Used by bench.py for the roofline of the dominant kernel and by tools/bench_kernels.py. */
q3_status q3_bench_linear(int device, int M, int N, int K, int epi, int rms, int tiled, int iters, int n_copies,
                          double* avg_us);
/* raw stream handle (hipStream_t) the session launches on */
q3_status q3_session_stream(q3_session* s, void** stream);
/* How this session's captured frame is replayed: *path = 0 nothing captured yet / eager launches, 1 = hipGraphLaunch (Q3_AQL=0),
 * 2 = the library's own AQL queue with HIP's packet headers (agent-scope fences at every kernel boundary; bit-identical to path
 * 1; Q3_AQL=1), 4 = own AQL queue, the boundaries between the frame's write-through kernels without those fences (the default
 * since round 6: same codes, ~4.5 % less time per frame; the first and last packet of every frame keep their fences), 3 = own
 * queue without ANY boundary fence — a measurement probe that gives WRONG results (state that crosses frames moves with plain
 * accesses), reachable only with Q3_AQL=2 plus the explicit opt-in Q3_AQL_UNSAFE=1 (a warning is printed);
 * *nodes = dispatch packets per frame (0 on paths 0 / 1). A graph the converter cannot take stays on path 1.
 * The reference replays nothing — every op is an eager candle launch (src/lib.rs:580-652); new here (environment: Q3_AQL). */
q3_status q3_session_submit_info(q3_session* s, int* path, int* nodes);
/* How many of the frame's dispatch packets go out WITHOUT their agent-scope acquire / release fence (paths 3 / 4 of
 * q3_session_submit_info; 0 / 0 on the other paths and before the frame is captured). On path 4 these are the packets of the kernel
 * families that move their data write-through; the first packet of a frame always acquires and the last always releases.
 * New here (the parity tests hold the policy to it). */
q3_status q3_session_submit_fences(q3_session* s, int* acquire_free, int* release_free);
/* Algorithmic HBM bytes of one frame for this session's batch at KV length L */
q3_status q3_session_frame_bytes(q3_session* s, int kv_len, double* weight_bytes, double* kv_bytes);

/* ---------------- on-disk formats (q3_io.cpp) ----------------
 * ModelType (config.rs:176-194); UNKNOWN = loaded without a usable config.json (lib.rs:383-389) */
enum { Q3_MODEL_UNKNOWN = -1, Q3_MODEL_BASE = 0, Q3_MODEL_CUSTOM_VOICE = 1, Q3_MODEL_VOICE_DESIGN = 2 };
/* TalkerConfig::default / ::custom_voice + CodePredictorConfig::default + Decoder12HzConfig::default
 * (talker.rs:176-290, code_predictor.rs:48-113, decoder_12hz.rs:14-67): variant 0 = 0.6B, 1 = 1.7B */
q3_status q3_config_default(int variant, q3_config* out);
/* ParsedModelConfig::from_file (config.rs:238-336): same keys, same unwrap_or defaults; decoder fields
 * are Decoder12HzConfig::default (the reference does not read them from config.json either, lib.rs:345) */
q3_status q3_config_from_json(const char* path, q3_config* out, int* model_type);
/* Qwen3TTS::from_pretrained minus the tokenizer (lib.rs:180-262): <dir>/config.json (optional; weight
 * inspection fallback of lib.rs:371-381), <dir>/model.safetensors, <dir>/speech_tokenizer/model.safetensors
 * (or the parent directory's), every expected tensor uploaded, q3_model_finalize run. Tensors the hot
 * path does not use (speaker_encoder.*, encoder.*) are skipped. device = -1: manifest-only handle. */
q3_status q3_model_load(const char* model_dir, int device, q3_model** out, int* model_type);
/* load_weights (lib.rs:1390-1396) into an existing handle: uploads every tensor of the file the model
 * expects (BF16 / F32 / F16 / F64 sources); n_loaded may be NULL */
q3_status q3_model_load_safetensors(q3_model* m, const char* path, int* n_loaded);
/* header lookup of one tensor: stored dtype (Q3_DTYPE_* or -1), rank and up to cap_dims dims */
q3_status q3_safetensors_info(const char* path, const char* name, int* dtype, int64_t* shape, int cap_dims, int* n_dims);
/* save_wav (audio/io.rs:143-165): mono PCM16, `(clamp(x,-1,1) * 32767) as i16` */
q3_status q3_pcm16_from_f32(const float* samples_host, int64_t n, int16_t* out_host);
q3_status q3_wav_write_pcm16(const char* path, const float* samples_host, int64_t n, uint32_t sample_rate);
/* ITU-T G.711 of n int16 samples, one byte each: law = Q3_PCM_ULAW or Q3_PCM_ALAW (else Q3_INVALID_ARG) — the bytes of the output
 * stage's formats of that name. No reference counterpart. */
q3_status q3_g711_from_pcm16(const int16_t* in_host, int64_t n, int law, uint8_t* out_host);
/* mono G.711 WAV: format tag 7 (mu-law) or 6 (A-law), 8 bits, an 18-byte fmt chunk (cbSize 0) and a fact chunk. q3_wav_read
 * does not read it back (it takes PCM and float). */
q3_status q3_wav_write_g711(const char* path, const uint8_t* bytes_host, int64_t n, uint32_t sample_rate, int law);
/* load_wav (audio/io.rs:106-141): int PCM scaled by 2^(bits-1), float as is, channels averaged to mono.
 * out_host = NULL queries *n_samples / *sample_rate only */
q3_status q3_wav_read(const char* path, float* out_host, int64_t cap, int64_t* n_samples, uint32_t* sample_rate);
/* save_codes_binary / save_audio_binary (bin/generate_audio.rs:788-813): i64 LE frame-major codes, f32 LE samples */
q3_status q3_codes_write_bin(const char* path, const uint32_t* codes_host, int n_frames, int n_groups);
q3_status q3_codes_read_bin(const char* path, uint32_t* codes_host, int cap_frames, int n_groups, int* n_frames);
q3_status q3_audio_write_bin(const char* path, const float* samples_host, int64_t n);
/* the same dump read back — how `--compare` loads the other side's audio (generate_audio.rs:880-886); out_host == NULL or
 * cap == 0: only *n_samples */
q3_status q3_audio_read_bin(const char* path, float* out_host, int64_t cap, int64_t* n_samples);
/* audio::resample / resample_to_24k (audio/resample.rs:17-176): windowed-sinc low-pass with rubato's parameters
 * (sinc_len 128, cutoff 0.95, BlackmanHarris2), output i at input time i * sr_in / sr_out; out_host = NULL queries
 * *n_out = round(n * sr_out / sr_in). Host arithmetic (once per reference clip). */
q3_status q3_resample(const float* in_host, int64_t n, uint32_t sr_in, uint32_t sr_out, float* out_host, int64_t cap, int64_t* n_out);

/* ---------------- speaker encoder (q3_speaker.hip): x-vector voice cloning ----------------
 * SpeakerEncoder (models/speaker.rs:345-469) behind create_voice_clone_prompt (lib.rs:1132-1190): 24 kHz mono
 * reference audio -> log-mel (audio/mel.rs:47-59, 135-227) -> ECAPA-TDNN -> [enc_dim] embedding, the `xvector`
 * of q3_request. Config = SpeakerEncoderConfig (models/config.rs:100-174), weights = `speaker_encoder.*` of a
 * Base checkpoint's model.safetensors (kept f32 on the device; bf16/f16 sources are widened on upload).
 * The ICL half of the prompt (reference codes) comes from the speech encoder below (q3_mimi_*). */
typedef struct q3_spk_config {
    int32_t mel_dim;            /* 128 */
    int32_t enc_dim;            /* 1024 (0.6B) / 2048 (1.7B): the talker's hidden size */
    int32_t channels[5];        /* 512,512,512,512,1536 */
    int32_t kernel_sizes[5];    /* 5,3,3,3,1 */
    int32_t dilations[5];       /* 1,2,3,4,1 */
    int32_t attention_channels; /* 128 */
    int32_t res2net_scale;      /* 8 */
    int32_t se_channels;        /* 128 */
    int32_t sample_rate;        /* 24000 */
} q3_spk_config;
typedef struct q3_speaker_encoder q3_speaker_encoder;
/* SpeakerEncoderConfig::default (config.rs:132-174) */
q3_status q3_spk_config_default(q3_spk_config* out);
/* `speaker_encoder_config` object of config.json (config.rs:233, serde defaults per field); *present = 0 and the
 * defaults when the key is absent (CustomVoice / VoiceDesign checkpoints) */
q3_status q3_spk_config_from_json(const char* path, q3_spk_config* out, int* present);
/* SpeakerEncoder::new (speaker.rs:362-428): allocates the weight arena for the config's tensor manifest */
q3_status q3_spk_create(const q3_spk_config* cfg, int device, q3_speaker_encoder** out);
void q3_spk_free(q3_speaker_encoder* e);
q3_status q3_spk_get_config(const q3_speaker_encoder* e, q3_spk_config* out);
int q3_spk_n_tensors(const q3_speaker_encoder* e);
q3_status q3_spk_tensor_info(const q3_speaker_encoder* e, int i, const char** name, int64_t* n);
/* data_host: n elements of src_dtype (Q3_DTYPE_F32 / Q3_DTYPE_BF16) */
q3_status q3_spk_set_tensor(q3_speaker_encoder* e, const char* name, const void* data_host, int src_dtype, int64_t n);
/* every tensor present -> packs the matrix-core weight images, builds window / DFT / mel-filter tables */
q3_status q3_spk_finalize(q3_speaker_encoder* e);
/* uploads every `speaker_encoder.*` tensor of a safetensors file and finalizes; Q3_MISSING_WEIGHT with the
 * reference's hint (lib.rs:1137-1153) when the file has none */
q3_status q3_spk_load_safetensors(q3_speaker_encoder* e, const char* path);
/* frames the mel front end yields for n samples: (n + 2*384 - 1024) / 256 + 1 (mel.rs:168-199). 0 for a clip too short for one
 * frame (n_samples < 256, zero and negative counts included). -1 = no count for n_samples above 2^38 (the count would leave the
 * result's range long before n + 768 leaves int64_t's): q3_spk_mel, q3_spk_encode and q3_spk_encode_ref answer such a length with
 * Q3_INVALID_ARG. Host only. */
int q3_spk_mel_frames(int64_t n_samples);
/* MelSpectrogram::compute_for_speaker_encoder (mel.rs:135-166): mel_host [mel_dim][T], T = q3_spk_mel_frames(n) */
q3_status q3_spk_mel(q3_speaker_encoder* e, const float* samples_host, int64_t n, float* mel_host, int64_t cap_floats, int* n_frames);
/* Test API: the front-end tables of a finalized encoder as its mel kernel reads them, copied back from the device: the periodic Hann
 * window win_host [1024] and the Slaney filterbank fb_host [mel_dim][513] */
q3_status q3_spk_tables(q3_speaker_encoder* e, float* win_host, float* fb_host);
/* SpeakerEncoder::forward (speaker.rs:443-469) for one mel [mel_dim][T]; taps (test hook): NULL or 6 host pointers
 * (NULL entries skipped): blocks.0 out, the three SE-Res2Net outs [C][T], MFA out [C4][T], pooled [2*C4] */
q3_status q3_spk_forward(q3_speaker_encoder* e, const float* mel_host, int T, float* out_host, float** taps_host);
/* SpeakerEncoder::encode (speaker.rs:431-438) = mel + forward; sample_rate must be 24000 (the reference resamples
 * first, lib.rs:1156-1166 — q3_resample before calling) */
q3_status q3_spk_encode(q3_speaker_encoder* e, const float* samples_host, int64_t n, uint32_t sample_rate, float* out_host);

/* ---------------- speech-tokenizer encoder (q3_mimi.hip): ICL reference codes from raw audio ----------------
 * Encoder12Hz (models/codec/encoder_12hz.rs:34-144) behind create_voice_clone_prompt's ICL branch (lib.rs:1172-1178):
 * 24 kHz mono reference audio -> SEANet encoder -> 8-layer transformer -> stride-2 conv -> split residual VQ ->
 * frames of 16 codebook indices at 12.5 Hz, the `ref_codes` of q3_request. The reference instantiates candle-transformers'
 * Mimi (`mimi::Config::v0_1(Some(16))`, encoder_12hz.rs:73) over the HF-format `encoder.*` keys of
 * speech_tokenizer/model.safetensors; this is the published Mimi encoder for that format (weights kept f32 on the device). */
typedef struct q3_mimi_config {
    int32_t n_filters;      /* 64   SEANet base width */
    int32_t hidden;         /* 512  SEANet output / transformer width */
    int32_t ratios[4];      /* 4, 5, 6, 8: strides of the four down-sampling stages, in encoder order (24 kHz -> 25 Hz) */
    int32_t kernel;         /* 7 */
    int32_t res_kernel;     /* 3 */
    int32_t last_kernel;    /* 3 */
    int32_t compress;       /* 2 */
    int32_t n_layers;       /* 8 */
    int32_t n_heads;        /* 8 */
    int32_t head_dim;       /* 64 */
    int32_t inter;          /* 2048 */
    int32_t window;         /* 250: causal attention context in frames */
    int32_t cb_size;        /* 2048 */
    int32_t cb_dim;         /* 256 */
    int32_t n_q;            /* 16 codebooks: */
    int32_t n_sem;          /* 1 semantic + 15 acoustic */
    float norm_eps;         /* 1e-5 */
    float rope_theta;       /* 1e4 */
} q3_mimi_config;
typedef struct q3_speech_encoder q3_speech_encoder;
/* mimi::Config::v0_1(Some(16)) (encoder_12hz.rs:73) */
q3_status q3_mimi_config_default(q3_mimi_config* out);
/* Encoder12Hz::from_weights (encoder_12hz.rs:54-117): allocates the weight arena for the config's tensor manifest; device -1 = manifest only */
q3_status q3_mimi_create(const q3_mimi_config* cfg, int device, q3_speech_encoder** out);
void q3_mimi_free(q3_speech_encoder* e);
q3_status q3_mimi_get_config(const q3_speech_encoder* e, q3_mimi_config* out);
int q3_mimi_n_tensors(const q3_speech_encoder* e);
q3_status q3_mimi_tensor_info(const q3_speech_encoder* e, int i, const char** name, int64_t* n);
/* data_host: n elements of src_dtype (Q3_DTYPE_F32 / Q3_DTYPE_BF16), checkpoint layout (the strided convs are re-laid on upload) */
q3_status q3_mimi_set_tensor(q3_speech_encoder* e, const char* name, const void* data_host, int src_dtype, int64_t n);
q3_status q3_mimi_finalize(q3_speech_encoder* e);
/* Encoder12Hz::from_safetensors (encoder_12hz.rs:45-48): every `encoder.*` tensor of speech_tokenizer/model.safetensors, then
 * finalize; Q3_MISSING_WEIGHT "No encoder keys found …" (encoder_12hz.rs:68-70) when the file has none */
q3_status q3_mimi_load_safetensors(q3_speech_encoder* e, const char* path);
/* frames for n samples: ceil over the four strides, then ceil(/2). 0 for a null config, n_samples < 1 or a stride outside 1 .. 16
 * (q3_mimi_create's range); -1 = no count for n_samples above 2^48 or a count beyond INT32_MAX. Host only. */
int q3_mimi_frames(const q3_mimi_config* cfg, int64_t n_samples);
/* Encoder12Hz::encode (encoder_12hz.rs:119-144): codes_host [T][n_q] u32 (frame-major, like q3_request.ref_codes);
 * codes_host == NULL: only *n_frames. sample_rate must be 24000 (q3_resample first). taps_host (test hook): NULL or 3 host
 * pointers (NULL entries skipped): SEANet out [hidden][T25], transformer out [hidden][T25], down-sampled [hidden][T] */
q3_status q3_mimi_encode(q3_speech_encoder* e, const float* samples_host, int64_t n, uint32_t sample_rate, uint32_t* codes_host,
                         int cap_frames, int* n_frames, float** taps_host);

/* ---------------- reference audio intake (q3_intake.hip, q3_io.cpp): a clip as it lies on disk -> 24 kHz mono f32 on the device ----
 * The mirror of the output stage (q3_pcm_stage_*) on the input side, DESIGN 4.14: load_wav + resample_to_24k (audio/io.rs:106-141,
 * audio/resample.rs:173-176, lib.rs:1156-1166) as one launch, k_intake. A clip's interleaved samples in their on-disk format are
 * decoded by q3_wav_read's rule (an integer iv becomes (float)iv / 2^(bits-1), 8-bit is unsigned, f32 as it is, G.711 expanded to
 * int16 first), the channels summed in ascending order in f32 and divided by (float)channels, and the mono stream resampled with
 * q3_resample's filter as a table: L / M = 24000 / sample_rate in lowest terms, output i = row (i M) mod L of taps[L][128] against
 * inputs c - 63 .. c + 64, c = floor(i M / L), zeros outside the clip, f32 fmas in k_pcm_stage's fixed order, n_out =
 * llround(frames * 24000 / sample_rate). At 24000 Hz there is no filter: the decoded, downmixed samples bit for bit.
 * Rates: 4000 .. 96000 Hz with 24000 / gcd(sample_rate, 24000) <= 320 (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100,
 * 48000, 96000, ...), else Q3_UNSUPPORTED before the device is touched (q3_resample takes every rate, on the host). Channels 1 .. 8,
 * n_out 1 .. 24000 * 120 (q3_mimi_encode's limit). The samples stay on the device for both encoders (q3_spk_encode_ref,
 * q3_mimi_encode_ref). No reference counterpart beyond the lines above. */
enum { Q3_SRC_U8 = 0, Q3_SRC_S16 = 1, Q3_SRC_S24 = 2, Q3_SRC_S32 = 3, Q3_SRC_F32 = 4, Q3_SRC_ULAW = 5, Q3_SRC_ALAW = 6 };
/* data: frames * channels interleaved little-endian samples of `format` (Q3_SRC_*), at any address */
typedef struct q3_clip { const void* data; int64_t frames; int32_t channels; uint32_t sample_rate; int32_t format; } q3_clip;
/* format: Q3_SRC_*; bits per sample as the file states them; data_offset / data_bytes: the data chunk's samples within the file
 * (whole frames only: frames * channels * bits / 8 bytes) */
typedef struct q3_wav_desc { int32_t format, channels, bits; uint32_t sample_rate; int64_t frames, data_offset, data_bytes; } q3_wav_desc;
typedef struct q3_ref_audio q3_ref_audio;
/* what a WAV file holds, without decoding it (host only): everything q3_wav_read accepts, and WAVE tags 7 / 6 (mu-law / A-law, 8
 * bits: the files q3_wav_write_g711 writes). Q3_IO / Q3_UNSUPPORTED as q3_wav_read. */
q3_status q3_wav_info(const char* path, q3_wav_desc* out);
/* ITU-T G.711 expansion of n bytes to int16, law = Q3_PCM_ULAW or Q3_PCM_ALAW (else Q3_INVALID_ARG): the counterpart of
 * q3_g711_from_pcm16 (host only) */
q3_status q3_g711_to_pcm16(const uint8_t* in_host, int64_t n, int law, int16_t* out_host);
/* the intake's table for sample_rate: *L, *M and taps_host[L][128]; taps_host == NULL queries L / M only (q3_pcm_stage_taps'
 * contract; host only) */
q3_status q3_intake_taps(uint32_t sample_rate, float* taps_host, size_t cap_floats, int* L, int* M);
/* *n_out = the 24 kHz samples n_in frames at sample_rate become (q3_resample's count; host only) */
q3_status q3_intake_count(uint32_t sample_rate, int64_t n_in, int64_t* n_out);
/* n clips (1 .. 64) in one upload and one launch; out[i] receives clip i's object. All or nothing: on any refusal or device error no
 * object is created and out is untouched. Synchronises before it returns: work on any stream may read the objects afterwards. */
q3_status q3_ref_audio_create_many(int device, int n, const q3_clip* clips, q3_ref_audio** out /* [n] */);
q3_status q3_ref_audio_create(int device, const q3_clip* clip, q3_ref_audio** out);
/* q3_wav_info, a read-only mapping of the file, q3_ref_audio_create */
q3_status q3_ref_audio_from_wav(const char* path, int device, q3_ref_audio** out);
/* any of the out pointers may be NULL; sr_in / format / channels: what the clip was */
q3_status q3_ref_audio_info(const q3_ref_audio* r, int64_t* n_samples, int* device, uint32_t* sr_in, int* format, int* channels);
/* the 24 kHz samples; host == NULL: only *n */
q3_status q3_ref_audio_read(q3_ref_audio* r, float* host, int64_t cap, int64_t* n);
/* the mark's detector (q3_mark_detect's definition) on the clip where the intake left it: the fold in f32 with a fixed summation
 * order (k_mark_fold), the 4096 x 4096 correlation with the carrier staged in LDS (k_mark_corr), the 16 KB of rho back, score and
 * offset from rho in f64 on the host. Clips shorter than 2 P = 8192 samples at 24 kHz and key 0 are Q3_INVALID_ARG. */
q3_status q3_ref_audio_mark_score(q3_ref_audio* r, uint64_t key, double* score, int* offset);
void q3_ref_audio_free(q3_ref_audio* r);
/* q3_spk_encode / q3_mimi_encode of the object's samples, read on the device by the encoder's own stream: the same kernels, workspace
 * and length checks. An object on another device than the encoder's: Q3_INVALID_ARG. */
q3_status q3_spk_encode_ref(q3_speaker_encoder* e, const q3_ref_audio* r, float* out_host);
q3_status q3_mimi_encode_ref(q3_speech_encoder* e, const q3_ref_audio* r, uint32_t* codes_host, int cap_frames, int* n_frames,
                             float** taps_host);

/* ---------------- many reference clips in one packed pass of each encoder ----------------
 * n = 1 .. 64 objects of different lengths, laid side by side along the time axis of the encoders' [C][L] tensors, so every conv
 * launch covers all of them. Each clip's result is bit-equal to q3_spk_encode_ref / q3_mimi_encode_ref of that clip alone, whatever
 * the other clips are and wherever it lies. All or nothing: every clip is checked before the device is touched (null entry, another
 * device, more than 120 s, too few mel frames for the reflect padding, output too small); a refusal names the clip's index
 * ("clip 2: ...") in q3_last_error and writes nothing. Both calls run on the encoder's own stream and synchronise before they return.
 * No reference counterpart: the reference encodes one clip per call. */
/* Encoder12Hz::encode's lengths (encoder_12hz.rs:119-144) for a list of clips: where each clip's slot lies. Pure host arithmetic, no
 * device. A slot is the clip's q3_mimi_frames frames plus one guard frame of *frame_samples = 2 * prod(ratios) samples; `start` is
 * the slot's first sample inside its pass. A pass holds consecutive clips whose slots sum to at most max_pass_samples (a clip whose
 * own slot is larger gets a pass to itself). *packable = 0: one guard frame does not cover the left context of every conv of this
 * configuration, and q3_mimi_encode_refs runs clip by clip. frame_samples / packable / n_passes may be NULL. */
typedef struct q3_mimi_pack_clip { int32_t frames; int32_t pass; int64_t start; } q3_mimi_pack_clip;
q3_status q3_mimi_pack_plan(const q3_mimi_config* cfg, const int64_t* n_samples, int n, int64_t max_pass_samples, q3_mimi_pack_clip* clips,
                            int64_t* frame_samples, int* packable, int* n_passes);
/* Encoder12Hz::encode (encoder_12hz.rs:119-144, as called by lib.rs:1172-1178) of n objects: n_frames [n]; codes_host
 * [sum of n_frames][n_q], clip after clip (NULL: only n_frames); cap_frames: frames codes_host holds. taps_host (test hook): NULL or
 * 3 * n host pointers indexed [clip][tap], each as q3_mimi_encode's (NULL entries skipped). Passes of at most 120 s of slots. */
q3_status q3_mimi_encode_refs(q3_speech_encoder* e, const q3_ref_audio* const* refs, int n, uint32_t* codes_host, int cap_frames,
                              int* n_frames, float** taps_host);
/* SpeakerEncoder::encode (speaker.rs:431-438, as called by lib.rs:1168) of n objects: out_host [n][enc_dim]. taps_host (test hook):
 * NULL or 6 * n host pointers indexed [clip][tap], each as q3_spk_forward's (NULL entries skipped). Passes of at most 120 s of audio. */
q3_status q3_spk_encode_refs(q3_speaker_encoder* e, const q3_ref_audio* const* refs, int n, float* out_host, float** taps_host);

/* ---------------- data parallelism without torch.distributed (q3_dp.cpp) ----------------
 * one process per GPU, utterance i -> rank i mod N, exactly one collective on the data path — the
 * broadcast of rank 0's weight arena over RCCL (xGMI) — plus an all-gather of a few doubles for end-of-job timing. The
 * reference has no multi-GPU code to replace (per-call KV / RNG / masks, lib.rs:744-756, make utterances independent);
 * these entry points are what its Rust host would call where bench.py uses torch.distributed. RCCL is dlopen'ed on the
 * first call. Rendezvous = the host ships the 128-byte id from rank 0 to the other ranks by its own means
 * (file, TCP, MPI, environment). */
#define Q3_DP_ID_BYTES 128
typedef struct q3_dp_comm q3_dp_comm;
/* ncclGetUniqueId: call on rank 0, hand the bytes to every rank */
q3_status q3_dp_unique_id(void* id_out /* Q3_DP_ID_BYTES */);
/* ncclCommInitRank on `device` (collective: every rank of the job must call it) */
q3_status q3_dp_init(int rank, int world, const void* id, int device, q3_dp_comm** out);
void q3_dp_free(q3_dp_comm* c);
q3_status q3_dp_info(const q3_dp_comm* c, int* rank, int* world);
/* ncclBroadcast of the whole weight arena from `root` (collective); non-root ranks are marked loaded and must then
 * call q3_model_finalize themselves. world == 1: the broadcast degenerates to a self-copy RCCL performs in place. */
q3_status q3_dp_broadcast_weights(q3_dp_comm* c, q3_model* m, int root);
/* ncclAllGather of n doubles per rank: out_host [world][n] (timings, frame counts) */
q3_status q3_dp_allgather_f64(q3_dp_comm* c, const double* in_host, int n, double* out_host);

#ifdef __cplusplus
}
#endif
#endif /* Q3TTS_H */
