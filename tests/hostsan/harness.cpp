// Host-sanitizer harness of the C ABI (built by tests/hostsan/build.sh, run by tests/test_host_sanitizers.py).
//
// libq3tts's HOST code, compiled with AddressSanitizer + UndefinedBehaviorSanitizer and linked into this stand-alone program.
// It calls only what needs no device, and refuses to run where there is one: its first act is q3_device_count().
//   harness sizes | files | dsp | refusals
// Every buffer handed to the library is a heap allocation of exactly the documented size (Buf<T>), so ASan's redzones stand right
// behind what the library may touch. Every status must be a q3_status, and a failure must carry a message. Each sub-command ends
// with "<name>: N cases, M accepted, K refused"; the sanitizers end the process at their first report.
//
// What this cannot see: anything behind a device (launchers, sessions, the batcher); the same code when it is loaded into python;
// and reads past the end of a MAPPED file at arbitrary lengths — ASan puts no redzone behind a mapping, a read past the end lands in
// the zero fill of the file's last page. Only a file that ends exactly on a page boundary has an unmapped byte behind it, so every
// seed also exists in a page-aligned form and every header mutation is applied to that form too; truncations (which move the end off
// the boundary) are run all the same, for the statuses and the buffers, but cannot show an over-read of the mapping.
#include "q3tts.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <limits>
#include <string>
#include <vector>

namespace {

enum { EXIT_HAS_DEVICE = 77 };        // the skip status: a device is visible, nothing was called
const size_t PAGE = 4096;

long g_cases = 0, g_ok = 0, g_refused = 0;

[[noreturn]] void die(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    fprintf(stdout, "HARNESS FAILURE: "); vfprintf(stdout, fmt, ap); fprintf(stdout, "\n");
    va_end(ap);
    fflush(stdout);
    exit(1);
}

// one call's status: inside the enum, and a failure has a message
int note(const char* what, int st) {
    ++g_cases;
    if (st < Q3_OK || st > Q3_OOM) die("%s: status %d is no q3_status", what, st);
    if (st == Q3_OK) { ++g_ok; return st; }
    ++g_refused;
    const char* e = q3_last_error();
    if (!e || !*e) die("%s: status %d with an empty q3_last_error()", what, st);
    return st;
}
// an entry that answers with a value: `accepted` says whether that value is an answer or the entry's refusal
void note_value(bool accepted) { ++g_cases; if (accepted) ++g_ok; else ++g_refused; }
void must(bool ok, const char* fmt, ...) {
    if (ok) return;
    va_list ap; va_start(ap, fmt);
    fprintf(stdout, "HARNESS FAILURE: "); vfprintf(stdout, fmt, ap); fprintf(stdout, "\n");
    va_end(ap);
    fflush(stdout);
    exit(1);
}
int finish(const char* name) {
    printf("%s: %ld cases, %ld accepted, %ld refused\n", name, g_cases, g_ok, g_refused);
    fflush(stdout);
    return 0;
}

// a heap block of exactly n elements (n = 0: a block of no bytes, every access to which ASan reports)
template <class T>
struct Buf {
    T* p; size_t n;
    explicit Buf(size_t n_, int fill = 0) : p((T*)malloc(n_ * sizeof(T))), n(n_) {
        if (!p) die("out of memory (%zu elements)", n_);
        memset((void*)p, fill, n * sizeof(T));
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { free(p); }
    T& operator[](size_t i) { return p[i]; }
    operator T*() { return p; }
};

// ---- the grids ----
const uint64_t P40 = 1ull << 40, P48 = 1ull << 48;
std::vector<uint64_t> grid_u64(std::initializer_list<uint64_t> limits) {
    std::vector<uint64_t> g = {0, 1, (uint64_t)INT32_MAX, P40, P48, P48 + 1, (uint64_t)INT64_MAX / 2, (uint64_t)INT64_MAX, (uint64_t)SIZE_MAX};
    for (uint64_t l : limits) { g.push_back(l - 1); g.push_back(l); g.push_back(l + 1); }
    return g;
}
std::vector<int64_t> grid_i64(std::initializer_list<int64_t> limits) {
    std::vector<int64_t> g = {0, 1, -1, INT64_MIN, INT32_MAX, (int64_t)P40, (int64_t)P48, (int64_t)P48 + 1, INT64_MAX / 2, INT64_MAX};
    for (int64_t l : limits) { g.push_back(l - 1); g.push_back(l); g.push_back(l + 1); }
    return g;
}
std::vector<int> grid_int(std::initializer_list<int> limits) {
    std::vector<int> g = {0, 1, -1, INT_MIN, INT_MAX};
    for (int l : limits) { g.push_back(l - 1); g.push_back(l); g.push_back(l + 1); }
    return g;
}
// every rate the output stage and the intake document, the ends of their range, and three that are none
const uint32_t RATES[] = {4000, 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000, 0, 7, 192001};
const uint32_t FEW_RATES[] = {24000, 44100, 8000, 7};

// ================================================================================================================================
// sizes: every host-only size, count, plan and path function
// ================================================================================================================================
q3_request request_of(int kind, Buf<uint32_t>& text, Buf<uint32_t>& ins, Buf<uint32_t>& ref, Buf<uint32_t>& ref_text, Buf<float>& xvec) {
    q3_request r; memset(&r, 0, sizeof r);
    r.text_ids = text; r.n_text = (int32_t)text.n;
    r.opts.temperature = 0.9; r.opts.top_p = 0.9; r.opts.repetition_penalty = 1.05; r.opts.max_length = 64; r.opts.top_k = 50;
    r.opts.eos_token_id = 2150; r.opts.chunk_frames = 10; r.opts.min_new_tokens = 2;
    r.speaker_id = 3000; r.language_id = 2050;
    switch (kind) {
        case 0: r.mode = Q3_MODE_CUSTOM_VOICE; break;                                                     // preset
        case 1: r.mode = Q3_MODE_VOICE_DESIGN; r.instruct_ids = ins; r.n_instruct = (int32_t)ins.n; break;
        case 2: r.mode = Q3_MODE_VOICE_CLONE; r.xvector = xvec; break;                                    // x-vector
        default: r.mode = Q3_MODE_VOICE_CLONE; r.xvector = xvec; r.ref_codes = ref; r.n_ref = (int32_t)(ref.n / 16);   // ICL
                 r.ref_text_ids = ref_text; r.n_ref_text = (int32_t)ref_text.n; break;
    }
    return r;
}

void sizes_pcm_stage() {
    size_t o = 0;
    for (uint32_t sr : RATES) {
        for (uint64_t n : grid_u64({P48})) note("q3_pcm_stage_bound", q3_pcm_stage_bound(sr, (size_t)n, &o));
        note("q3_pcm_stage_bound", q3_pcm_stage_bound(sr, 10, nullptr));
        for (int tempo : grid_int({500, 1000, 2000}))
            for (uint64_t n : grid_u64({P48})) {
                note("q3_pcm_stage_bound_tempo", q3_pcm_stage_bound_tempo(sr, tempo, (size_t)n, &o));
                note("q3_pcm_stage_bound_level", q3_pcm_stage_bound_level(sr, tempo, (size_t)n, &o));
            }
        // the tables: the query, then a buffer of exactly that size, then one float short
        int L = 0, M = 0;
        if (note("q3_pcm_stage_taps", q3_pcm_stage_taps(sr, nullptr, 0, &L, &M)) == Q3_OK) {
            Buf<float> t((size_t)L * 128), s((size_t)L * 128 - 1);
            must(note("q3_pcm_stage_taps", q3_pcm_stage_taps(sr, t, t.n, &L, &M)) == Q3_OK, "q3_pcm_stage_taps refused its own size at %u", sr);
            must(note("q3_pcm_stage_taps", q3_pcm_stage_taps(sr, s, s.n, nullptr, nullptr)) != Q3_OK, "q3_pcm_stage_taps took a short buffer at %u", sr);
        }
        if (note("q3_intake_taps", q3_intake_taps(sr, nullptr, 0, &L, &M)) == Q3_OK) {
            Buf<float> t((size_t)L * 128), s((size_t)L * 128 - 1);
            must(note("q3_intake_taps", q3_intake_taps(sr, t, t.n, &L, &M)) == Q3_OK, "q3_intake_taps refused its own size at %u", sr);
            must(note("q3_intake_taps", q3_intake_taps(sr, s, s.n, nullptr, nullptr)) != Q3_OK, "q3_intake_taps took a short buffer at %u", sr);
        }
        int64_t c = 0;
        for (int64_t n : grid_i64({24000LL * 120, 24000LL * 480})) note("q3_intake_count", q3_intake_count(sr, n, &c));
        note("q3_intake_count", q3_intake_count(sr, 1, nullptr));
    }
    for (uint32_t sr : {7999u, 8000u, 8001u, 24000u, 44100u, 191999u, 192000u, 192001u, 0u, UINT32_MAX}) {
        Buf<double> sh(6), hp(6);
        note("q3_loudness_kweight", q3_loudness_kweight(sr, sh, hp));
        note("q3_loudness_kweight", q3_loudness_kweight(sr, nullptr, hp));
    }
    for (uint32_t sr : FEW_RATES)
        for (int tempo : grid_int({500, 1000, 2000}))
            for (int cents : grid_int({-1200, 1200}))
                for (int lvl = 0; lvl < 2; ++lvl)
                    for (uint64_t n : grid_u64({P48})) note("q3_pcm_stage_bound_pitch", q3_pcm_stage_bound_pitch(sr, tempo, cents, lvl, (size_t)n, &o));
    for (uint32_t sr : {24000u, 44100u, 7u})
        for (int tempo : {499, 500, 1000, 2000, 2001})
            for (int cents : {-1200, 0, 1200, 1201})
                for (int lvl = 0; lvl < 2; ++lvl)
                    for (int edge : grid_int({10, 1000, 15}))
                        for (int pause : grid_int({20, 2000, 25}))
                            for (uint64_t n : grid_u64({P48, P48 - 48000}))
                                note("q3_pcm_stage_bound_silence", q3_pcm_stage_bound_silence(sr, tempo, cents, lvl, edge, pause, (size_t)n, &o));
    note("q3_pcm_stage_bound_silence", q3_pcm_stage_bound_silence(24000, 1000, 0, 0, 100, 200, 10, nullptr));
    for (int tempo : grid_int({500, 1000, 2000}))
        for (uint64_t n : grid_u64({P48, 720, 960}))
            for (int ended = 0; ended < 2; ++ended) {
                size_t f = 0, y = 0;
                note("q3_pcm_stage_tempo_count", q3_pcm_stage_tempo_count(tempo, (size_t)n, ended, &f, &y));
                note("q3_pcm_stage_tempo_count", q3_pcm_stage_tempo_count(tempo, (size_t)n, ended, nullptr, nullptr));
                for (int cents : grid_int({-1200, 1200})) note("q3_pcm_stage_pitch_count", q3_pcm_stage_pitch_count(tempo, cents, (size_t)n, ended, &y));
            }
    note("q3_pcm_stage_pitch_count", q3_pcm_stage_pitch_count(1000, 100, 10, 0, nullptr));
    for (uint64_t n : grid_u64({P48, 127, 128}))
        for (int ended = 0; ended < 2; ++ended) { note("q3_pcm_stage_level_count", q3_pcm_stage_level_count((size_t)n, ended, &o)); }
    note("q3_pcm_stage_level_count", q3_pcm_stage_level_count(1, 0, nullptr));
    for (int tempo : grid_int({500, 1000, 2000}))
        for (int cents : grid_int({-1200, 1200})) {
            int te = 0; double cr = 0;
            note("q3_pcm_stage_pitch_plan", q3_pcm_stage_pitch_plan(tempo, cents, &te, &cr));
            note("q3_pcm_stage_pitch_plan", q3_pcm_stage_pitch_plan(tempo, cents, nullptr, nullptr));
        }
    {
        int S1 = 0, S2 = 0;
        must(note("q3_pcm_stage_pitch_tables", q3_pcm_stage_pitch_tables(nullptr, 0, nullptr, 0, &S1, &S2)) == Q3_OK, "pitch table query refused");
        const size_t n1 = 61 * (size_t)S1 + 2, n2 = 64 * (size_t)S2 + 2;
        Buf<float> a(n1), b(n2), a1(n1 - 1), b1(n2 - 1);
        must(note("q3_pcm_stage_pitch_tables", q3_pcm_stage_pitch_tables(a, n1, b, n2, nullptr, nullptr)) == Q3_OK, "pitch tables refused their own sizes");
        must(note("q3_pcm_stage_pitch_tables", q3_pcm_stage_pitch_tables(a, n1, nullptr, 0, nullptr, nullptr)) == Q3_OK, "sinc table alone refused");
        must(note("q3_pcm_stage_pitch_tables", q3_pcm_stage_pitch_tables(nullptr, 0, b, n2, nullptr, nullptr)) == Q3_OK, "window table alone refused");
        must(note("q3_pcm_stage_pitch_tables", q3_pcm_stage_pitch_tables(a1, n1 - 1, b, n2, nullptr, nullptr)) != Q3_OK, "short sinc table taken");
        must(note("q3_pcm_stage_pitch_tables", q3_pcm_stage_pitch_tables(a, n1, b1, n2 - 1, nullptr, nullptr)) != Q3_OK, "short window table taken");
    }
    for (int gain : grid_int({-6000, 2400}))
        for (int ceil_mB : grid_int({-2400, 0})) {
            float g = 0, c = 0;
            note("q3_pcm_stage_level_coeffs", q3_pcm_stage_level_coeffs(gain, ceil_mB, &g, &c));
            note("q3_pcm_stage_level_coeffs", q3_pcm_stage_level_coeffs(gain, ceil_mB, nullptr, nullptr));
        }
}

void sizes_encoders() {
    // (n + 768 - 1024) / 256 + 1 frames: the first clip with a frame is 256 samples long
    for (int64_t n : grid_i64({256, 24000LL * 120, (int64_t)INT32_MAX * 256})) note_value(q3_spk_mel_frames(n) > 0);
    q3_mimi_config dflt, tiny;
    must(q3_mimi_config_default(&dflt) == Q3_OK, "q3_mimi_config_default");
    tiny = dflt; tiny.n_filters = 8; tiny.hidden = 128; tiny.ratios[0] = 2; tiny.ratios[1] = 3; tiny.ratios[2] = 2; tiny.ratios[3] = 4;
    tiny.n_layers = 2; tiny.n_heads = 2; tiny.inter = 96; tiny.window = 7; tiny.cb_size = 64; tiny.cb_dim = 24; tiny.n_q = 5;
    q3_mimi_config zero = dflt; zero.ratios[2] = 0;
    q3_mimi_config neg = dflt; neg.ratios[0] = -4;
    q3_mimi_config wide = dflt; wide.ratios[1] = 17;
    for (int64_t n : grid_i64({1920, 24000LL * 120, (int64_t)INT32_MAX * 1920})) {
        for (const q3_mimi_config* c : {&dflt, &tiny, &zero, &neg, &wide}) {
            Buf<q3_mimi_config> cfg(1); cfg[0] = *c;
            note_value(q3_mimi_frames(cfg, n) > 0);
        }
        note_value(q3_mimi_frames(nullptr, n) > 0);
    }
    // the pack plan: lists of 0, 1, 64 and 65 clips, every clip length of the grid in turn at the front of the list
    for (const q3_mimi_config* c : {&dflt, &tiny, &zero, &neg, &wide})
        for (int n : {0, 1, 64, 65})
            for (int64_t len : grid_i64({1920, 24000LL * 120, (int64_t)INT32_MAX * 1920}))
                for (int64_t pass : grid_i64({24000LL * 120})) {
                    Buf<q3_mimi_config> cfg(1); cfg[0] = *c;
                    Buf<int64_t> ns((size_t)n); Buf<q3_mimi_pack_clip> clips((size_t)n);
                    for (int i = 0; i < n; ++i) ns[(size_t)i] = i == 0 ? len : 24000 + 1000 * i;
                    int64_t fs = 0; int packable = 0, np = 0;
                    const int st = note("q3_mimi_pack_plan", q3_mimi_pack_plan(cfg, ns, n, pass, clips, &fs, &packable, &np));
                    if (st == Q3_OK) {
                        must(np >= 1 && np <= n, "q3_mimi_pack_plan: %d passes for %d clips", np, n);
                        for (int i = 0; i < n; ++i) must(clips[(size_t)i].pass >= 0 && clips[(size_t)i].pass < np && clips[(size_t)i].start >= 0, "q3_mimi_pack_plan: clip %d out of its passes", i);
                    }
                    note("q3_mimi_pack_plan", q3_mimi_pack_plan(cfg, ns, n, pass, clips, nullptr, nullptr, nullptr));
                }
    {
        Buf<int64_t> ns(1); ns[0] = 24000; Buf<q3_mimi_pack_clip> clips(1);
        note("q3_mimi_pack_plan", q3_mimi_pack_plan(nullptr, ns, 1, 24000, clips, nullptr, nullptr, nullptr));
        note("q3_mimi_pack_plan", q3_mimi_pack_plan(&dflt, nullptr, 1, 24000, clips, nullptr, nullptr, nullptr));
        note("q3_mimi_pack_plan", q3_mimi_pack_plan(&dflt, ns, 1, 24000, nullptr, nullptr, nullptr, nullptr));
    }
}

void sizes_session() {
    // q3_prefill_pack_plan: n = 0, 1, the most rows of a session and one more; every length of the grid in turn at the front
    for (int n : {0, 1, Q3_MAX_BATCH, Q3_MAX_BATCH + 1})
        for (int len : grid_int({48, 1024, 128}))
            for (int budget : grid_int({128, 4224}))
                for (int hits = 0; hits < 3; ++hits)                         // no table / no hit / a hit in every third row
                    for (int gemm_ok = 0; gemm_ok < 2; ++gemm_ok) {
                        Buf<int32_t> lengths((size_t)n), hit((size_t)n), pass((size_t)n), row0((size_t)n);
                        for (int i = 0; i < n; ++i) { lengths[(size_t)i] = i == 0 ? len : 48 + 37 * i; hit[(size_t)i] = hits == 2 && i % 3 == 1 ? 1 : 0; }
                        if (hits == 2 && n > 0 && len == -1) hit[0] = -1;
                        int32_t np = 0;
                        const int st = note("q3_prefill_pack_plan", q3_prefill_pack_plan(lengths, hits ? hit.p : nullptr, n, budget, gemm_ok, pass, row0, &np));
                        if (st == Q3_OK)
                            for (int i = 0; i < n; ++i) {
                                must(pass[(size_t)i] >= -1 && pass[(size_t)i] < n, "q3_prefill_pack_plan: row %d in pass %d", i, pass[(size_t)i]);
                                must(row0[(size_t)i] >= 0 && (pass[(size_t)i] < 0 || (long long)row0[(size_t)i] + lengths[(size_t)i] <= budget), "q3_prefill_pack_plan: row %d leaves the budget", i);
                            }
                    }
    {
        Buf<int32_t> one(1); one[0] = 100;
        note("q3_prefill_pack_plan", q3_prefill_pack_plan(nullptr, nullptr, 1, 4224, 1, one, one, nullptr));
        note("q3_prefill_pack_plan", q3_prefill_pack_plan(one, nullptr, 1, 4224, 1, nullptr, one, nullptr));
        note("q3_prefill_pack_plan", q3_prefill_pack_plan(one, nullptr, 1, 4224, 1, one, nullptr, nullptr));
    }
    // q3_prompt_shape: the four prompt kinds; the query, then tables of exactly prefill_len positions, then one short
    for (int kind = 0; kind < 4; ++kind)
        for (size_t n_text_arr : {(size_t)0, (size_t)1, (size_t)13})
            for (size_t n_ins : {(size_t)0, (size_t)1, (size_t)127, (size_t)128, (size_t)129})
                for (size_t n_ref : {(size_t)0, (size_t)1, (size_t)9})
                    for (size_t n_ref_text : {(size_t)0, (size_t)4}) {
                        if (kind != 1 && n_ins > 1) continue;
                        if (kind != 3 && (n_ref > 1 || n_ref_text > 0)) continue;
                        Buf<uint32_t> text(n_text_arr), ins(n_ins), ref(n_ref * 16), ref_text(n_ref_text); Buf<float> xvec(64);
                        const q3_request r = request_of(kind, text, ins, ref, ref_text, xvec);
                        for (int n_text : grid_int({(int)n_text_arr, 1 << 28})) {
                            Buf<q3_prompt_shape_rec> rec(1);
                            if (note("q3_prompt_shape", q3_prompt_shape(&r, n_text, rec, nullptr, nullptr, 0)) != Q3_OK) continue;
                            const int P = rec[0].prefill_len;
                            must(P >= 1 && P < (1 << 29), "q3_prompt_shape: prefill_len %d", P);
                            if (P > (1 << 20)) continue;                      // (tables of a gigabyte prove nothing more)
                            Buf<int> tr((size_t)P), ci((size_t)P), tr1((size_t)P - 1), ci1((size_t)P - 1);
                            must(note("q3_prompt_shape", q3_prompt_shape(&r, n_text, rec, tr, ci, P)) == Q3_OK, "q3_prompt_shape refused tables of its own size");
                            must(note("q3_prompt_shape", q3_prompt_shape(&r, n_text, rec, tr1, ci1, P - 1)) != Q3_OK, "q3_prompt_shape took short tables");
                            note("q3_prompt_shape", q3_prompt_shape(&r, n_text, rec, tr, nullptr, P));
                        }
                    }
    {
        Buf<uint32_t> z(0); Buf<float> xv(64); Buf<q3_prompt_shape_rec> rec(1);
        q3_request r = request_of(1, z, z, z, z, xv);
        for (int v : grid_int({1 << 28})) {
            q3_request q = r; q.n_instruct = v; note("q3_prompt_shape", q3_prompt_shape(&q, 1, rec, nullptr, nullptr, 0));
            q = r; q.mode = Q3_MODE_VOICE_CLONE; q.n_ref = v; note("q3_prompt_shape", q3_prompt_shape(&q, 1, rec, nullptr, nullptr, 0));
            q = r; q.mode = Q3_MODE_VOICE_CLONE; q.n_ref_text = v; note("q3_prompt_shape", q3_prompt_shape(&q, 1, rec, nullptr, nullptr, 0));
            q = r; q.mode = v; note("q3_prompt_shape", q3_prompt_shape(&q, 1, rec, nullptr, nullptr, 0));
            q = r; q.opts.max_length = v; note("q3_prompt_shape", q3_prompt_shape(&q, 1, rec, nullptr, nullptr, 0));
        }
        note("q3_prompt_shape", q3_prompt_shape(nullptr, 1, rec, nullptr, nullptr, 0));
        note("q3_prompt_shape", q3_prompt_shape(&r, 1, nullptr, nullptr, nullptr, 0));
    }
    // q3_sample_row
    for (double temp : {0.0, 1e-9, 0.9, 1.0, 1e30, -1.0, (double)NAN, (double)INFINITY})
        for (double top_p : {0.0, 0.9, 1.0, 1.5, -0.5, (double)NAN})
            for (double rep : {0.0, 1.0, 1.05, 1.5, -2.0, (double)NAN, (double)INFINITY})
                for (int top_k : grid_int({50, 4096})) {
                    Buf<q3_options> o(1); Buf<q3_sample_rec> rec(1);
                    o[0].temperature = temp; o[0].top_p = top_p; o[0].repetition_penalty = rep; o[0].top_k = top_k;
                    o[0].max_length = 2048; o[0].eos_token_id = top_k % 2 ? -1 : 2150; o[0].chunk_frames = 10; o[0].min_new_tokens = top_k;
                    note("q3_sample_row", q3_sample_row(o, rec));
                }
    { Buf<q3_options> o(1); Buf<q3_sample_rec> rec(1); note("q3_sample_row", q3_sample_row(nullptr, rec)); note("q3_sample_row", q3_sample_row(o, nullptr)); }
    for (int v : grid_int({2})) { Buf<q3_config> c(1); note("q3_config_default", q3_config_default(v, c)); }
    note("q3_config_default", q3_config_default(0, nullptr));
}

void sizes_paths() {
    // the launchers' decision functions: every code they return must have a name
    auto conv = [&](int cout, int cin, int L, int k, int dil, int phases, int packed, int resid, int planes, int al) {
        const int code = q3_conv_path(cout, cin, L, k, dil, phases, packed, resid, planes, al);
        note_value(code != 0);
        const char* nm = q3_conv_path_name(code);
        must(nm && *nm, "q3_conv_path_name(%d) is empty", code);
    };
    const int dims[] = {0, 1, -1, 2, 7, 16, 17, 64, 96, 128, 512, 1536, 65535, 65536, INT_MAX, INT_MIN};
    for (int cout : dims) for (int cin : dims) for (int L : {0, 1, 127, 128, 1920, INT_MAX, -1})
        for (int k : {0, 1, 3, 7, 16, -1, INT_MAX}) conv(cout, cin, L, k, 1, 1, 1, 0, 3, 1);
    for (int dil : grid_int({9, 27})) for (int phases : grid_int({8, 16})) for (int packed = 0; packed < 2; ++packed)
        for (int resid = 0; resid < 2; ++resid) for (int planes : grid_int({2, 3})) for (int al = 0; al < 2; ++al) {
            conv(512, 512, 640, 7, dil, 1, packed, resid, planes, al);
            conv(96, 192, 640, 2, 1, phases, packed, resid, planes, al);
        }
    for (int C : dims) for (int L : {0, 1, 128, 1920, INT_MAX, -1}) for (int dil : grid_int({9})) for (int packed = 0; packed < 2; ++packed)
        for (int yx = 0; yx < 2; ++yx) for (int planes : {0, 2, 3, 4}) note_value(q3_resunit_path(C, L, dil, packed, yx, planes) != 0);
    for (int code : grid_int({16, 31, 32, 64, 128, 256, 511, 512})) { const char* nm = q3_conv_path_name(code); must(nm != nullptr, "q3_conv_path_name(%d) is null", code); note_value(true); }
    const int mnk[] = {0, 1, -1, 16, 127, 128, 129, 1024, 2048, 6144, 8192, 1 << 20, INT_MAX, INT_MIN};
    for (int M : mnk) for (int N : mnk) for (int K : mnk) for (int epi : {-1, 0, 1, 2, 3, 4})
        for (int flags = 0; flags < 8; ++flags) {
            Buf<int> path(4);
            note_value(q3_gemm_path(M, N, K, epi, flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, (M & 1) ? nullptr : path.p) >= 0);
        }
    for (int nh : grid_int({2, 16, 32, 64})) for (int nkv : grid_int({1, 8, 16})) for (int pl : {0, 1}) for (int halves : grid_int({1, 2})) {
        Buf<int> path(2);
        note_value(q3_attn_prefill_path(nh, nkv, pl, halves, path) >= 0);
        note_value(q3_attn_prefill_path(nh, nkv, pl, halves, nullptr) >= 0);
    }
    for (int hd : grid_int({64, 128})) for (int kernel : grid_int({2})) note_value(q3_attn_c_path(hd, kernel) >= 0);
}

int cmd_sizes() {
    sizes_pcm_stage();
    sizes_encoders();
    sizes_session();
    sizes_paths();
    return finish("sizes");
}

}  // namespace

int cmd_files(const char* dir);
int cmd_dsp();
int cmd_refusals();

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    // never on a GPU: with a device visible nothing else is called (-1 is the library's answer where there is no driver either)
    const int ndev = q3_device_count();
    if (ndev > 0) {
        printf("SKIP: q3_device_count() = %d: the host-sanitizer harness runs only where there is no device\n", ndev);
        return EXIT_HAS_DEVICE;
    }
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "sizes") return cmd_sizes();
    if (cmd == "files" && argc > 2) return cmd_files(argv[2]);
    if (cmd == "dsp") return cmd_dsp();
    if (cmd == "refusals") return cmd_refusals();
    fprintf(stderr, "usage: %s sizes | files <scratch directory> | dsp | refusals\n", argv[0]);
    return 2;
}

// ================================================================================================================================
// files: the readers, over seeds and their mutants in a scratch directory
// ================================================================================================================================
namespace {

typedef std::vector<uint8_t> Bytes;
std::string g_dir;

void put16(Bytes& b, uint32_t v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
void put32(Bytes& b, uint32_t v) { put16(b, v & 0xFFFF); put16(b, v >> 16); }
void put64(Bytes& b, uint64_t v) { put32(b, (uint32_t)v); put32(b, (uint32_t)(v >> 32)); }
void put_tag(Bytes& b, const char* t) { b.insert(b.end(), t, t + 4); }
void set32(Bytes& b, size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) b[at + (size_t)i] = (uint8_t)(v >> (8 * i)); }
uint32_t get32(const Bytes& b, size_t at) { return (uint32_t)b[at] | ((uint32_t)b[at + 1] << 8) | ((uint32_t)b[at + 2] << 16) | ((uint32_t)b[at + 3] << 24); }
uint32_t g_lcg = 12345;
uint8_t rnd8() { g_lcg = g_lcg * 1664525u + 1013904223u; return (uint8_t)(g_lcg >> 24); }

std::string path_of(const char* name) { return g_dir + "/" + name; }
void write_file(const std::string& path, const uint8_t* p, size_t n) {
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
    if (fd < 0) die("cannot create %s", path.c_str());
    size_t at = 0;
    while (at < n) { const ssize_t w = write(fd, p + at, n - at); if (w <= 0) die("cannot write %s", path.c_str()); at += (size_t)w; }
    close(fd);
}
void write_file(const std::string& path, const Bytes& b) { write_file(path, b.data(), b.size()); }
void write_text(const std::string& path, const std::string& t) { write_file(path, (const uint8_t*)t.data(), t.size()); }
Bytes read_back(const std::string& path) {
    Bytes b; FILE* f = fopen(path.c_str(), "rb");
    if (!f) die("cannot read back %s", path.c_str());
    uint8_t buf[4096]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

// ---- the mutants of a seed: `header` bytes at the front are its header region; len_at: where 32-bit lengths lie ----
const uint8_t VALS[5] = {0, 1, 0x7f, 0x80, 0xff};
void header_mutants(const Bytes& seed, size_t header, const std::vector<size_t>& len_at, bool truncations, const std::function<void(const Bytes&)>& run) {
    run(seed);
    if (truncations) {                                           // every length up to the end of the header region, and at the end
        for (size_t n = 0; n <= header && n < seed.size(); ++n) run(Bytes(seed.begin(), seed.begin() + (long)n));
        for (size_t cut = 1; cut <= 9 && cut < seed.size(); ++cut) run(Bytes(seed.begin(), seed.end() - (long)cut));
    }
    for (size_t i = 0; i < header; ++i)
        for (uint8_t v : VALS) {
            if (seed[i] != v) { Bytes m = seed; m[i] = v; run(m); }
            if (i + 1 < header) { Bytes m = seed; m[i] = v; m[i + 1] = v; run(m); }
        }
    // lengths that lie, in both directions
    for (size_t at : len_at) {
        const uint32_t len = get32(seed, at), rest = (uint32_t)(seed.size() - at - 4);
        for (uint32_t v : {0u, len - 1, len + 1, len + 2, len / 2, rest - 1, rest, rest + 1, rest + 2, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu}) {
            Bytes m = seed; set32(m, at, v); run(m);
        }
    }
}

// ---- WAV ----
struct WavSeed { const char* name; int tag, bits, ch; bool ext; };
const WavSeed WAV_SEEDS[] = {
    {"pcm8", 1, 8, 1, false}, {"pcm16", 1, 16, 2, false}, {"pcm24", 1, 24, 2, false}, {"pcm32", 1, 32, 1, false}, {"float", 3, 32, 2, false},
    {"ulaw", 7, 8, 1, false}, {"alaw", 6, 8, 2, false}, {"ext16", 1, 16, 2, true}, {"extfloat", 3, 32, 1, true}};
// RIFF | fmt (16 bytes; 18 for G.711; 40 extensible) | an odd-length LIST chunk | data. data_bytes = 0: a page-aligned file.
Bytes wav_build(const WavSeed& s, uint32_t rate, size_t data_bytes, bool data_first = false) {
    Bytes fmt;
    const int fb = s.bits / 8 * s.ch;
    put16(fmt, s.ext ? 0xFFFE : (uint32_t)s.tag); put16(fmt, (uint32_t)s.ch); put32(fmt, rate); put32(fmt, rate * (uint32_t)fb); put16(fmt, (uint32_t)fb); put16(fmt, (uint32_t)s.bits);
    if (s.ext) {
        put16(fmt, 22); put16(fmt, (uint32_t)s.bits); put32(fmt, s.ch == 2 ? 3 : 4);
        put16(fmt, (uint32_t)s.tag); for (uint8_t g : {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71}) fmt.push_back(g);
    } else if (s.tag == 7 || s.tag == 6) put16(fmt, 0);
    const size_t front = 12 + 8 + fmt.size() + 8 + 5 + 1 + 8;
    if (data_bytes == 0) data_bytes = PAGE - front;
    Bytes data(data_bytes); for (auto& v : data) v = rnd8();
    Bytes b;
    put_tag(b, "RIFF"); put32(b, 0); put_tag(b, "WAVE");
    auto put_fmt = [&] { put_tag(b, "fmt "); put32(b, (uint32_t)fmt.size()); b.insert(b.end(), fmt.begin(), fmt.end()); };
    auto put_data = [&] { put_tag(b, "data"); put32(b, (uint32_t)data.size()); b.insert(b.end(), data.begin(), data.end()); if (data_first && (data.size() & 1)) b.push_back(0); };
    if (data_first) { put_data(); put_fmt(); }
    else { put_fmt(); put_tag(b, "LIST"); put32(b, 5); for (int i = 0; i < 5; ++i) b.push_back((uint8_t)('a' + i)); b.push_back(0); put_data(); }
    set32(b, 4, (uint32_t)(b.size() - 8));
    return b;
}
// where a RIFF file's 32-bit lengths lie, and where its data chunk's body starts (the end of the header region)
void wav_layout(const Bytes& b, std::vector<size_t>* len_at, size_t* header) {
    len_at->clear(); len_at->push_back(4);
    *header = b.size();
    size_t off = 12;
    while (off + 8 <= b.size()) {
        len_at->push_back(off + 4);
        if (memcmp(&b[off], "data", 4) == 0) { *header = off + 8; return; }
        const uint32_t len = get32(b, off + 4);
        off += 8 + (size_t)len + (len & 1);
    }
}
void read_wav(const Bytes& file) {
    const std::string path = path_of("m.wav");
    write_file(path, file);
    const int64_t fsize = (int64_t)file.size();
    Buf<q3_wav_desc> d(1);
    if (note("q3_wav_info", q3_wav_info(path.c_str(), d)) == Q3_OK) {
        const q3_wav_desc& w = d[0];
        must(w.channels >= 1 && w.bits >= 8 && w.frames >= 0 && w.data_offset >= 12 && w.data_bytes >= 0, "q3_wav_info: impossible record");
        must(w.frames * (int64_t)(w.bits / 8) * w.channels == w.data_bytes, "q3_wav_info: %lld frames are not %lld bytes", (long long)w.frames, (long long)w.data_bytes);
        must(w.data_offset + w.data_bytes <= fsize, "q3_wav_info: samples at %lld + %lld leave a file of %lld bytes", (long long)w.data_offset, (long long)w.data_bytes, (long long)fsize);
    }
    int64_t n = -1; uint32_t sr = 0;
    if (note("q3_wav_read", q3_wav_read(path.c_str(), nullptr, 0, &n, &sr)) != Q3_OK) return;
    must(n >= 0 && n <= fsize, "q3_wav_read: %lld samples from %lld bytes", (long long)n, (long long)fsize);
    Buf<float> out((size_t)n);
    int64_t n2 = -1;
    must(note("q3_wav_read", q3_wav_read(path.c_str(), out, n, &n2, &sr)) == Q3_OK && n2 == n, "q3_wav_read refused a buffer of its own count");
    if (n > 0) { Buf<float> shrt((size_t)n - 1); must(note("q3_wav_read", q3_wav_read(path.c_str(), shrt, n - 1, &n2, nullptr)) != Q3_OK, "q3_wav_read took a short buffer"); }
}
void files_wav() {
    std::vector<Bytes> seeds; std::vector<bool> aligned;
    for (const WavSeed& s : WAV_SEEDS) {
        seeds.push_back(wav_build(s, 16000, (size_t)(s.bits / 8 * s.ch) * 37)); aligned.push_back(false);
        seeds.push_back(wav_build(s, 44100, 0)); aligned.push_back(true);
        must(seeds.back().size() == PAGE, "page-aligned %s seed has %zu bytes", s.name, seeds.back().size());
        // `data` in front of `fmt `
        read_wav(wav_build(s, 16000, (size_t)(s.bits / 8 * s.ch) * 37, true));
    }
    // the library's own writers: 41 samples (an odd byte count for G.711: a pad byte), and as many as end a file on a page
    {
        Buf<float> x(2026); for (size_t i = 0; i < x.n; ++i) x[i] = (float)rnd8() / 128.0f - 1.0f;
        Buf<uint8_t> g(4038); for (size_t i = 0; i < g.n; ++i) g[i] = rnd8();
        const std::string p = path_of("seed.wav");
        must(note("q3_wav_write_pcm16", q3_wav_write_pcm16(p.c_str(), x, 41, 24000)) == Q3_OK, "q3_wav_write_pcm16"); seeds.push_back(read_back(p)); aligned.push_back(false);
        must(note("q3_wav_write_pcm16", q3_wav_write_pcm16(p.c_str(), x, 2026, 24000)) == Q3_OK, "q3_wav_write_pcm16"); seeds.push_back(read_back(p)); aligned.push_back(true);
        must(seeds.back().size() == PAGE, "q3_wav_write_pcm16's page seed has %zu bytes", seeds.back().size());
        for (int law : {(int)Q3_PCM_ULAW, (int)Q3_PCM_ALAW}) {
            must(note("q3_wav_write_g711", q3_wav_write_g711(p.c_str(), g, 41, 8000, law)) == Q3_OK, "q3_wav_write_g711"); seeds.push_back(read_back(p)); aligned.push_back(false);
            must(note("q3_wav_write_g711", q3_wav_write_g711(p.c_str(), g, 4038, 8000, law)) == Q3_OK, "q3_wav_write_g711"); seeds.push_back(read_back(p)); aligned.push_back(true);
            must(seeds.back().size() == PAGE, "q3_wav_write_g711's page seed has %zu bytes", seeds.back().size());
        }
    }
    for (size_t i = 0; i < seeds.size(); ++i) {
        std::vector<size_t> len_at; size_t header = 0;
        wav_layout(seeds[i], &len_at, &header);
        must(header < seeds[i].size(), "seed %zu has no data chunk", i);
        // (a truncated page-aligned file no longer ends on the boundary: truncations go to the other form)
        header_mutants(seeds[i], header, len_at, !aligned[i], read_wav);
    }
    Buf<q3_wav_desc> d(1); int64_t n = 0;
    note("q3_wav_info", q3_wav_info(path_of("absent.wav").c_str(), d));
    note("q3_wav_info", q3_wav_info(nullptr, d));
    note("q3_wav_info", q3_wav_info(path_of("m.wav").c_str(), nullptr));
    note("q3_wav_read", q3_wav_read(path_of("absent.wav").c_str(), nullptr, 0, &n, nullptr));
    note("q3_wav_read", q3_wav_read(nullptr, nullptr, 0, &n, nullptr));
    note("q3_wav_read", q3_wav_read(path_of("m.wav").c_str(), nullptr, 0, nullptr, nullptr));
    note("q3_wav_info", q3_wav_info(g_dir.c_str(), d));                    // a directory
}

// ---- JSON texts that try the parser ----
std::string nested(int depth) { return std::string((size_t)depth, '[') + "1" + std::string((size_t)depth, ']'); }
std::vector<std::string> json_values() {
    return {nested(63), nested(64), nested(65), nested(4000), "\"\\ud800\"", "\"\\ud83d\\ude00\"", "\"\\ude00\\ud83d\"", "\"\\ud800\\u0041\"", "\"\\ud800\\ud800\"",
            "\"\\udbff\\udfff\"", "\"\\ud800\\u\"", "\"\\x41\"", "\"\\u12\"", "\"\\u12G4\"", "\"\\", "\"\\u", "\"unterminated", "\"\\ud800\\", "9223372036854775807",
            "9223372036854775808", "-9223372036854775809", "18446744073709551616", "123456789012345678901234567890", "1e999", "-1e999", "-0", "1E+2", "-", "1e", "1.",
            "4294968320", "2147483648", "-1", "0.5", "tru", "nul", "{\"a\":1,\"a\":2}", "[1,]", "{,}", "{\"a\"}", "", " ", "\x01", "\xff\xfe"};
}

// ---- safetensors ----
struct StTensor { std::string name, dtype; std::string shape; uint64_t b, e; };
// header text of the entries (shape as JSON text, so that a mutant can say anything), padded with spaces to a multiple of 64
std::string st_header(const std::vector<StTensor>& ts, const std::string& extra = "") {
    std::string h = "{\"__metadata__\":{\"format\":\"pt\",\"note\":\"\\u00e9\"}";
    for (const StTensor& t : ts)
        h += ",\"" + t.name + "\":{\"dtype\":\"" + t.dtype + "\",\"shape\":" + t.shape + ",\"data_offsets\":[" + std::to_string(t.b) + "," + std::to_string(t.e) + "]}";
    h += extra + "}";
    while ((h.size() + 8) % 64) h += ' ';
    return h;
}
Bytes st_file(const std::string& header, size_t data_bytes) {
    Bytes b; put64(b, header.size());
    b.insert(b.end(), header.begin(), header.end());
    for (size_t i = 0; i < data_bytes; ++i) b.push_back(rnd8());
    return b;
}
int dt_bytes(const std::string& d) { return d == "F32" ? 4 : d == "F64" ? 8 : 2; }
// entries of n[i] elements of dtypes[i], laid end to end; the last one grows until the file ends on a page when `aligned`
Bytes st_build(const std::vector<std::string>& names, const std::vector<std::string>& dtypes, std::vector<int64_t> n, bool aligned, size_t* header_end,
               std::vector<StTensor>* out = nullptr) {
    for (int round = 0; round < 4; ++round) {
        std::vector<StTensor> ts; uint64_t at = 0;
        for (size_t i = 0; i < names.size(); ++i) {
            const uint64_t bytes = (uint64_t)n[i] * (uint64_t)dt_bytes(dtypes[i]);
            ts.push_back({names[i], dtypes[i], "[" + std::to_string(n[i]) + "]", at, at + bytes});
            at += bytes;
        }
        const std::string h = st_header(ts);
        const size_t total = 8 + h.size() + (size_t)at;
        if (!aligned || total % PAGE == 0) { *header_end = 8 + h.size(); if (out) *out = ts; return st_file(h, (size_t)at); }
        const size_t want = (total + PAGE - 1) / PAGE * PAGE, es = (size_t)dt_bytes(dtypes.back());
        must((want - total) % es == 0, "cannot page-align a safetensors seed");
        n.back() += (int64_t)((want - total) / es);
    }
    die("safetensors seed does not settle on a page");
}
void read_st_info(const Bytes& file, const std::vector<std::string>& names) {
    const std::string path = path_of("m.safetensors");
    write_file(path, file);
    for (const std::string& nm : names) {
        int dtype = 0, nd = -1;
        if (note("q3_safetensors_info", q3_safetensors_info(path.c_str(), nm.c_str(), &dtype, nullptr, 0, &nd)) != Q3_OK) continue;
        must(nd >= 0 && nd <= (int)file.size() && dtype >= -1 && dtype <= Q3_DTYPE_BF16, "q3_safetensors_info: rank %d dtype %d", nd, dtype);
        Buf<int64_t> shape((size_t)nd);
        must(note("q3_safetensors_info", q3_safetensors_info(path.c_str(), nm.c_str(), nullptr, shape, nd, nullptr)) == Q3_OK, "q3_safetensors_info refused its own rank");
        for (int i = 0; i < nd; ++i) must(shape[(size_t)i] >= 0, "q3_safetensors_info: negative dim");
        if (nd > 0) { Buf<int64_t> s1((size_t)nd - 1); note("q3_safetensors_info", q3_safetensors_info(path.c_str(), nm.c_str(), &dtype, s1, nd - 1, &nd)); }
    }
}
void files_safetensors() {
    const std::vector<std::string> names = {"a.f32", "b.bf16", "c.f16", "d.f64", "e.f32"}, dtypes = {"F32", "BF16", "F16", "F64", "F32"};
    std::vector<std::string> ask = names; ask.push_back("absent"); ask.push_back("__metadata__"); ask.push_back("");
    for (int aligned = 0; aligned < 2; ++aligned) {
        size_t header = 0;
        const Bytes seed = st_build(names, dtypes, {12, 4, 8, 7, 3}, aligned != 0, &header);
        must(!aligned || seed.size() % PAGE == 0, "safetensors seed of %zu bytes", seed.size());
        header_mutants(seed, header, {0, 4}, !aligned, [&](const Bytes& b) { read_st_info(b, ask); });
    }
    // headers that try the JSON parser: each text as the whole header, as a tensor's entry, as its shape and as its offsets
    for (const std::string& v : json_values()) {
        read_st_info(st_file(v, 64), ask);
        read_st_info(st_file("{\"a.f32\":" + v + "}", 64), ask);
        read_st_info(st_file("{\"a.f32\":{\"dtype\":\"F32\",\"shape\":" + v + ",\"data_offsets\":[0,48]}}", 64), ask);
        read_st_info(st_file("{\"a.f32\":{\"dtype\":\"F32\",\"shape\":[" + v + "],\"data_offsets\":[0,48]}}", 64), ask);
        read_st_info(st_file("{\"a.f32\":{\"dtype\":\"F32\",\"shape\":[12],\"data_offsets\":" + v + "}}", 64), ask);
        read_st_info(st_file("{\"a.f32\":{\"dtype\":\"F32\",\"shape\":[12],\"data_offsets\":[0," + v + "]}}", 64), ask);
        read_st_info(st_file("{\"a.f32\":{\"dtype\":" + v + ",\"shape\":[12],\"data_offsets\":[0,48]}}", 64), ask);
        read_st_info(st_file("{" + v + ":{\"dtype\":\"F32\",\"shape\":[12],\"data_offsets\":[0,48]}}", 64), ask);
    }
    // offsets that are negative, reversed or beyond the file
    for (const char* off : {"[-1,48]", "[48,0]", "[0,65]", "[64,64]", "[65,65]", "[0,1000000000000]", "[0]", "[0,48,64]", "[0.0,48]", "[\"0\",\"48\"]", "[null,48]"})
        read_st_info(st_file(std::string("{\"a.f32\":{\"dtype\":\"F32\",\"shape\":[12],\"data_offsets\":") + off + "}}", 64), ask);
    int dtype = 0, nd = 0;
    note("q3_safetensors_info", q3_safetensors_info(nullptr, "a", &dtype, nullptr, 0, &nd));
    note("q3_safetensors_info", q3_safetensors_info(path_of("m.safetensors").c_str(), nullptr, &dtype, nullptr, 0, &nd));
    note("q3_safetensors_info", q3_safetensors_info(path_of("absent.safetensors").c_str(), "a", &dtype, nullptr, 0, &nd));
}

// ---- the model loaders: q3_model_load over a directory (device -1: the manifest alone), and q3_model_load_safetensors into a
// manifest-only handle, which walks a file's entries through every host check of an upload (shape product, byte range, the
// f16 / f64 conversions over the mapped bytes) before the handle refuses the tensor itself ----
q3_config tiny_config() {
    q3_config c;
    must(q3_config_default(0, &c) == Q3_OK, "q3_config_default");
    c.text_dim = 32; c.hidden = 64; c.inter = 128; c.n_layers = 2; c.n_heads = 2; c.n_kv_heads = 1;
    c.cp_hidden = 32; c.cp_inter = 64; c.cp_layers = 2; c.cp_heads = 2; c.cp_kv_heads = 1;
    c.dec_cb_dim = 16; c.dec_q_dim = 32; c.dec_latent = 64; c.dec_hidden = 32; c.dec_layers = 2; c.dec_heads = 2; c.dec_inter = 64; c.dec_dim = 96;
    return c;
}
const char* CONFIG_17B =
    "{\n  \"architectures\": [\"Qwen3TTSForConditionalGeneration\"],\n  \"tts_model_type\": \"custom_voice\",\n  \"tts_model_size\": \"1.7B\",\n"
    "  \"speaker_encoder_config\": {\"mel_dim\": 128, \"enc_dim\": 2048, \"enc_channels\": [512, 512, 512, 512, 1536], \"enc_kernel_sizes\": [5, 3, 3, 3, 1],\n"
    "    \"enc_dilations\": [1, 2, 3, 4, 1], \"enc_attention_channels\": 128, \"enc_res2net_scale\": 8, \"enc_se_channels\": 128, \"sample_rate\": 24000},\n"
    "  \"talker_config\": {\n    \"hidden_size\": 2048, \"intermediate_size\": 6144, \"num_hidden_layers\": 28, \"num_attention_heads\": 16,\n"
    "    \"num_key_value_heads\": 8, \"head_dim\": 128, \"vocab_size\": 3072, \"text_vocab_size\": 151936, \"text_hidden_size\": 2048,\n"
    "    \"rms_norm_eps\": 1e-06, \"rope_theta\": 1000000, \"spk_id\": {\"vivian\": 3065, \"ryan\": 3061},\n"
    "    \"code_predictor_config\": {\"hidden_size\": 1024, \"intermediate_size\": 3072, \"num_hidden_layers\": 5, \"num_attention_heads\": 16,\n"
    "      \"num_key_value_heads\": 8, \"head_dim\": 128, \"vocab_size\": 2048, \"num_code_groups\": 16, \"rms_norm_eps\": 1e-06, \"rope_theta\": 1000000}\n  }\n}\n";
void read_config(const std::string& text) {
    const std::string path = path_of("m.json");
    write_text(path, text);
    Buf<q3_config> c(1); int mt = -1;
    if (note("q3_config_from_json", q3_config_from_json(path.c_str(), c, &mt)) == Q3_OK) must(mt >= Q3_MODEL_BASE && mt <= Q3_MODEL_VOICE_DESIGN, "q3_config_from_json: model type %d", mt);
    note("q3_config_from_json", q3_config_from_json(path.c_str(), c, nullptr));
    Buf<q3_spk_config> sc(1); int present = -1;
    if (note("q3_spk_config_from_json", q3_spk_config_from_json(path.c_str(), sc, &present)) == Q3_OK) must(present == 0 || present == 1, "q3_spk_config_from_json: present %d", present);
}
void files_config() {
    const std::string seed = CONFIG_17B;
    {
        const std::string path = path_of("m.json"); write_text(path, seed);
        Buf<q3_config> c(1); int mt = -1;
        must(note("q3_config_from_json", q3_config_from_json(path.c_str(), c, &mt)) == Q3_OK && c[0].hidden == 2048 && c[0].inter == 6144 && c[0].cp_hidden == 1024 && mt == Q3_MODEL_CUSTOM_VOICE,
             "the 1.7B-shaped config.json does not parse as one");
    }
    for (size_t n = 0; n <= seed.size(); ++n) read_config(seed.substr(0, n));
    for (size_t i = 0; i < seed.size(); ++i)
        for (uint8_t v : VALS) {
            std::string m = seed; m[i] = (char)v; read_config(m);
            if (i + 1 < seed.size()) { m[i + 1] = (char)v; read_config(m); }
        }
    for (const std::string& v : json_values()) {
        read_config(v);
        read_config("{\"talker_config\":" + v + "}");
        read_config("{\"tts_model_type\":" + v + ",\"talker_config\":{\"hidden_size\":" + v + ",\"rms_norm_eps\":" + v + ",\"code_predictor_config\":{\"head_dim\":" + v + "}}}");
        read_config("{\"speaker_encoder_config\":{\"mel_dim\":" + v + ",\"enc_channels\":" + v + "}}");
        read_config("{\"speaker_encoder_config\":{\"enc_channels\":[1,2,3,4," + v + "],\"enc_dilations\":[" + v + "]}}");
        read_config("{\"speaker_encoder_config\":" + v + "}");
        read_config("{\"a\":" + v + ",\"a\":" + v + ",\"talker_config\":{\"hidden_size\":64},\"talker_config\":{\"hidden_size\":128}}");
    }
    Buf<q3_config> c(1); Buf<q3_spk_config> sc(1);
    note("q3_config_from_json", q3_config_from_json(nullptr, c, nullptr));
    note("q3_config_from_json", q3_config_from_json(path_of("m.json").c_str(), nullptr, nullptr));
    note("q3_config_from_json", q3_config_from_json(path_of("absent.json").c_str(), c, nullptr));
    note("q3_spk_config_from_json", q3_spk_config_from_json(nullptr, sc, nullptr));
    note("q3_spk_config_from_json", q3_spk_config_from_json(path_of("m.json").c_str(), nullptr, nullptr));
    note("q3_spk_config_from_json", q3_spk_config_from_json(path_of("absent.json").c_str(), sc, nullptr));
}

void files_model() {
    const q3_config cfg = tiny_config();
    q3_model* m = nullptr;
    must(note("q3_model_create", q3_model_create(&cfg, -1, &m)) == Q3_OK && m, "no manifest-only handle for the tiny configuration");
    // the first small tensors of the manifest (counts that are multiples of 4), and the one weight inspection looks for
    std::vector<std::string> names; std::vector<int64_t> counts;
    const int nt = q3_model_n_tensors(m);
    must(nt > 0, "empty manifest");
    for (int i = 0; i < nt && names.size() < 4; ++i) {
        const char* nm = nullptr; int64_t n = 0; int stored = 0;
        must(note("q3_model_tensor_info", q3_model_tensor_info(m, i, &nm, &n, &stored)) == Q3_OK, "q3_model_tensor_info(%d)", i);
        if (n >= 4 && n <= 4096 && n % 4 == 0 && strcmp(nm, "talker.model.norm.weight") != 0) { names.push_back(nm); counts.push_back(n); }
    }
    must(names.size() == 4, "the tiny manifest has fewer than four small tensors");
    names.push_back("talker.model.norm.weight"); counts.push_back(cfg.hidden);
    const std::vector<std::string> dtypes = {"F32", "BF16", "F16", "F64", "F32"};
    const std::string path = path_of("m.safetensors");
    auto load = [&](const Bytes& file) -> int {
        write_file(path, file);
        int n_loaded = -1;
        const int st = note("q3_model_load_safetensors", q3_model_load_safetensors(m, path.c_str(), &n_loaded));
        must(st != Q3_OK || n_loaded == 0, "a manifest-only handle took %d tensors", n_loaded);
        return st;
    };
    std::vector<StTensor> ts;
    for (int aligned = 0; aligned < 2; ++aligned) {
        size_t header = 0;
        // (a manifest-only handle answers the first tensor it is handed: of these files the first entry in manifest order is the one
        // that is checked; every entry gets a file of its own below)
        const Bytes seed = st_build(names, dtypes, counts, aligned != 0, &header, aligned ? nullptr : &ts);
        must(!aligned || seed.size() % PAGE == 0, "model seed of %zu bytes", seed.size());
        must(load(seed) == Q3_UNSUPPORTED, "a manifest-only handle must answer a well-formed file with Q3_UNSUPPORTED");
        header_mutants(seed, header, {0, 4}, !aligned, [&](const Bytes& b) { load(b); });
    }
    // each entry alone, in each dtype, so that the conversions run over a tensor that ends the file on a page
    for (size_t i = 0; i < names.size(); ++i)
        for (const char* dt : {"F32", "BF16", "F16", "F64", "I64", ""}) {
            const int es = dt_bytes(dt);
            const int64_t per_page = (int64_t)PAGE / es;
            const int64_t n = counts[i];
            // the entry's bytes end the file, and the file ends on a page: pad in front with a filler tensor
            std::vector<StTensor> one = {{"filler", "F32", "[1]", 0, 0}, {names[i], dt, "[" + std::to_string(n) + "]", 0, 0}};
            for (int round = 0; round < 3; ++round) {
                const std::string h = st_header(one);
                const size_t body = (size_t)(n * es), total = 8 + h.size() + body;
                const size_t fill = (PAGE - total % PAGE) % PAGE;
                one[0].shape = "[" + std::to_string(fill / 4) + "]"; one[0].b = 0; one[0].e = fill;
                one[1].b = fill; one[1].e = fill + body;
                if (fill % 4) die("filler of %zu bytes", fill);
            }
            const std::string h = st_header(one);
            const Bytes f = st_file(h, (size_t)one[1].e);
            (void)per_page;
            if (f.size() % PAGE == 0) load(f);
        }
    // shapes: products beyond 2^63, one that wraps to the expected count, and counts that do not match
    for (size_t i = 0; i < names.size(); ++i) {
        const int64_t n = counts[i];
        int t = 0; while (((n >> t) & 1) == 0) ++t;                           // n = 2^t * odd, t >= 2
        const uint64_t wrap_b = (1ull << (64 - t)) + (uint64_t)(n >> t);        // 2^t * wrap_b = 2^64 + n
        const std::string sn = std::to_string(n);
        const uint64_t bytes = (uint64_t)n * (uint64_t)dt_bytes(dtypes[i]);
        // (one entry per file: a manifest-only handle answers the first tensor it is handed, so only that one is checked)
        auto alone = [&](const std::string& shape, const char* dt, uint64_t begin) { return StTensor{names[i], dt, shape, begin, begin + (uint64_t)n * (uint64_t)dt_bytes(dt)}; };
        for (const std::string& shape : std::vector<std::string>{std::string("[4294967296,4294967296]"), std::string("[9223372036854775807,3]"), std::string("[3037000500,3037000500]"),
                                         "[" + std::to_string(1ll << t) + "," + std::to_string(wrap_b) + "]", std::string("[2,4611686018427387904]"), "[" + sn + ",9223372036854775807]",
                                         std::string("[9223372036854775807,9223372036854775807,9223372036854775807]"), "[" + sn + ",0,9223372036854775807,9223372036854775807]",
                                         "[" + sn + ",1,1]", std::string("[]"), std::string("[0]"), "[" + std::to_string(n + 1) + "]", "[" + std::to_string(n - 1) + "]"}) {
            load(st_file(st_header({alone(shape, dtypes[i].c_str(), 0)}), (size_t)bytes));
        }
        for (const char* dt : {"F32", "BF16", "F16", "F64", "I64", "f32", ""}) load(st_file(st_header({alone("[" + sn + "]", dt, 0)}), (size_t)n * (size_t)dt_bytes(dt)));
        // a well-formed range at an odd address, in every dtype
        for (const char* dt : {"F32", "BF16", "F16", "F64"}) load(st_file(st_header({alone("[" + sn + "]", dt, 1)}), (size_t)n * (size_t)dt_bytes(dt) + 1));
        for (const char* off : {"[-1,48]", "[48,0]", "[0,1000000000000]", "[0,9223372036854775808]", "[1,17]", "[3,7]"}) {
            std::string h = st_header({alone("[" + sn + "]", dtypes[i].c_str(), 0)});
            const std::string own = "\"data_offsets\":[0," + std::to_string(bytes) + "]";
            const size_t at = h.find(own);
            must(at != std::string::npos, "entry %zu has no offsets in its header", i);
            h.replace(at, own.size(), std::string("\"data_offsets\":") + off);
            load(st_file(h, (size_t)bytes));
        }
    }
    note("q3_model_load_safetensors", q3_model_load_safetensors(nullptr, path.c_str(), nullptr));
    note("q3_model_load_safetensors", q3_model_load_safetensors(m, nullptr, nullptr));
    note("q3_model_load_safetensors", q3_model_load_safetensors(m, path_of("absent.safetensors").c_str(), nullptr));
    q3_model_free(m);

    // q3_model_load with device -1 over a directory: config.json (present, absent, broken), both weight files, either missing
    const std::string dir = path_of("model"), sub = dir + "/speech_tokenizer";
    mkdir(dir.c_str(), 0700); mkdir(sub.c_str(), 0700);
    size_t header = 0;
    const Bytes weights = st_build(names, dtypes, counts, false, &header);
    const std::string w_path = dir + "/model.safetensors", st_path = sub + "/model.safetensors", c_path = dir + "/config.json";
    auto model_load = [&](const char* d, bool expect_ok) {
        q3_model* mm = nullptr; int mt = -7;
        const int st = note("q3_model_load", q3_model_load(d, -1, &mm, &mt));
        if (st == Q3_OK) { must(mm && q3_model_n_tensors(mm) > 0 && mt >= Q3_MODEL_UNKNOWN && mt <= Q3_MODEL_VOICE_DESIGN, "q3_model_load: no manifest (model type %d)", mt); q3_model_free(mm); }
        else must(mm == nullptr, "q3_model_load left a handle behind a failure");
        must(!expect_ok || st == Q3_OK, "q3_model_load refused a well-formed directory: %s", q3_last_error());
    };
    write_file(w_path, weights); write_file(st_path, weights); write_text(c_path, CONFIG_17B);
    model_load(dir.c_str(), true);
    model_load((dir + "/").c_str(), true);
    model_load((dir + "///").c_str(), true);
    unlink(c_path.c_str());
    model_load(dir.c_str(), true);                                          // weight inspection
    for (const char* broken : {"", "{", "[1,2", "{\"talker_config\":{\"hidden_size\":\"x\"}}", "{\"talker_config\":{\"hidden_size\":7}}",
                               "{\"talker_config\":{\"num_key_value_heads\":0}}", "{\"talker_config\":{\"hidden_size\":4294968320}}"}) {
        write_text(c_path, broken);
        model_load(dir.c_str(), false);
    }
    unlink(c_path.c_str());
    // weight inspection over mutated headers (the truncations of the header region, and the lying header length)
    header_mutants(weights, 16, {0, 4}, true, [&](const Bytes& b) { write_file(w_path, b); model_load(dir.c_str(), false); });
    write_file(w_path, weights);
    unlink(st_path.c_str());
    model_load(dir.c_str(), false);                                         // no speech tokenizer here nor beside the directory
    write_file(path_of("speech_tokenizer_probe"), weights);
    unlink(w_path.c_str());
    model_load(dir.c_str(), false);
    model_load(path_of("absent").c_str(), false);
    model_load("", false);
    model_load("/", false);
    { q3_model* mm = nullptr; note("q3_model_load", q3_model_load(nullptr, -1, &mm, nullptr)); note("q3_model_load", q3_model_load(dir.c_str(), -1, nullptr, nullptr)); }
}

// ---- codes_*.bin and audio_*.bin ----
void read_codes(const Bytes& file) {
    const std::string path = path_of("m.bin");
    write_file(path, file);
    for (int groups : {16, 1, 15, 17, 0, -1, INT_MAX, INT_MIN, 512}) {
        int nf = -1;
        if (note("q3_codes_read_bin", q3_codes_read_bin(path.c_str(), nullptr, 0, groups, &nf)) != Q3_OK) continue;
        must(nf >= 0 && (size_t)nf * (size_t)groups * 8 == file.size(), "q3_codes_read_bin: %d frames of %d from %zu bytes", nf, groups, file.size());
        Buf<uint32_t> codes((size_t)nf * (size_t)groups, 0xAB);
        note("q3_codes_read_bin", q3_codes_read_bin(path.c_str(), codes, nf, groups, &nf));
        if (nf > 0) { Buf<uint32_t> shrt((size_t)(nf - 1) * (size_t)groups); must(note("q3_codes_read_bin", q3_codes_read_bin(path.c_str(), shrt, nf - 1, groups, &nf)) != Q3_OK, "q3_codes_read_bin took a short buffer"); }
        { Buf<uint32_t> none(0); note("q3_codes_read_bin", q3_codes_read_bin(path.c_str(), none, -1, groups, &nf)); note("q3_codes_read_bin", q3_codes_read_bin(path.c_str(), none, INT_MIN, groups, &nf)); }
    }
    note("q3_codes_read_bin", q3_codes_read_bin(path.c_str(), nullptr, 0, 16, nullptr));
}
void read_audio(const Bytes& file) {
    const std::string path = path_of("m.bin");
    write_file(path, file);
    int64_t n = -1;
    if (note("q3_audio_read_bin", q3_audio_read_bin(path.c_str(), nullptr, 0, &n)) != Q3_OK) return;
    must(n >= 0 && (size_t)n * 4 == file.size(), "q3_audio_read_bin: %lld samples from %zu bytes", (long long)n, file.size());
    Buf<float> out((size_t)n);
    note("q3_audio_read_bin", q3_audio_read_bin(path.c_str(), out, n, &n));
    if (n > 1) { Buf<float> shrt((size_t)n - 1); must(note("q3_audio_read_bin", q3_audio_read_bin(path.c_str(), shrt, n - 1, &n)) != Q3_OK, "q3_audio_read_bin took a short buffer"); }
    for (int64_t cap : {(int64_t)-1, INT64_MIN, INT64_MAX}) { Buf<float> big((size_t)n); note("q3_audio_read_bin", q3_audio_read_bin(path.c_str(), big, cap, &n)); }
}
void files_bins() {
    const std::string path = path_of("seed.bin");
    for (int nf : {0, 1, 7, 32}) {                                           // 32 frames of 16 codes: exactly one page
        Buf<uint32_t> codes((size_t)nf * 16); for (size_t i = 0; i < codes.n; ++i) codes[i] = (uint32_t)rnd8() * 16777259u;
        must(note("q3_codes_write_bin", q3_codes_write_bin(path.c_str(), codes, nf, 16)) == Q3_OK, "q3_codes_write_bin");
        const Bytes seed = read_back(path);
        must(seed.size() == (size_t)nf * 128, "q3_codes_write_bin wrote %zu bytes", seed.size());
        read_codes(seed);
        if (nf == 7) for (size_t n = 0; n < seed.size(); ++n) read_codes(Bytes(seed.begin(), seed.begin() + (long)n));
        // a code that does not fit u32, in the first and in the last place
        if (nf > 0) for (size_t at : {(size_t)4, (size_t)7, seed.size() - 1, seed.size() - 4}) for (uint8_t v : {(uint8_t)1, (uint8_t)0x80, (uint8_t)0xff}) { Bytes m = seed; m[at] = v; read_codes(m); }
    }
    for (int g : grid_int({16})) for (int nf : grid_int({1})) { Buf<uint32_t> c(16); note("q3_codes_write_bin", q3_codes_write_bin(path.c_str(), c, nf > 1 ? 1 : nf, g > 16 ? 16 : g)); }
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)1024}) {  // 1024 samples: exactly one page
        Buf<float> x((size_t)n); for (size_t i = 0; i < x.n; ++i) x[i] = (float)rnd8();
        must(note("q3_audio_write_bin", q3_audio_write_bin(path.c_str(), x, n)) == Q3_OK, "q3_audio_write_bin");
        const Bytes seed = read_back(path);
        read_audio(seed);
        if (n == 5) for (size_t k = 0; k < seed.size(); ++k) read_audio(Bytes(seed.begin(), seed.begin() + (long)k));
    }
    int64_t n = 0; int nf = 0;
    note("q3_audio_read_bin", q3_audio_read_bin(nullptr, nullptr, 0, &n));
    note("q3_audio_read_bin", q3_audio_read_bin(path.c_str(), nullptr, 0, nullptr));
    note("q3_audio_read_bin", q3_audio_read_bin(path_of("absent.bin").c_str(), nullptr, 0, &n));
    note("q3_codes_read_bin", q3_codes_read_bin(nullptr, nullptr, 0, 16, &nf));
    note("q3_codes_read_bin", q3_codes_read_bin(path_of("absent.bin").c_str(), nullptr, 0, 16, &nf));
    note("q3_audio_write_bin", q3_audio_write_bin(path.c_str(), nullptr, 1));
    note("q3_audio_write_bin", q3_audio_write_bin(path.c_str(), nullptr, -1));
    note("q3_audio_write_bin", q3_audio_write_bin((g_dir + "/absent/x.bin").c_str(), nullptr, 0));
}

}  // namespace

int cmd_files(const char* dir) {
    g_dir = dir;
    struct stat st;
    if (stat(dir, &st) != 0 || !S_ISDIR(st.st_mode)) die("%s is no directory", dir);
    files_wav();
    files_safetensors();
    files_config();
    files_model();
    files_bins();
    return finish("files");
}

// ================================================================================================================================
// dsp: host arithmetic over exact-size buffers
// ================================================================================================================================
namespace {

void dsp_resample() {
    // the rate pairs of tests/test_io_formats.py, both ways, and the copy
    const uint32_t pairs[][2] = {{16000, 24000}, {48000, 24000}, {44100, 24000}, {22050, 24000}, {24000, 16000}, {24000, 48000}, {24000, 44100}, {24000, 22050},
                                 {24000, 24000}, {8000, 96000}, {96000, 8000}, {0, 24000}, {24000, 0}, {1, 4000000000u}};
    for (const auto& pr : pairs)
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)127, (int64_t)128, (int64_t)129}) {
            Buf<float> in((size_t)n); for (size_t i = 0; i < in.n; ++i) in[i] = (float)rnd8() / 128.0f - 1.0f;
            int64_t no = -1;
            if (note("q3_resample", q3_resample(in, n, pr[0], pr[1], nullptr, 0, &no)) != Q3_OK) continue;
            must(no >= 0, "q3_resample: %lld samples out", (long long)no);
            if (no > (1 << 22)) continue;                          // (1 Hz to 4 GHz: the count alone)
            Buf<float> out((size_t)no);
            int64_t no2 = -1;
            must(note("q3_resample", q3_resample(in, n, pr[0], pr[1], out, no, &no2)) == Q3_OK && no2 == no, "q3_resample refused a buffer of its own count");
            for (size_t i = 0; i < out.n; ++i) must(std::isfinite(out[i]), "q3_resample: a non-finite sample from finite input");
            if (no > 0) { Buf<float> shrt((size_t)no - 1); must(note("q3_resample", q3_resample(in, n, pr[0], pr[1], shrt, no - 1, nullptr)) != Q3_OK, "q3_resample took a short buffer"); }
        }
    { Buf<float> in(4); int64_t no = 0; note("q3_resample", q3_resample(nullptr, 4, 16000, 24000, nullptr, 0, &no)); note("q3_resample", q3_resample(in, -1, 16000, 24000, nullptr, 0, &no));
      note("q3_resample", q3_resample(in, INT64_MIN, 16000, 24000, nullptr, 0, &no)); }
}

void dsp_pcm() {
    const float edge[] = {0.0f, -0.0f, 1.0f, -1.0f, 1.0000001f, -1.0000001f, 0.99999994f, 3.0517578e-5f, 1e30f, -1e30f, INFINITY, -INFINITY, NAN, -NAN, 1e-45f, 0.5f};
    for (size_t n : {(size_t)0, (size_t)1, sizeof edge / sizeof edge[0], (size_t)1000}) {
        Buf<float> x(n); Buf<int16_t> y(n);
        for (size_t i = 0; i < n; ++i) x[i] = i < sizeof edge / sizeof edge[0] ? edge[i] : (float)rnd8() / 100.0f - 1.28f;
        must(note("q3_pcm16_from_f32", q3_pcm16_from_f32(x, (int64_t)n, y)) == Q3_OK, "q3_pcm16_from_f32");
    }
    { Buf<float> x(1); Buf<int16_t> y(1); note("q3_pcm16_from_f32", q3_pcm16_from_f32(nullptr, 1, y)); note("q3_pcm16_from_f32", q3_pcm16_from_f32(x, 1, nullptr));
      note("q3_pcm16_from_f32", q3_pcm16_from_f32(nullptr, 0, nullptr)); note("q3_pcm16_from_f32", q3_pcm16_from_f32(x, -1, y)); note("q3_pcm16_from_f32", q3_pcm16_from_f32(x, INT64_MIN, y)); }
    // G.711, both directions, over every value there is
    Buf<int16_t> all(65536); for (int i = 0; i < 65536; ++i) all[(size_t)i] = (int16_t)(i - 32768);
    Buf<uint8_t> bytes(256); for (int i = 0; i < 256; ++i) bytes[(size_t)i] = (uint8_t)i;
    for (int law : grid_int({Q3_PCM_ULAW, Q3_PCM_ALAW})) {
        Buf<uint8_t> enc(65536); Buf<int16_t> dec(256);
        const int a = note("q3_g711_from_pcm16", q3_g711_from_pcm16(all, 65536, law, enc));
        const int b = note("q3_g711_to_pcm16", q3_g711_to_pcm16(bytes, 256, law, dec));
        must((a == Q3_OK) == (law == Q3_PCM_ULAW || law == Q3_PCM_ALAW) && a == b, "G.711: law %d gives %d / %d", law, a, b);
        if (a == Q3_OK) {                                          // expanding and compressing again gives the byte back
            Buf<uint8_t> again(256);
            must(note("q3_g711_from_pcm16", q3_g711_from_pcm16(dec, 256, law, again)) == Q3_OK, "G.711 round trip");
            for (int i = 0; i < 256; ++i) must(again[(size_t)i] == i || (law == Q3_PCM_ULAW && i == 0x7f && again[(size_t)i] == 0xff), "G.711 law %d: byte %d comes back as %d", law, i, again[(size_t)i]);
        }
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)-1, INT64_MIN}) {
            Buf<int16_t> p((size_t)(n > 0 ? n : 0)); Buf<uint8_t> q((size_t)(n > 0 ? n : 0));
            note("q3_g711_from_pcm16", q3_g711_from_pcm16(p, n, law, q)); note("q3_g711_to_pcm16", q3_g711_to_pcm16(q, n, law, p));
            note("q3_g711_from_pcm16", q3_g711_from_pcm16(nullptr, n, law, q)); note("q3_g711_to_pcm16", q3_g711_to_pcm16(q, n, law, nullptr));
        }
    }
    // codes_to_tensor: [n][16] -> [16][n]
    for (int n : {0, 1, 7, 640}) {
        Buf<uint32_t> fr((size_t)n * 16); Buf<int64_t> t((size_t)n * 16);
        for (size_t i = 0; i < fr.n; ++i) fr[i] = (uint32_t)i * 2654435761u;
        q3_codes_to_tensor(fr, n, t);
        for (int f = 0; f < n; ++f) for (int q = 0; q < 16; ++q) must(t[(size_t)q * (size_t)n + (size_t)f] == (int64_t)fr[(size_t)f * 16 + (size_t)q], "q3_codes_to_tensor");
        note_value(true);
    }
    // the PCG stream: every draw inside [0, 1]
    for (uint64_t seed : grid_u64({42})) {
        Buf<uint64_t> st(1);
        q3_rng_seed(seed, st);
        for (int i = 0; i < 4096; ++i) { const float u = q3_rng_next(st); must(u >= 0.0f && u <= 1.0f, "q3_rng_next: %g", (double)u); }
        note_value(true);
    }
}

void dsp_silence() {
    // n = 0, one hop, a hop and a sample, many hops with pauses; non-finite samples; a cap one below the need
    for (size_t n : {(size_t)0, (size_t)1, (size_t)239, (size_t)240, (size_t)241, (size_t)4800, (size_t)24000 * 3 + 17})
        for (int kind = 0; kind < 4; ++kind)                       // silence / loud / bursts with pauses / non-finite
            for (int thr : {-9000, -4000, -2000})
                for (int edge : {0, 10, 100, 1000})
                    for (int pause : {20, 200, 2000}) {
                        Buf<float> x(n);
                        for (size_t i = 0; i < n; ++i) {
                            const float v = (float)rnd8() / 256.0f - 0.5f;
                            x[i] = kind == 0 ? 0.0f : kind == 1 ? v : ((i / 6000) % 2 ? v : 1e-6f * v);
                            if (kind == 3 && i % 97 == 0) x[i] = i % 2 ? NAN : (i % 3 ? INFINITY : -INFINITY);
                        }
                        size_t ny = (size_t)-1; Buf<int64_t> counts(5);
                        must(note("q3_silence_trim", q3_silence_trim(x, n, thr, edge, pause, nullptr, 0, &ny, counts)) == Q3_OK, "q3_silence_trim's count query: %s", q3_last_error());
                        must(ny <= n && counts[0] == (int64_t)n && counts[1] == (int64_t)ny && counts[0] - counts[2] - counts[3] - counts[4] == counts[1], "q3_silence_trim: counts do not add up");
                        Buf<float> y(ny);
                        must(note("q3_silence_trim", q3_silence_trim(x, n, thr, edge, pause, y, ny, &ny, nullptr)) == Q3_OK, "q3_silence_trim refused a buffer of its own count");
                        if (ny > 0) { Buf<float> shrt(ny - 1); must(note("q3_silence_trim", q3_silence_trim(x, n, thr, edge, pause, shrt, ny - 1, &ny, nullptr)) != Q3_OK, "q3_silence_trim took a short buffer"); }
                    }
    Buf<float> x(480); size_t ny = 0;
    for (int thr : grid_int({-9000, -2000})) for (int edge : grid_int({10, 1000, 15})) for (int pause : grid_int({20, 2000, 25}))
        note("q3_silence_trim", q3_silence_trim(x, 480, thr, edge, pause, nullptr, 0, &ny, nullptr));
    note("q3_silence_trim", q3_silence_trim(nullptr, 480, -4000, 100, 200, nullptr, 0, &ny, nullptr));
    note("q3_silence_trim", q3_silence_trim(x, 480, -4000, 100, 200, nullptr, 0, nullptr, nullptr));
    note("q3_silence_trim", q3_silence_trim(x, 480, -4000, 100, 200, nullptr, 5, &ny, nullptr));
    for (uint64_t n : grid_u64({P40})) if (n > P40) note("q3_silence_trim", q3_silence_trim(x, (size_t)n, -4000, 100, 200, nullptr, 0, &ny, nullptr));
    for (int e : grid_int({10, 1000})) for (int p : grid_int({20, 2000})) { size_t h = 0; note("q3_pcm_stage_silence_hold", q3_pcm_stage_silence_hold(e, p, &h)); }
    note("q3_pcm_stage_silence_hold", q3_pcm_stage_silence_hold(100, 200, nullptr));
    for (int t : grid_int({-4000, -500})) for (int p : grid_int({-6000, 2400})) {
        float a = 0, b = 0, c = 0, d = 0, e = 0;
        note("q3_pcm_stage_loudness_consts", q3_pcm_stage_loudness_consts(t, p, &a, &b, &c, &d, &e));
        note("q3_pcm_stage_loudness_consts", q3_pcm_stage_loudness_consts(t, p, nullptr, nullptr, nullptr, nullptr, nullptr));
    }
}

}  // namespace

int cmd_dsp() {
    dsp_resample();
    dsp_pcm();
    dsp_silence();
    return finish("dsp");
}

// ================================================================================================================================
// refusals: entries that read caller arrays before they touch a device. With no device every call must come back as a status: a
// refusal row with the status its reference test lists, a well-formed call with the error of the device it did not find.
// The tables are those of the Python reference tests, copied by hand (the test named at each).
// ================================================================================================================================
namespace {

void expect(const char* what, int row, int st, int want) {
    note(what, st);
    must(st == want, "%s: row %d: status %d, expected %d (%s)", what, row, st, want, q3_last_error());
}
// a well-formed call: everything was read, then the device was asked for and is not there
void expect_no_device(const char* what, int st) {
    note(what, st);
    must(st != Q3_OK && st != Q3_INVALID_ARG, "%s: a well-formed call gives status %d without a device (%s)", what, st, st == Q3_OK ? "" : q3_last_error());
}
template <class T> void fill(Buf<T>& b, T v) { for (size_t i = 0; i < b.n; ++i) b[i] = v; }

// tests/test_abi.py::test_null_handles_return_status_not_crash
void refusals_null_handles() {
    q3_model* m = nullptr; q3_session* s = nullptr; q3_batcher* bt = nullptr; q3_speaker_encoder* se = nullptr; q3_dp_comm* dp = nullptr;
    int i = 0, j = 0, k = 0; size_t sz = 0; int64_t t64 = 0;
    const char* W = "null-handle table";
    int row = 0;
    auto bad = [&](int st) { note(W, st); must(st != Q3_OK, "%s: row %d is accepted", W, row); ++row; };
    bad(q3_model_create(nullptr, 0, &m));
    bad(q3_model_set_tensor(nullptr, "x", 0, nullptr, 0));
    bad(q3_model_finalize(nullptr));
    bad(q3_model_arena(nullptr, nullptr, nullptr));
    bad(q3_session_create(nullptr, nullptr, 1, &s));
    bad(q3_session_prefill(nullptr));
    bad(q3_session_generate(nullptr, 1, 1));
    bad(q3_session_frames(nullptr, 0, &i, &j));
    bad(q3_session_codes(nullptr, 0, nullptr, 0, &i));
    bad(q3_session_decode(nullptr, 0, 0, 0, nullptr, 0, &sz));
    bad(q3_session_run(nullptr, 1, nullptr, nullptr, nullptr, nullptr));
    bad(q3_session_next_chunk(nullptr, nullptr, 0, &sz, &i));
    bad(q3_session_set_stream_mode(nullptr, 1));
    bad(q3_session_set_kv_dtype(nullptr, 1));
    bad(q3_model_set_codec_planes(nullptr, 2));
    bad(q3_session_create_reserved(nullptr, nullptr, 1, 8, 16, &s));
    bad(q3_session_replace(nullptr, 0, nullptr));
    bad(q3_session_next_chunk_row(nullptr, 0, nullptr, 0, &sz, &i));
    bad(q3_batcher_create(nullptr, 8, 64, 0, &bt));
    bad(q3_batcher_submit(nullptr, nullptr, 0, &t64));
    bad(q3_batcher_step(nullptr, 8, 1, &i, &j, &k));
    bad(q3_batcher_poll(nullptr, 1, &i, &j, &sz));
    bad(q3_batcher_fetch(nullptr, 1, nullptr, 0, nullptr, 0));
    bad(q3_decode_codes(nullptr, nullptr, 0, nullptr, nullptr));
    bad(q3_spk_create(nullptr, 0, &se));
    bad(q3_spk_finalize(nullptr));
    bad(q3_spk_encode(nullptr, nullptr, 0, 24000, nullptr));
    bad(q3_spk_load_safetensors(nullptr, "/nonexistent"));
    bad(q3_dp_init(0, 1, nullptr, 0, &dp));
    bad(q3_dp_broadcast_weights(nullptr, nullptr, 0));
    bad(q3_config_from_json("/nonexistent/config.json", nullptr, nullptr));
    bad(q3_model_load("/nonexistent", -1, &m, &i));
    bad(q3_wav_read("/nonexistent.wav", nullptr, 0, nullptr, nullptr));
    bad(q3_resample(nullptr, 1, 16000, 24000, nullptr, 0, nullptr));
    { Buf<q3_linear_ex_args> a(1); bad(q3_linear_ex(0, nullptr)); bad(q3_linear_ex(0, a)); }
    { Buf<q3_attn_step_args> a(1); bad(q3_attn_step(0, nullptr)); bad(q3_attn_step(0, a)); }
    { Buf<q3_attn_step_ex_args> a(1); bad(q3_attn_step_ex(0, nullptr)); bad(q3_attn_step_ex(0, a)); }
    bad(q3_kv_pages_to_bf16_ex(0, 1, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    { Buf<q3_conv_ex_args> a(1); bad(q3_conv_ex(0, nullptr)); bad(q3_conv_ex(0, a)); }
    { Buf<q3_gemm_ex_args> a(1); bad(q3_gemm_ex(0, nullptr)); bad(q3_gemm_ex(0, a)); }
    { Buf<q3_attn_prefill_ex_args> a(1); bad(q3_attn_prefill_ex(0, nullptr)); bad(q3_attn_prefill_ex(0, a)); }
    { Buf<q3_prompt_rows_ex_args> a(1); bad(q3_prompt_rows_ex(0, nullptr)); bad(q3_prompt_rows_ex(0, a)); }
    { Buf<q3_attn_c_ex_args> a(1); bad(q3_attn_c_ex(0, nullptr)); bad(q3_attn_c_ex(0, a)); }
    bad(q3_rope_c_ex(0, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 64, 8, 8));
    bad(q3_copy_cols_ex(0, nullptr, 16, nullptr, 16, 1, 1, nullptr, nullptr, nullptr, nullptr, 0, 0));
    bad(q3_copy_segs_ex(0, nullptr, 16, nullptr, 16, 1, nullptr));
    bad(q3_gather_frames_ex(0, nullptr, 16, nullptr, 1, nullptr, 16));
    bad(q3_rvq_embed_ex(0, nullptr, 1, nullptr, nullptr, 8, 16, nullptr, nullptr, 0, 8));
    bad(q3_silu_mul_ex(0, nullptr, nullptr, nullptr, 8, 8));
    { Buf<q3_spk_op_ex_args> a(1); bad(q3_spk_op_ex(0, nullptr)); bad(q3_spk_op_ex(0, a)); }
    { Buf<q3_mimi_op_ex_args> a(1); bad(q3_mimi_op_ex(0, nullptr)); bad(q3_mimi_op_ex(0, a)); }
    bad(q3_mimi_rvq_ex(0, nullptr, 1, nullptr, 1, 4, 8, nullptr, 1, 0));
    bad(q3_spk_tables(nullptr, nullptr, nullptr));
    bad(q3_sample_row(nullptr, nullptr));
    bad(q3_prompt_shape(nullptr, 0, nullptr, nullptr, nullptr, 0));
    { Buf<q3_sample_ex_args> a(1); bad(q3_sample_ex(0, nullptr)); bad(q3_sample_ex(0, a)); }
    { Buf<q3_frame_embed_ex_args> a(1); bad(q3_frame_embed_ex(0, nullptr)); bad(q3_frame_embed_ex(0, a)); }
    { Buf<q3_cp_gather_ex_args> a(1); bad(q3_cp_gather_ex(0, nullptr)); bad(q3_cp_gather_ex(0, a)); }
    bad(q3_rmsnorm_ex(0, nullptr, 8, 0, 8, nullptr, nullptr, 8, 0, 8, 1, 8, 1e-6f, nullptr, nullptr));
    bad(q3_norm_c(0, 0, nullptr, nullptr, nullptr, 16, 8, 1e-6f, nullptr, 0, 128));
    bad(q3_dwconv7(0, nullptr, nullptr, nullptr, 16, 8, nullptr, 0, 128));
    must(row == 74, "the null-handle table has %d rows", row);
    q3_model_free(nullptr); q3_session_free(nullptr); q3_spk_free(nullptr); q3_dp_free(nullptr); q3_batcher_free(nullptr);      // free(NULL) is a no-op
    must(!m && !s && !bt && !se && !dp, "a refused create wrote a handle");
}

// tests/test_row_state_op.py::test_bad_arguments_return_status
void refusals_row_move() {
    const char* W = "q3_row_move";
    Buf<uint8_t> buf(64), dst(64); Buf<size_t> zero(1), n(1), far(1); Buf<int> mode(1), bad(1);
    zero[0] = 0; n[0] = 16; far[0] = 60; mode[0] = 0; bad[0] = 7;
    expect_no_device(W, q3_row_move(0, buf, 64, dst, 64, 1, zero, zero, n, mode));
    expect(W, 0, q3_row_move(0, nullptr, 64, dst, 64, 1, zero, zero, n, mode), Q3_INVALID_ARG);
    expect(W, 1, q3_row_move(0, buf, 64, dst, 64, 0, zero, zero, n, mode), Q3_INVALID_ARG);
    expect(W, 2, q3_row_move(0, buf, 64, dst, 64, 1, zero, zero, n, nullptr), Q3_INVALID_ARG);
    expect(W, 3, q3_row_move(0, buf, 64, dst, 64, 1, far, zero, n, mode), Q3_INVALID_ARG);          // 16 bytes from offset 60 of 64: leaves the source
    expect(W, 4, q3_row_move(0, buf, 64, dst, 64, 1, zero, far, n, mode), Q3_INVALID_ARG);          // ... the destination
    expect(W, 5, q3_row_move(0, buf, 64, dst, 64, 1, zero, zero, n, bad), Q3_INVALID_ARG);
    // the ends of the ranges: a segment that ends with its buffer, one byte more, offsets and lengths near SIZE_MAX
    { Buf<size_t> o(1), l(1); o[0] = 48; l[0] = 16; expect_no_device(W, q3_row_move(0, buf, 64, dst, 64, 1, o, o, l, mode)); l[0] = 17; expect(W, 6, q3_row_move(0, buf, 64, dst, 64, 1, o, o, l, mode), Q3_INVALID_ARG);
      o[0] = SIZE_MAX; l[0] = 2; expect(W, 7, q3_row_move(0, buf, 64, dst, 64, 1, o, zero, l, mode), Q3_INVALID_ARG); o[0] = 1; l[0] = SIZE_MAX; expect(W, 8, q3_row_move(0, buf, 64, dst, 64, 1, zero, o, l, mode), Q3_INVALID_ARG); }
    expect(W, 9, q3_row_move(0, buf, 0, dst, 64, 1, zero, zero, n, mode), Q3_INVALID_ARG);
    expect(W, 10, q3_row_move(0, buf, 64, dst, 64, 65536, zero, zero, n, mode), Q3_INVALID_ARG);
    expect(W, 11, q3_row_move(0, buf, 64, dst, 64, -1, zero, zero, n, mode), Q3_INVALID_ARG);
}

// tests/test_intake_host.py::test_refusals_need_no_device, and lists of 1, 64 and 65 clips and a null entry
void refusals_ref_audio() {
    const char* W = "q3_ref_audio_create";
    Buf<int16_t> data(64);
    auto clip = [&](int64_t frames = 16, int channels = 1, uint32_t rate = 16000, int fmt = Q3_SRC_S16, bool ptr = true) {
        q3_clip c; c.data = ptr ? data.p : nullptr; c.frames = frames; c.channels = channels; c.sample_rate = rate; c.format = fmt; return c;
    };
    q3_ref_audio* h = nullptr;
    auto one = [&](int row, int device, const q3_clip* c, q3_ref_audio** out, int want) {
        Buf<q3_clip> b(1); if (c) b[0] = *c;
        expect(W, row, q3_ref_audio_create(device, c ? b.p : nullptr, out), want);
    };
    q3_clip c = clip();
    one(0, 0, nullptr, &h, Q3_INVALID_ARG); one(1, 0, &c, nullptr, Q3_INVALID_ARG); one(2, -1, &c, &h, Q3_INVALID_ARG);
    c = clip(0); one(3, 0, &c, &h, Q3_INVALID_ARG); c = clip(16, 0); one(4, 0, &c, &h, Q3_INVALID_ARG); c = clip(16, 9); one(5, 0, &c, &h, Q3_INVALID_ARG);
    c = clip(16, 1, 16000, 7); one(6, 0, &c, &h, Q3_INVALID_ARG); c = clip(16, 1, 16000, -1); one(7, 0, &c, &h, Q3_INVALID_ARG);
    c = clip(16, 1, 16000, Q3_SRC_S16, false); one(8, 0, &c, &h, Q3_INVALID_ARG);
    c = clip(16, 1, 44101); one(9, 0, &c, &h, Q3_UNSUPPORTED); c = clip(16, 1, 192000); one(10, 0, &c, &h, Q3_UNSUPPORTED);
    c = clip(1, 1, 96000); one(11, 0, &c, &h, Q3_INVALID_ARG);                                       // n_out 0
    c = clip(24000LL * 121, 1, 24000); one(12, 0, &c, &h, Q3_INVALID_ARG);                           // longer than 120 s
    for (int64_t fr : grid_i64({24000LL * 120 * 4})) { c = clip(fr, 1, 96000); if (fr < 1 || fr > 64) { Buf<q3_clip> b(1); b[0] = c; note(W, q3_ref_audio_create(0, b, &h)); must(!h, "a refused clip left an object"); } }
    const char* WM = "q3_ref_audio_create_many";
    {
        Buf<q3_clip> three(3); three[0] = clip(); three[1] = clip(); three[2] = clip(16, 1, 44101);
        Buf<q3_ref_audio*> hs(3);
        expect(WM, 0, q3_ref_audio_create_many(0, 0, three, hs), Q3_INVALID_ARG);
        expect(WM, 1, q3_ref_audio_create_many(0, 65, three, hs), Q3_INVALID_ARG);
        expect(WM, 2, q3_ref_audio_create_many(0, 3, nullptr, hs), Q3_INVALID_ARG);
        expect(WM, 3, q3_ref_audio_create_many(0, 3, three, nullptr), Q3_INVALID_ARG);
        expect(WM, 4, q3_ref_audio_create_many(0, 3, three, hs), Q3_UNSUPPORTED);
        expect(WM, 5, q3_ref_audio_create_many(-1, 2, three, hs), Q3_INVALID_ARG);
        for (size_t i = 0; i < 3; ++i) must(!hs[i], "a refused list left an object");
    }
    for (int n : {1, 64, 65}) {
        // every clip with data of exactly its own size, in every format in turn; then the same list with a null entry in each place
        std::vector<Buf<uint8_t>*> raw;
        Buf<q3_clip> clips((size_t)n); Buf<q3_ref_audio*> hs((size_t)n);
        const int bytes_of[] = {1, 2, 3, 4, 4, 1, 1};
        for (int i = 0; i < n; ++i) {
            const int fmt = i % 7, ch = 1 + i % 8; const int64_t frames = 16 + 3 * i;
            raw.push_back(new Buf<uint8_t>((size_t)(frames * ch * bytes_of[fmt])));
            q3_clip& q = clips[(size_t)i]; q.data = raw.back()->p; q.frames = frames; q.channels = ch; q.sample_rate = i % 2 ? 44100 : 24000; q.format = fmt;
        }
        if (n <= 64) expect_no_device(WM, q3_ref_audio_create_many(0, n, clips, hs)); else expect(WM, 6, q3_ref_audio_create_many(0, n, clips, hs), Q3_INVALID_ARG);
        for (int i = 0; i < n && n <= 64; i += (n > 8 ? 21 : 1)) {
            const void* keep = clips[(size_t)i].data; clips[(size_t)i].data = nullptr;
            expect(WM, 7, q3_ref_audio_create_many(0, n, clips, hs), Q3_INVALID_ARG);
            must(strstr(q3_last_error(), ("clip " + std::to_string(i)).c_str()) != nullptr, "the refusal of a null entry does not name clip %d: %s", i, q3_last_error());
            clips[(size_t)i].data = keep;
        }
        for (size_t i = 0; i < hs.n; ++i) must(!hs[i], "a refused list left an object");
        for (auto* r : raw) delete r;
    }
    int64_t n64 = 0; int i = 0;
    expect("q3_ref_audio_from_wav", 0, q3_ref_audio_from_wav(nullptr, 0, &h), Q3_INVALID_ARG);
    expect("q3_ref_audio_from_wav", 1, q3_ref_audio_from_wav("/nonexistent.wav", 0, nullptr), Q3_INVALID_ARG);
    expect("q3_ref_audio_from_wav", 2, q3_ref_audio_from_wav("/nonexistent.wav", 0, &h), Q3_IO);
    expect("q3_ref_audio_info", 0, q3_ref_audio_info(nullptr, &n64, nullptr, nullptr, nullptr, nullptr), Q3_INVALID_ARG);
    expect("q3_ref_audio_read", 0, q3_ref_audio_read(nullptr, nullptr, 0, &n64), Q3_INVALID_ARG);
    expect("q3_spk_encode_ref", 0, q3_spk_encode_ref(nullptr, nullptr, nullptr), Q3_INVALID_ARG);
    expect("q3_mimi_encode_ref", 0, q3_mimi_encode_ref(nullptr, nullptr, nullptr, 0, &i, nullptr), Q3_INVALID_ARG);
    must(!h, "a refused call wrote a handle");
    q3_ref_audio_free(nullptr);
}

// the codec stream's movers and the RVQ embedding (the shapes of tests/test_gpu_codec_attn_ops.py; the refusals its header documents)
void refusals_movers() {
    {
        const char* W = "q3_copy_cols_ex";
        const int n = 3, C = 4;
        Buf<float> src(40), dst(48); Buf<long long> so(n), dof(n); Buf<int> sp(n), dp(n);
        auto reset = [&] { for (int j = 0; j < n; ++j) { so[(size_t)j] = j; dof[(size_t)j] = 2 * j; sp[(size_t)j] = 10; dp[(size_t)j] = 12; } so[1] = -1; };
        reset(); expect_no_device(W, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, 0));
        reset(); so[2] = 9; sp[2] = 10; expect_no_device(W, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, 0));       // the last float of the source
        reset(); so[2] = 10; expect(W, 0, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG);
        reset(); dof[2] = 12; expect(W, 1, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG);
        reset(); dof[0] = -1; expect(W, 2, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG);
        reset(); sp[0] = -1; expect(W, 3, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG);
        reset(); sp[0] = INT_MAX; expect(W, 4, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG);
        reset(); so[0] = LLONG_MAX; expect(W, 5, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG);
        reset(); dof[0] = LLONG_MIN; expect(W, 6, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG);
        reset(); expect(W, 7, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 8, 0), Q3_INVALID_ARG);
        reset(); expect(W, 8, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, 0, SIZE_MAX), Q3_INVALID_ARG);
        reset(); expect(W, 9, q3_copy_cols_ex(0, src, 40, dst, 48, n, C, so, dof, sp, dp, SIZE_MAX, 0), Q3_INVALID_ARG);
        for (int v : grid_int({1 << 20})) if (v < 1 || v > (1 << 20)) { reset(); expect(W, 10, q3_copy_cols_ex(0, src, 40, dst, 48, v, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG); }
        for (int v : grid_int({1 << 16})) if (v < 1 || v > (1 << 16)) { reset(); expect(W, 11, q3_copy_cols_ex(0, src, 40, dst, 48, n, v, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG); }
        for (uint64_t v : grid_u64({1ull << 28})) if (v < 1 || v > (1ull << 28)) { reset(); expect(W, 12, q3_copy_cols_ex(0, src, (size_t)v, dst, 48, n, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG);
                                                                                   expect(W, 13, q3_copy_cols_ex(0, src, 40, dst, (size_t)v, n, C, so, dof, sp, dp, 0, 0), Q3_INVALID_ARG); }
    }
    {
        const char* W = "q3_copy_segs_ex";
        Buf<float> src(32), dst(24); Buf<unsigned long long> segs(6);
        auto reset = [&] { segs[0] = 0; segs[1] = 4; segs[2] = 20; segs[3] = 31; segs[4] = 0; segs[5] = 1; };
        reset(); expect_no_device(W, q3_copy_segs_ex(0, src, 32, dst, 24, 2, segs));
        reset(); segs[2] = 21; expect(W, 0, q3_copy_segs_ex(0, src, 32, dst, 24, 2, segs), Q3_INVALID_ARG);
        reset(); segs[3] = 32; expect(W, 1, q3_copy_segs_ex(0, src, 32, dst, 24, 2, segs), Q3_INVALID_ARG);
        reset(); segs[3] = 33; segs[5] = 0; expect(W, 2, q3_copy_segs_ex(0, src, 32, dst, 24, 2, segs), Q3_INVALID_ARG);
        reset(); segs[0] = ULLONG_MAX; expect(W, 3, q3_copy_segs_ex(0, src, 32, dst, 24, 2, segs), Q3_INVALID_ARG);
        reset(); segs[2] = ULLONG_MAX; expect(W, 4, q3_copy_segs_ex(0, src, 32, dst, 24, 2, segs), Q3_INVALID_ARG);
        reset(); segs[4] = ULLONG_MAX - 1; expect(W, 5, q3_copy_segs_ex(0, src, 32, dst, 24, 2, segs), Q3_INVALID_ARG);
        reset(); segs[2] = 0; segs[5] = 0; expect(W, 6, q3_copy_segs_ex(0, src, 32, dst, 24, 2, segs), Q3_INVALID_ARG);          // every segment empty
        for (int v : grid_int({65535})) if (v < 1 || v > 65535) { reset(); expect(W, 7, q3_copy_segs_ex(0, src, 32, dst, 24, v, segs), Q3_INVALID_ARG); }
        for (uint64_t v : grid_u64({1ull << 28})) if (v < 1 || v > (1ull << 28)) { reset(); expect(W, 8, q3_copy_segs_ex(0, src, (size_t)v, dst, 24, 2, segs), Q3_INVALID_ARG);
                                                                                   expect(W, 9, q3_copy_segs_ex(0, src, 32, dst, (size_t)v, 2, segs), Q3_INVALID_ARG); }
    }
    {
        const char* W = "q3_gather_frames_ex";
        Buf<uint32_t> src(40), dst(48); Buf<long long> so(3);
        auto reset = [&] { so[0] = 0; so[1] = 24; so[2] = 7; };
        reset(); expect_no_device(W, q3_gather_frames_ex(0, src, 40, so, 3, dst, 48));
        reset(); so[1] = 25; expect(W, 0, q3_gather_frames_ex(0, src, 40, so, 3, dst, 48), Q3_INVALID_ARG);
        reset(); so[2] = -1; expect(W, 1, q3_gather_frames_ex(0, src, 40, so, 3, dst, 48), Q3_INVALID_ARG);
        reset(); so[0] = LLONG_MAX; expect(W, 2, q3_gather_frames_ex(0, src, 40, so, 3, dst, 48), Q3_INVALID_ARG);
        reset(); so[0] = LLONG_MIN; expect(W, 3, q3_gather_frames_ex(0, src, 40, so, 3, dst, 48), Q3_INVALID_ARG);
        reset(); expect(W, 4, q3_gather_frames_ex(0, src, 40, so, 3, dst, 47), Q3_INVALID_ARG);
        reset(); expect(W, 5, q3_gather_frames_ex(0, src, 15, so, 3, dst, 48), Q3_INVALID_ARG);
        for (int v : grid_int({1 << 20})) if (v < 1 || v > 3) { reset(); expect(W, 6, q3_gather_frames_ex(0, src, 40, so, v, dst, 48), Q3_INVALID_ARG); }
        for (uint64_t v : grid_u64({1ull << 28})) if (v < 16 || v > (1ull << 28)) { reset(); expect(W, 7, q3_gather_frames_ex(0, src, (size_t)v, so, 3, dst, 48), Q3_INVALID_ARG);
                                                                                    expect(W, 8, q3_gather_frames_ex(0, src, 40, so, 3, dst, (size_t)v), Q3_INVALID_ARG); }
    }
    {
        const char* W = "q3_rvq_embed_ex";
        const int nf = 5, cd = 6, cs = 7, front = 8, elems = front + cd * nf + 8;
        Buf<uint32_t> frames((size_t)nf * 16); Buf<float> fcb((size_t)cs * cd), rcb((size_t)15 * cs * cd), fo((size_t)elems), ro((size_t)elems);
        fill<uint32_t>(frames, 0xffffffffu);                        // (codes are taken modulo / clamped on the device: nothing to refuse)
        expect_no_device(W, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, cd, cs, fo, ro, front, elems));
        { Buf<float> fo0((size_t)cd * nf), ro0((size_t)cd * nf); expect_no_device(W, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, cd, cs, fo0, ro0, 0, cd * nf)); }
        expect(W, 0, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, cd, cs, fo, ro, front, front + cd * nf - 1), Q3_INVALID_ARG);
        expect(W, 1, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, cd, cs, fo, ro, -1, elems), Q3_INVALID_ARG);
        expect(W, 2, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, cd, cs, fo, ro, front, -1), Q3_INVALID_ARG);
        expect(W, 3, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, cd, cs, fo, ro, INT_MAX, INT_MAX), Q3_INVALID_ARG);
        for (int v : grid_int({1 << 16})) if (v < 1 || v > (1 << 16)) { expect(W, 4, q3_rvq_embed_ex(0, frames, v, fcb, rcb, cd, cs, fo, ro, front, elems), Q3_INVALID_ARG);
                                                                        expect(W, 5, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, cd, v, fo, ro, front, elems), Q3_INVALID_ARG); }
        for (int v : grid_int({256})) if (v < 1 || v > 256) expect(W, 6, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, v, cs, fo, ro, front, elems), Q3_INVALID_ARG);
        expect(W, 7, q3_rvq_embed_ex(0, nullptr, nf, fcb, rcb, cd, cs, fo, ro, front, elems), Q3_INVALID_ARG);
        expect(W, 8, q3_rvq_embed_ex(0, frames, nf, nullptr, rcb, cd, cs, fo, ro, front, elems), Q3_INVALID_ARG);
        expect(W, 9, q3_rvq_embed_ex(0, frames, nf, fcb, nullptr, cd, cs, fo, ro, front, elems), Q3_INVALID_ARG);
        expect(W, 10, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, cd, cs, nullptr, ro, front, elems), Q3_INVALID_ARG);
        expect(W, 11, q3_rvq_embed_ex(0, frames, nf, fcb, rcb, cd, cs, fo, nullptr, front, elems), Q3_INVALID_ARG);
    }
}

// tests/test_prompt_rows_reference.py::test_entry_refuses_what_a_kernel_could_not_address (the shapes of tests/prompt_rows_cases.py)
void refusals_prompt_rows() {
    const char* W = "q3_prompt_rows_ex";
    const int G = 64, VOCAB = 37, COLS = 24, N_TEXT = 9, N_REF = 3, CPV = 11;
    auto guarded = [&](size_t payload) { return payload + 2 * (size_t)G; };
    auto run = [&](const q3_prompt_rows_ex_args& a) { Buf<q3_prompt_rows_ex_args> b(1); b[0] = a; return (int)q3_prompt_rows_ex(0, b); };
    q3_prompt_rows_ex_args z; memset(&z, 0, sizeof z);
    // mode 0: the gather
    {
        const int n = 5;
        Buf<uint16_t> table((size_t)VOCAB * COLS); Buf<uint32_t> ids(n); Buf<float> out(guarded((size_t)n * COLS));
        auto args = [&] { q3_prompt_rows_ex_args a = z; a.mode = 0; a.n = n; a.cols = COLS; a.n_table = VOCAB; a.table = table; a.ids = ids; a.out = out; return a; };
        for (int i = 0; i < n; ++i) ids[(size_t)i] = (uint32_t)(i == 2 ? VOCAB - 1 : i);
        expect_no_device(W, run(args()));
        ids[2] = (uint32_t)VOCAB; expect(W, 0, run(args()), Q3_INVALID_ARG);
        ids[2] = 0xffffffffu; expect(W, 1, run(args()), Q3_INVALID_ARG);
        ids[2] = 0;
        { q3_prompt_rows_ex_args a = args(); a.cols = 0; expect(W, 2, run(a), Q3_INVALID_ARG); a = args(); a.cols = 65537; expect(W, 3, run(a), Q3_INVALID_ARG); a = args(); a.out = nullptr; expect(W, 4, run(a), Q3_INVALID_ARG);
          a = args(); a.table = nullptr; expect(W, 5, run(a), Q3_INVALID_ARG); a = args(); a.ids = nullptr; expect(W, 6, run(a), Q3_INVALID_ARG);
          for (int v : grid_int({1 << 20})) if (v < 1 || v > (1 << 20)) { a = args(); a.n_table = v; expect(W, 7, run(a), Q3_INVALID_ARG); }
          for (int v : grid_int({65535})) if (v < 1 || v > 65535) { a = args(); a.n = v; expect(W, 8, run(a), Q3_INVALID_ARG); }
          for (int v : grid_int({4})) if (v < 0 || v > 4) { a = args(); a.mode = v; expect(W, 9, run(a), Q3_INVALID_ARG); } }
    }
    // mode 1: the assembly
    {
        Buf<float> rows((size_t)N_TEXT * COLS), xvec(COLS); Buf<uint16_t> emb((size_t)VOCAB * COLS), cp((size_t)15 * CPV * COLS); Buf<uint32_t> ref((size_t)N_REF * 16);
        auto assemble = [&](int text_row, int codec_id, bool with_ref = true, bool with_cp = true, bool with_x = true) {
            Buf<int> tr(1), ci(1); tr[0] = text_row; ci[0] = codec_id; Buf<float> out(guarded(COLS));
            q3_prompt_rows_ex_args a = z; a.mode = 1; a.n = 1; a.cols = COLS; a.n_table = VOCAB; a.n_rows = N_TEXT; a.n_ref = N_REF; a.cp_vocab = CPV;
            a.src = rows; a.text_row = tr; a.codec_id = ci; a.table = emb; a.xvec = with_x ? xvec.p : nullptr; a.ref_codes = with_ref ? ref.p : nullptr; a.cp_embs = with_cp ? cp.p : nullptr; a.out = out;
            return run(a);
        };
        for (int cid : {0, VOCAB - 1, -1, -2, -3, -3 - (N_REF - 1)}) for (int tr : {0, N_TEXT - 1, -1, INT_MIN}) expect_no_device(W, assemble(tr, cid));
        expect(W, 10, assemble(N_TEXT, 0), Q3_INVALID_ARG);
        expect(W, 11, assemble(0, VOCAB), Q3_INVALID_ARG);
        expect(W, 12, assemble(0, -3 - N_REF), Q3_INVALID_ARG);
        expect(W, 13, assemble(0, INT_MIN), Q3_INVALID_ARG);
        expect(W, 14, assemble(0, -3, false), Q3_INVALID_ARG);
        expect(W, 15, assemble(0, -3, true, false), Q3_INVALID_ARG);
        expect(W, 16, assemble(0, -2, true, true, false), Q3_INVALID_ARG);
        ref[16] = (uint32_t)VOCAB; expect(W, 17, assemble(0, -4), Q3_INVALID_ARG); ref[16] = 0;          // frame 1: code 0 outside codec_emb
        ref[16 + 15] = (uint32_t)CPV; expect(W, 18, assemble(0, -4), Q3_INVALID_ARG); ref[16 + 15] = 0;   // ... code 15 outside its table
        expect(W, 19, assemble(INT_MAX, 0), Q3_INVALID_ARG);
        expect(W, 20, assemble(0, INT_MAX), Q3_INVALID_ARG);
    }
    // mode 2: the copy
    {
        const int n = 3;
        Buf<float> src((size_t)n * 12);
        auto copy = [&](int cols, int lds, int ldd, size_t out_payload) {
            Buf<float> out(guarded(out_payload));
            q3_prompt_rows_ex_args a = z; a.mode = 2; a.n = n; a.cols = cols; a.lds = lds; a.ldd = ldd; a.src = src; a.out = out;
            return run(a);
        };
        expect_no_device(W, copy(8, 12, 16, (size_t)n * 16));
        expect_no_device(W, copy(12, 12, 12, (size_t)n * 12));
        expect(W, 21, copy(13, 12, 16, (size_t)n * 16), Q3_INVALID_ARG);              // cols > lds
        expect(W, 22, copy(8, 12, 7, (size_t)n * 7), Q3_INVALID_ARG);                 // cols > ldd
        expect(W, 23, copy(8, (1 << 20) + 1, 16, (size_t)n * 16), Q3_INVALID_ARG);
        expect(W, 24, copy(8, 12, (1 << 20) + 1, (size_t)n * 16), Q3_INVALID_ARG);
        expect(W, 25, copy(8, INT_MAX, INT_MAX, (size_t)n * 16), Q3_INVALID_ARG);
    }
    // mode 3: the scatter
    {
        const int n = 8, ROWS = 12;
        Buf<float> src((size_t)n * COLS);
        auto scatter = [&](std::initializer_list<int> dst_rows, int n_rows = 12) {
            Buf<int> d(dst_rows.size()); size_t i = 0; for (int v : dst_rows) d[i++] = v;
            Buf<float> out(guarded((size_t)(n_rows > 0 && n_rows <= ROWS ? n_rows : ROWS) * COLS));
            q3_prompt_rows_ex_args a = z; a.mode = 3; a.n = (int)dst_rows.size(); a.cols = COLS; a.n_rows = n_rows; a.src = src; a.dst_row = d; a.out = out;
            return run(a);
        };
        expect_no_device(W, scatter({10, -1, 3, 0, -1, 7, -1, ROWS - 1}));
        expect(W, 26, scatter({10, -1, 3, 0, -1, 7, -1, ROWS}), Q3_INVALID_ARG);
        expect(W, 27, scatter({10, -1, 3, 0, -1, 7, -1, 3}), Q3_INVALID_ARG);
        expect(W, 28, scatter({10, -1, 3, 0, -1, 7, -1, INT_MAX}), Q3_INVALID_ARG);
        expect_no_device(W, scatter({INT_MIN, -1, 3, 0, -1, 7, -1, 1}));
        for (int v : grid_int({1 << 20})) if (v < 1 || v > (1 << 20)) expect(W, 29, scatter({0, 1}, v), Q3_INVALID_ARG);
    }
    // mode 4: the publish
    {
        const int ROWS = 9;
        auto publish = [&](std::initializer_list<std::initializer_list<int>> ent, int n_rows = 9) {
            Buf<int> e(ent.size() * 4); size_t i = 0; for (auto& r : ent) for (int v : r) e[i++] = v;
            const size_t rows = (size_t)(n_rows > 0 && n_rows <= ROWS ? n_rows : ROWS);
            Buf<int> tl(guarded(rows)), rd(guarded(rows)), lim(guarded(rows));
            q3_prompt_rows_ex_args a = z; a.mode = 4; a.n = (int)ent.size(); a.n_rows = n_rows; a.ent = e; a.trail_len = tl; a.text_ready = rd; a.limit = lim;
            return run(a);
        };
        expect_no_device(W, publish({{4, 1, 2, 3}, {ROWS - 1, 1, 2, 3}, {0, 7, 8, 9}}));
        expect(W, 30, publish({{ROWS, 1, 2, 3}}), Q3_INVALID_ARG);
        expect(W, 31, publish({{-1, 1, 2, 3}}), Q3_INVALID_ARG);
        expect(W, 32, publish({{4, 1, 2, 3}, {5, 1, 2, 3}, {4, 7, 8, 9}}), Q3_INVALID_ARG);
        expect(W, 33, publish({{INT_MAX, 1, 2, 3}}), Q3_INVALID_ARG);
        expect(W, 34, publish({{INT_MIN, 1, 2, 3}}), Q3_INVALID_ARG);
        for (int v : grid_int({1 << 20})) if (v < 1 || v > (1 << 20)) expect(W, 35, publish({{0, 1, 2, 3}}, v), Q3_INVALID_ARG);
        { Buf<int> e(4), tl(guarded(ROWS)); q3_prompt_rows_ex_args a = z; a.mode = 4; a.n = 1; a.n_rows = ROWS; a.ent = e; a.trail_len = tl; a.text_ready = tl; expect(W, 36, run(a), Q3_INVALID_ARG); }
    }
}

// tests/test_sampler_reference.py::test_sample_ex_refuses_bad_arguments_before_any_device_call and
// tests/test_frame_seam_reference.py::test_seam_entries_refuse_bad_arguments_before_any_device_call
void refusals_sampler_and_seam() {
    {
        const char* W = "q3_sample_ex";
        const int B = 3, V = 40, LD = 48, G = 8, HS = 2 * V;
        Buf<float> logits((size_t)B * LD), u((size_t)B * 2), hist((size_t)B * HS + 2 * G); Buf<int> didx(B), lim(B), rdy(B), tc(B + 2 * G), fi(B + 2 * G), pos(B + 2 * G);
        Buf<uint32_t> tok(B + 2 * G); Buf<uint8_t> seen((size_t)B * V + 2 * G); Buf<q3_sample_rec> rows(B);
        auto args = [&] {
            q3_sample_ex_args a; memset(&a, 0, sizeof a);
            a.B = B; a.vocab = V; a.ld = LD; a.u_stride = 2; a.u_elems = B * 2; a.advance = 1; a.hist_stride_b = HS; a.hist_cap = 2; a.codec_eos = V - 1; a.guard = G;
            a.logits = logits; a.u = u; a.draw_idx = didx; a.rows = rows; a.limit = lim; a.text_ready = rdy; a.tok = tok; a.seen = seen; a.token_count = tc; a.frame_idx = fi; a.pos = pos; a.logits_hist = hist;
            return a;
        };
        auto run = [&](const q3_sample_ex_args& a) { Buf<q3_sample_ex_args> b(1); b[0] = a; return (int)q3_sample_ex(0, b); };
        for (int i = 0; i < B; ++i) didx[(size_t)i] = i % 2;
        expect_no_device(W, run(args()));
        q3_sample_ex_args a = args(); a.vocab = 1; expect(W, 0, run(a), Q3_INVALID_ARG); a = args(); a.vocab = 4097; a.ld = 4097; expect(W, 1, run(a), Q3_INVALID_ARG);
        a = args(); a.B = 0; expect(W, 2, run(a), Q3_INVALID_ARG); a = args(); a.B = 1025; expect(W, 3, run(a), Q3_INVALID_ARG); a = args(); a.guard = -1; expect(W, 4, run(a), Q3_INVALID_ARG);
        a = args(); a.guard = 4097; expect(W, 5, run(a), Q3_INVALID_ARG); a = args(); a.ld = V - 1; expect(W, 6, run(a), Q3_INVALID_ARG); a = args(); a.ld = (1 << 16) + 1; expect(W, 7, run(a), Q3_INVALID_ARG);
        a = args(); a.u_stride = 0; expect(W, 8, run(a), Q3_INVALID_ARG); a = args(); a.u_elems = 0; expect(W, 9, run(a), Q3_INVALID_ARG);
        a = args(); a.frame_idx = nullptr; expect(W, 10, run(a), Q3_INVALID_ARG); a = args(); a.pos = nullptr; expect(W, 11, run(a), Q3_INVALID_ARG);
        a = args(); a.hist_cap = -1; expect(W, 12, run(a), Q3_INVALID_ARG); a = args(); a.hist_cap = 4097; expect(W, 13, run(a), Q3_INVALID_ARG); a = args(); a.hist_stride_b = 2 * V - 1; expect(W, 14, run(a), Q3_INVALID_ARG);
        didx[2] = 2; expect(W, 15, run(args()), Q3_INVALID_ARG); didx[2] = -1; expect(W, 16, run(args()), Q3_INVALID_ARG); didx[2] = INT_MAX; expect(W, 17, run(args()), Q3_INVALID_ARG); didx[2] = 0;
        a = args(); a.u_stride = INT_MAX; expect(W, 18, run(a), Q3_INVALID_ARG);
        tc[(size_t)G + 1] = -1; expect(W, 19, run(args()), Q3_INVALID_ARG); tc[(size_t)G + 1] = 0;
        a = args(); a.logits = nullptr; expect(W, 20, run(a), Q3_INVALID_ARG); a = args(); a.u = nullptr; expect(W, 21, run(a), Q3_INVALID_ARG); a = args(); a.tok = nullptr; expect(W, 22, run(a), Q3_INVALID_ARG);
    }
    {
        const char* W = "q3_frame_embed_ex";
        const int B = 2, H = 32, NS = 20, V = 12, MF = 3, NT = 7, G = 4;
        Buf<uint16_t> sem((size_t)NS * H), embs((size_t)15 * V * H); Buf<uint32_t> tok(B), codes((size_t)B * MF * 16 + 2 * G); Buf<float> lg((size_t)B * V), text((size_t)NT * H), out((size_t)B * H + 2 * G);
        Buf<int> fi(B), tb(B), tl(B), pr(B), rdy(B);
        auto reset = [&] { for (int b = 0; b < B; ++b) { fi[(size_t)b] = b ? MF : 1; tb[(size_t)b] = 2; tl[(size_t)b] = 2; pr[(size_t)b] = NT - 1; tok[(size_t)b] = (uint32_t)(NS - 1); } fill<uint32_t>(codes, (uint32_t)(V - 1)); };
        auto args = [&] {
            q3_frame_embed_ex_args a; memset(&a, 0, sizeof a);
            a.B = B; a.H = H; a.n_sem = NS; a.cp_vocab = V; a.max_frames = MF; a.n_text_rows = NT; a.guard = G;
            a.codec_emb = sem; a.cp_embs = embs; a.tok = tok; a.cp_logits_last = lg; a.frame_idx = fi; a.text_rows = text; a.trail_base = tb; a.trail_len = tl; a.pad_row = pr; a.text_ready = rdy; a.codes = codes; a.out = out;
            return a;
        };
        auto run = [&](const q3_frame_embed_ex_args& a) { Buf<q3_frame_embed_ex_args> b(1); b[0] = a; return (int)q3_frame_embed_ex(0, b); };
        reset(); expect_no_device(W, run(args()));
        reset(); fi[0] = -1; expect(W, 0, run(args()), Q3_INVALID_ARG); reset(); fi[1] = MF + 1; expect(W, 1, run(args()), Q3_INVALID_ARG); reset(); fi[0] = INT_MAX; expect(W, 2, run(args()), Q3_INVALID_ARG);
        reset(); tok[1] = (uint32_t)NS; expect(W, 3, run(args()), Q3_INVALID_ARG); reset(); tok[0] = 0xffffffffu; expect(W, 4, run(args()), Q3_INVALID_ARG);
        reset(); codes[(size_t)G + (0 * MF + 1) * 16 + 14] = (uint32_t)V; expect(W, 5, run(args()), Q3_INVALID_ARG);
        reset(); codes[(size_t)G + (1 * MF + MF - 1) * 16 + 1] = (uint32_t)V; expect(W, 6, run(args()), Q3_INVALID_ARG);          // a frozen row: its last slot is read
        reset(); codes[(size_t)G + (0 * MF + 1) * 16 + 0] = 0xffffffffu; codes[(size_t)G + (0 * MF + 1) * 16 + 15] = 0xffffffffu; expect_no_device(W, run(args()));      // (slots 0 and 15 are written, not read)
        reset(); tb[0] = NT - 1; expect(W, 7, run(args()), Q3_INVALID_ARG); reset(); tb[0] = -2; expect(W, 8, run(args()), Q3_INVALID_ARG); reset(); tb[0] = INT_MAX; expect(W, 9, run(args()), Q3_INVALID_ARG);
        reset(); pr[1] = NT; expect(W, 10, run(args()), Q3_INVALID_ARG); reset(); pr[1] = -1; expect(W, 11, run(args()), Q3_INVALID_ARG);
        reset();
        q3_frame_embed_ex_args a = args(); a.B = 0; expect(W, 12, run(a), Q3_INVALID_ARG); a = args(); a.B = 1025; expect(W, 13, run(a), Q3_INVALID_ARG); a = args(); a.H = 8193; expect(W, 14, run(a), Q3_INVALID_ARG);
        a = args(); a.max_frames = 0; expect(W, 15, run(a), Q3_INVALID_ARG); a = args(); a.max_frames = 4097; expect(W, 16, run(a), Q3_INVALID_ARG); a = args(); a.guard = -1; expect(W, 17, run(a), Q3_INVALID_ARG);
        a = args(); a.n_text_rows = 0; expect(W, 18, run(a), Q3_INVALID_ARG); a = args(); a.cp_vocab = 65537; expect(W, 19, run(a), Q3_INVALID_ARG); a = args(); a.n_sem = 0; expect(W, 20, run(a), Q3_INVALID_ARG);
        a = args(); a.codes = nullptr; expect(W, 21, run(a), Q3_INVALID_ARG); a = args(); a.pad_row = nullptr; expect(W, 22, run(a), Q3_INVALID_ARG); a = args(); a.text_ready = nullptr; expect_no_device(W, run(a));
    }
    {
        const char* W = "q3_cp_gather_ex";
        const int B = 2, H = 32, NS = 20, V = 12, MF = 3, G = 4, PD = 16, QD = 24, LDO = 36, LDQ = 28;
        Buf<float> lh((size_t)B * H), lg((size_t)B * V), out((size_t)B * LDO + 2 * G), qo((size_t)B * LDQ + 2 * G);
        Buf<uint16_t> sem((size_t)NS * H), emb((size_t)V * H); Buf<uint32_t> tok(B), codes((size_t)B * MF * 16 + 2 * G); Buf<int> fi(B);
        auto args = [&](int pass) {
            q3_cp_gather_ex_args a; memset(&a, 0, sizeof a);
            a.pass = pass; a.B = B; a.H = H; a.n_sem = NS; a.cp_vocab = V; a.max_frames = MF; a.ld_out = LDO; a.guard = G;
            a.last_hidden = lh; a.codec_emb = sem; a.tok = tok; a.cp_emb = emb; a.cp_logits = lg; a.frame_idx = fi; a.codes = codes; a.out = out;
            return a;
        };
        auto run = [&](const q3_cp_gather_ex_args& a) { Buf<q3_cp_gather_ex_args> b(1); b[0] = a; return (int)q3_cp_gather_ex(0, b); };
        tok[0] = 0; tok[1] = (uint32_t)(NS - 1); fi[0] = 0; fi[1] = MF;
        for (int pass : {0, 1, 2, 15}) expect_no_device(W, run(args(pass)));
        { Buf<float> pt((size_t)NS * PD), qt((size_t)NS * QD); q3_cp_gather_ex_args a = args(1); a.proj_tab = pt; a.proj_dim = PD; a.qkv_tab = qt; a.qkv_dim = QD; a.qkv_out = qo; a.ld_qkv_out = LDQ; expect_no_device(W, run(a));
          a.qkv_dim = 22; expect(W, 0, run(a), Q3_INVALID_ARG); a.qkv_dim = QD; a.ld_qkv_out = 20; expect(W, 1, run(a), Q3_INVALID_ARG); a.ld_qkv_out = LDQ; a.qkv_out = nullptr; expect(W, 2, run(a), Q3_INVALID_ARG);
          a.qkv_out = qo; a.guard = 3; expect(W, 3, run(a), Q3_INVALID_ARG); a.guard = G; a.proj_dim = LDO + 1; expect(W, 4, run(a), Q3_INVALID_ARG); a.proj_dim = 0; expect(W, 5, run(a), Q3_INVALID_ARG); }
        q3_cp_gather_ex_args a = args(-1); expect(W, 6, run(a), Q3_INVALID_ARG); a = args(16); expect(W, 7, run(a), Q3_INVALID_ARG); a = args(0); a.last_hidden = nullptr; expect(W, 8, run(a), Q3_INVALID_ARG);
        a = args(1); a.tok = nullptr; expect(W, 9, run(a), Q3_INVALID_ARG); a = args(1); a.codec_emb = nullptr; expect(W, 10, run(a), Q3_INVALID_ARG); a = args(1); a.n_sem = 0; expect(W, 11, run(a), Q3_INVALID_ARG);
        tok[1] = (uint32_t)NS; expect(W, 12, run(args(1)), Q3_INVALID_ARG); tok[1] = 0xffffffffu; expect(W, 13, run(args(1)), Q3_INVALID_ARG); tok[1] = 0;
        a = args(2); a.cp_logits = nullptr; expect(W, 14, run(a), Q3_INVALID_ARG); a = args(2); a.codes = nullptr; expect(W, 15, run(a), Q3_INVALID_ARG); a = args(2); a.max_frames = 0; expect(W, 16, run(a), Q3_INVALID_ARG);
        a = args(2); a.cp_vocab = 65537; expect(W, 17, run(a), Q3_INVALID_ARG); fi[0] = -1; expect(W, 18, run(args(2)), Q3_INVALID_ARG); fi[0] = INT_MIN; expect(W, 19, run(args(3)), Q3_INVALID_ARG); fi[0] = 0;
        a = args(0); a.ld_out = H - 1; expect(W, 20, run(a), Q3_INVALID_ARG); a = args(0); a.B = 0; expect(W, 21, run(a), Q3_INVALID_ARG); a = args(0); a.H = 8193; a.ld_out = 8193; expect(W, 22, run(a), Q3_INVALID_ARG);
        a = args(0); a.out = nullptr; expect(W, 23, run(a), Q3_INVALID_ARG);
    }
}

// the vocoder conv family and the prefill GEMM (the argument checks tests/test_gpu_conv_ops.py and tests/test_gpu_prefill_ops.py name)
void refusals_conv_gemm() {
    {
        const char* W = "q3_conv_ex";
        const int cin = 16, cout = 32, L = 40, k = 7, front = 8, elems = front + cout * L + 8;
        Buf<float> x((size_t)cin * L), w((size_t)cout * cin * k), b(cout), sa(cin), sb(cin), resid((size_t)cout * L), y((size_t)elems), y2((size_t)elems), w2((size_t)cin * cin), ma(cin), mb(cin);
        Buf<int> path(1);
        auto args = [&] {
            q3_conv_ex_args a; memset(&a, 0, sizeof a);
            a.kind = 0; a.cin = cin; a.cout = cout; a.L = L; a.k = k; a.dil = 1; a.stride = 1; a.planes = 3; a.packed = 1; a.y_front = front; a.y_elems = elems; a.path = path;
            a.x = x; a.w = w; a.b = b; a.snake_a = sa; a.snake_b = sb; a.resid = resid; a.y = y; a.y2 = y2;
            return a;
        };
        auto run = [&](const q3_conv_ex_args& a) { Buf<q3_conv_ex_args> bb(1); bb[0] = a; return (int)q3_conv_ex(0, bb); };
        expect_no_device(W, run(args()));
        q3_conv_ex_args a = args(); a.kind = 3; expect(W, 0, run(a), Q3_INVALID_ARG); a = args(); a.kind = -1; expect(W, 1, run(a), Q3_INVALID_ARG);
        a = args(); a.cin = 0; expect(W, 2, run(a), Q3_INVALID_ARG); a = args(); a.cout = 8193; expect(W, 3, run(a), Q3_INVALID_ARG); a = args(); a.L = 0; expect(W, 4, run(a), Q3_INVALID_ARG);
        a = args(); a.L = (1 << 22) + 1; expect(W, 5, run(a), Q3_INVALID_ARG); a = args(); a.L = INT_MAX; expect(W, 6, run(a), Q3_INVALID_ARG); a = args(); a.k = 65; expect(W, 7, run(a), Q3_INVALID_ARG);
        a = args(); a.dil = 0; expect(W, 8, run(a), Q3_INVALID_ARG); a = args(); a.dil = INT_MIN; expect(W, 9, run(a), Q3_INVALID_ARG); a = args(); a.act = 7; expect(W, 10, run(a), Q3_INVALID_ARG);
        a = args(); a.snake_b = nullptr; expect(W, 11, run(a), Q3_INVALID_ARG); a = args(); a.post_a = sa; expect(W, 12, run(a), Q3_INVALID_ARG);
        a = args(); a.resid_in_place = 1; expect(W, 13, run(a), Q3_INVALID_ARG);                     // two residuals
        a = args(); a.y_front = 6; expect(W, 14, run(a), Q3_INVALID_ARG); a = args(); a.y_front = -4; expect(W, 15, run(a), Q3_INVALID_ARG); a = args(); a.y_elems = front + cout * L - 1; expect(W, 16, run(a), Q3_INVALID_ARG);
        a = args(); a.y_elems = -1; expect(W, 17, run(a), Q3_INVALID_ARG); a = args(); a.y_front = INT_MAX - 3; a.y_elems = INT_MAX; expect(W, 18, run(a), Q3_INVALID_ARG);
        a = args(); a.kind = 1; a.stride = 3; expect(W, 19, run(a), Q3_INVALID_ARG);                  // k % stride, and resid belongs to kind 0
        a = args(); a.kind = 1; a.stride = 7; expect(W, 20, run(a), Q3_INVALID_ARG);                  // resid / act belong to kind 0
        a = args(); a.kind = 2; expect(W, 21, run(a), Q3_INVALID_ARG);                                // cin != cout
        a = args(); a.kind = 2; a.cout = cin; a.resid = nullptr; a.w2 = w2; a.mid_a = ma; expect(W, 22, run(a), Q3_INVALID_ARG);          // half a middle pair
        a = args(); a.x = nullptr; expect(W, 23, run(a), Q3_INVALID_ARG); a = args(); a.w = nullptr; expect(W, 24, run(a), Q3_INVALID_ARG); a = args(); a.y = nullptr; expect(W, 25, run(a), Q3_INVALID_ARG);
        { q3_conv_ex_args c = args(); c.kind = 2; c.cout = cin; c.resid = nullptr; c.w2 = w2; c.mid_a = ma; c.mid_ib = mb; c.y_elems = front + cin * L + 8; Buf<float> w7((size_t)cin * cin * 7); c.w = w7; expect_no_device(W, run(c)); }
    }
    {
        const char* W = "q3_gemm_ex";
        const int M = 5, N = 64, K = 40, ldx = 48, ldy = 72, ldr = 68, MA = 6;
        Buf<float> x((size_t)M * ldx), bias(N), nw(K), resid((size_t)M * ldr), y((size_t)MA * ldy); Buf<uint16_t> w((size_t)N * K), w2((size_t)N * K); Buf<int> path(4);
        auto args = [&] {
            q3_gemm_ex_args a; memset(&a, 0, sizeof a);
            a.M = M; a.N = N; a.K = K; a.ldx = ldx; a.ldy = ldy; a.ldr = ldr; a.M_alloc = MA; a.epi = 1; a.geometry = -1; a.eps = 1e-6f; a.path = path;
            a.x = x; a.w = w; a.bias = bias; a.resid = resid; a.y = y;
            return a;
        };
        auto run = [&](const q3_gemm_ex_args& a) { Buf<q3_gemm_ex_args> bb(1); bb[0] = a; return (int)q3_gemm_ex(0, bb); };
        expect_no_device(W, run(args()));
        { q3_gemm_ex_args a = args(); a.epi = 3; a.w2 = w2; a.norm_w = nw; a.resid = nullptr; expect_no_device(W, run(a)); }
        q3_gemm_ex_args a = args(); a.M = 0; expect(W, 0, run(a), Q3_INVALID_ARG); a = args(); a.M = 8193; expect(W, 1, run(a), Q3_INVALID_ARG); a = args(); a.N = 16385; expect(W, 2, run(a), Q3_INVALID_ARG);
        a = args(); a.K = 3; expect(W, 3, run(a), Q3_INVALID_ARG); a = args(); a.K = INT_MAX; expect(W, 4, run(a), Q3_INVALID_ARG); a = args(); a.ldx = K - 1; expect(W, 5, run(a), Q3_INVALID_ARG);
        a = args(); a.ldy = N - 1; expect(W, 6, run(a), Q3_INVALID_ARG); a = args(); a.M_alloc = M - 1; expect(W, 7, run(a), Q3_INVALID_ARG); a = args(); a.epi = 4; expect(W, 8, run(a), Q3_INVALID_ARG);
        a = args(); a.geometry = 4; expect(W, 9, run(a), Q3_INVALID_ARG); a = args(); a.geometry = -2; expect(W, 10, run(a), Q3_INVALID_ARG); a = args(); a.k_split = -1; expect(W, 11, run(a), Q3_INVALID_ARG);
        a = args(); a.sup_m = 2; expect(W, 12, run(a), Q3_INVALID_ARG); a = args(); a.resid = nullptr; expect(W, 13, run(a), Q3_INVALID_ARG); a = args(); a.ldr = N - 1; expect(W, 14, run(a), Q3_INVALID_ARG);
        a = args(); a.K = 42; a.ldx = 48; expect(W, 15, run(a), Q3_UNSUPPORTED); a = args(); a.ldx = 50; expect(W, 16, run(a), Q3_UNSUPPORTED); a = args(); a.ldy = 74; expect(W, 17, run(a), Q3_UNSUPPORTED);
        a = args(); a.N = 32; expect(W, 18, run(a), Q3_UNSUPPORTED); a = args(); a.ldr = 70; expect(W, 19, run(a), Q3_UNSUPPORTED); a = args(); a.K = 36; expect(W, 20, run(a), Q3_UNSUPPORTED);
        a = args(); a.x = nullptr; expect(W, 21, run(a), Q3_INVALID_ARG); a = args(); a.w = nullptr; expect(W, 22, run(a), Q3_INVALID_ARG); a = args(); a.y = nullptr; expect(W, 23, run(a), Q3_INVALID_ARG);
    }
}

// the attention entries: tests/test_attention_forms_reference.py, tests/test_prefill_ops_reference.py::test_paged_entry_refuses_
// before_a_device_is_touched (slot tables and the sharing rule) and the packed sibling's checks
void refusals_attention() {
    const int HD = 128;
    Buf<float> qw(HD), kw(HD);
    {
        const char* W = "q3_attn_step_ex";
        const int B = 2, nh = 2, nkv = 1, MS = 200, NPG = 2;
        Buf<int> pos(B), slots((size_t)B * NPG), rot((size_t)B * NPG * nkv); Buf<long long> stray(2);
        Buf<float> qkv((size_t)B * (nh + 2 * nkv) * HD), rc((size_t)MS * 64), rs((size_t)MS * 64), kc((size_t)B * nkv * MS * HD), vc((size_t)B * nkv * MS * HD), out((size_t)B * nh * HD), zero(16 + 4);
        auto reset = [&] { pos[0] = 0; pos[1] = MS - 1; slots[0] = 0; slots[1] = 31; slots[2] = 7; slots[3] = 8; };
        auto args = [&](int variant, int layout) {
            q3_attn_step_ex_args a; memset(&a, 0, sizeof a);
            a.variant = variant; a.layout = layout; a.B = B; a.nh = nh; a.nkv = nkv; a.n_splits = 2; a.max_seq = MS; a.rows_per_seq = 1; a.n_layers = 2; a.layer = 1; a.n_slabs = 1; a.kv_row_pages = 2;
            a.eps = 1e-6f; a.pos = pos; a.qkv = qkv; a.q_norm_w = qw; a.k_norm_w = kw; a.rope_cos = rc; a.rope_sin = rs; a.kcache = kc; a.vcache = vc; a.out = out;
            a.page_slots = slots; a.rot_used = rot; a.stray = stray; a.zero_n = 16; a.zero_guard = 4; a.zero_buf = zero;
            return a;
        };
        auto run = [&](const q3_attn_step_ex_args& a) { Buf<q3_attn_step_ex_args> bb(1); bb[0] = a; return (int)q3_attn_step_ex(0, bb); };
        reset();
        for (int layout = 0; layout < 3; ++layout) expect_no_device(W, run(args(0, layout)));
        { q3_attn_step_ex_args a = args(1, 1); a.zero_n = 0; expect_no_device(W, run(a)); }
        q3_attn_step_ex_args a = args(4, 0); expect(W, 0, run(a), Q3_INVALID_ARG); a = args(0, 3); expect(W, 1, run(a), Q3_INVALID_ARG); a = args(0, 0); a.B = 0; expect(W, 2, run(a), Q3_INVALID_ARG);
        a = args(0, 0); a.B = Q3_MAX_BATCH + 1; expect(W, 3, run(a), Q3_INVALID_ARG); a = args(0, 0); a.nkv = 0; expect(W, 4, run(a), Q3_INVALID_ARG); a = args(0, 0); a.nh = 3; a.nkv = 2; expect(W, 5, run(a), Q3_INVALID_ARG);
        a = args(0, 0); a.nh = 65; a.nkv = 65; expect(W, 6, run(a), Q3_INVALID_ARG); a = args(0, 0); a.max_seq = 0; expect(W, 7, run(a), Q3_INVALID_ARG); a = args(0, 0); a.max_seq = (1 << 20) + 1; expect(W, 8, run(a), Q3_INVALID_ARG);
        a = args(0, 0); a.n_splits = 0; expect(W, 9, run(a), Q3_INVALID_ARG); a = args(0, 0); a.n_splits = 65; expect(W, 10, run(a), Q3_INVALID_ARG);
        a = args(0, 0); a.nh = 8; a.nkv = 1; expect(W, 11, run(a), Q3_UNSUPPORTED);
        a = args(1, 0); a.rows_per_seq = 9; expect(W, 12, run(a), Q3_INVALID_ARG); a = args(0, 0); a.rows_per_seq = 2; expect(W, 13, run(a), Q3_UNSUPPORTED);
        a = args(3, 0); a.n_splits = 1; expect(W, 14, run(a), Q3_INVALID_ARG); a = args(2, 1); expect(W, 15, run(a), Q3_UNSUPPORTED); a = args(1, 2); a.zero_n = 0; expect(W, 16, run(a), Q3_UNSUPPORTED);
        pos[1] = MS; expect(W, 17, run(args(0, 0)), Q3_INVALID_ARG); pos[1] = -1; expect(W, 18, run(args(0, 0)), Q3_INVALID_ARG); pos[1] = INT_MAX; expect(W, 19, run(args(0, 0)), Q3_INVALID_ARG); reset();
        a = args(2, 0); a.n_splits = 1; expect(W, 20, run(a), Q3_INVALID_ARG);                            // variant 2: one position for every row
        pos[1] = 0; a = args(2, 0); expect(W, 21, run(a), Q3_UNSUPPORTED); reset();                         // ... one split
        a = args(0, 1); a.n_layers = 5; expect(W, 22, run(a), Q3_INVALID_ARG); a = args(0, 1); a.layer = 2; expect(W, 23, run(a), Q3_INVALID_ARG); a = args(0, 1); a.n_slabs = 3; expect(W, 24, run(a), Q3_INVALID_ARG);
        a = args(0, 1); a.page_slots = nullptr; expect(W, 25, run(a), Q3_INVALID_ARG); a = args(0, 1); a.stray = nullptr; expect(W, 26, run(a), Q3_INVALID_ARG);
        a = args(0, 1); a.kv_row_pages = 1; expect(W, 27, run(a), Q3_INVALID_ARG); a = args(0, 1); a.kv_row_pages = 65; expect(W, 28, run(a), Q3_INVALID_ARG); a = args(0, 1); a.kv_row_pages = -1; expect(W, 29, run(a), Q3_INVALID_ARG);
        slots[3] = 32; expect(W, 30, run(args(0, 1)), Q3_INVALID_ARG); { q3_attn_step_ex_args c = args(0, 1); c.n_slabs = 2; expect_no_device(W, run(c)); }
        slots[3] = 7; expect(W, 31, run(args(0, 1)), Q3_INVALID_ARG); slots[3] = -1; expect(W, 32, run(args(0, 1)), Q3_INVALID_ARG); slots[3] = INT_MAX; expect(W, 33, run(args(0, 1)), Q3_INVALID_ARG); reset();
        kc[kc.n - 1] = 1.0000001f; expect(W, 34, run(args(0, 2)), Q3_INVALID_ARG); kc[kc.n - 1] = 0.0f;           // not exact in bf16
        a = args(0, 0); a.zero_n = 6; expect(W, 35, run(a), Q3_INVALID_ARG); a = args(0, 0); a.zero_buf = nullptr; expect(W, 36, run(a), Q3_INVALID_ARG); a = args(1, 0); expect(W, 37, run(a), Q3_INVALID_ARG);
        a = args(0, 0); a.qkv = nullptr; expect(W, 38, run(a), Q3_INVALID_ARG); a = args(0, 0); a.out = nullptr; expect(W, 39, run(a), Q3_INVALID_ARG);
        { Buf<float> part((size_t)2 * B * 512), ssq((size_t)2 * B); a = args(1, 0); a.zero_n = 0; a.qkv_part = part; a.qkv_ssq = ssq; a.qkv_S = 2; a.qkv_K = 64; expect(W, 40, run(a), Q3_INVALID_ARG);
          a = args(0, 0); a.qkv_part = part; a.qkv_S = 2; a.qkv_K = 64; expect(W, 41, run(a), Q3_INVALID_ARG); a.qkv_ssq = ssq; a.qkv_S = 9; expect(W, 42, run(a), Q3_INVALID_ARG); }
        { Buf<uint32_t> gt(B); a = args(0, 0); a.g_tok = gt; expect(W, 43, run(a), Q3_INVALID_ARG); }
    }
    {
        const char* W = "q3_attn_prefill_ex";
        const int NS = 2, RPS = 4, BASE = 128, nh = 2, nkv = 1, MS = 256, NPG = 2, LDQ = (nh + 2 * nkv) * HD, LDO = nh * HD + 4;
        Buf<float> qkv((size_t)NS * RPS * LDQ), rc((size_t)MS * 64), rs((size_t)MS * 64), kc((size_t)NS * nkv * MS * HD), vc((size_t)NS * nkv * MS * HD), out((size_t)NS * RPS * LDO);
        Buf<int> slots((size_t)NS * NPG), rot((size_t)NS * NPG * nkv), path(2); Buf<long long> stray(2);
        auto reset = [&] { slots[0] = 5; slots[1] = 1; slots[2] = 5; slots[3] = 2; };                    // page 0 shared: a whole page below base_pos with the same bits
        auto args = [&](int layout) {
            q3_attn_prefill_ex_args a; memset(&a, 0, sizeof a);
            a.n_seq = NS; a.rps = RPS; a.base_pos = BASE; a.nh = nh; a.nkv = nkv; a.max_seq = MS; a.ld_qkv = LDQ; a.ld_out = LDO; a.kernel = -1; a.halves = 1; a.use_planes = 1; a.eps = 1e-6f; a.path = path;
            a.qkv = qkv; a.q_norm_w = qw; a.k_norm_w = kw; a.rope_cos = rc; a.rope_sin = rs; a.kcache = kc; a.vcache = vc; a.out = out;
            a.layout = layout; a.n_layers = 2; a.layer = 0; a.n_slabs = 1; a.page_slots = slots; a.rot_used = rot; a.stray = stray;
            return a;
        };
        auto run = [&](const q3_attn_prefill_ex_args& a) { Buf<q3_attn_prefill_ex_args> bb(1); bb[0] = a; return (int)q3_attn_prefill_ex(0, bb); };
        reset(); expect_no_device(W, run(args(0))); expect_no_device(W, run(args(1)));
        q3_attn_prefill_ex_args a = args(1); a.base_pos = 127; a.rps = 4; expect(W, 0, run(a), Q3_INVALID_ARG);                  // the shared page is not wholly below base_pos
        vc[(size_t)(1 * nkv * MS + 127) * HD + 127] = 1.0f; expect(W, 1, run(args(1)), Q3_INVALID_ARG); vc[(size_t)(1 * nkv * MS + 127) * HD + 127] = 0.0f;          // ... or its bits differ
        slots[2] = 1; expect(W, 2, run(args(1)), Q3_INVALID_ARG); reset();                                  // page 1 of one sequence as page 0 of another
        slots[1] = 5; expect(W, 3, run(args(1)), Q3_INVALID_ARG); reset();                                  // twice in one sequence
        slots[3] = 32; expect(W, 4, run(args(1)), Q3_INVALID_ARG); { q3_attn_prefill_ex_args c = args(1); c.n_slabs = 2; expect_no_device(W, run(c)); }
        slots[3] = -1; expect(W, 5, run(args(1)), Q3_INVALID_ARG); slots[3] = INT_MAX; expect(W, 6, run(args(1)), Q3_INVALID_ARG); slots[3] = INT_MIN; expect(W, 7, run(args(1)), Q3_INVALID_ARG); reset();
        a = args(2); expect(W, 8, run(a), Q3_UNSUPPORTED); a = args(3); expect(W, 9, run(a), Q3_INVALID_ARG); a = args(-1); expect(W, 10, run(a), Q3_INVALID_ARG);
        a = args(1); a.n_layers = 0; expect(W, 11, run(a), Q3_INVALID_ARG); a = args(1); a.layer = 2; expect(W, 12, run(a), Q3_INVALID_ARG); a = args(1); a.n_slabs = 0; expect(W, 13, run(a), Q3_INVALID_ARG);
        a = args(1); a.page_slots = nullptr; expect(W, 14, run(a), Q3_INVALID_ARG); a = args(1); a.stray = nullptr; expect(W, 15, run(a), Q3_INVALID_ARG);
        a = args(1); a.max_seq = 64 * 128 + 1; a.base_pos = 0; expect(W, 16, run(a), Q3_INVALID_ARG);
        a = args(0); a.kernel = 4; expect(W, 17, run(a), Q3_INVALID_ARG); a = args(0); a.halves = 3; expect(W, 18, run(a), Q3_INVALID_ARG); a = args(0); a.n_seq = 65; expect(W, 19, run(a), Q3_INVALID_ARG);
        a = args(0); a.rps = 8193; expect(W, 20, run(a), Q3_INVALID_ARG); a = args(0); a.base_pos = MS - RPS + 1; expect(W, 21, run(a), Q3_INVALID_ARG); a = args(0); a.base_pos = -1; expect(W, 22, run(a), Q3_INVALID_ARG);
        a = args(0); a.base_pos = INT_MAX; expect(W, 23, run(a), Q3_INVALID_ARG); a = args(0); a.base_pos = INT_MAX - 3; expect(W, 24, run(a), Q3_INVALID_ARG);
        a = args(0); a.max_seq = INT_MAX; a.base_pos = 0; expect(W, 31, run(a), Q3_INVALID_ARG); a = args(0); a.max_seq = (1 << 20) + 1; expect(W, 32, run(a), Q3_INVALID_ARG);
        a = args(0); a.ld_qkv = LDQ - 4; expect(W, 25, run(a), Q3_INVALID_ARG); a = args(0); a.ld_qkv = LDQ + 2; expect(W, 26, run(a), Q3_INVALID_ARG); a = args(0); a.ld_out = nh * HD - 4; expect(W, 27, run(a), Q3_INVALID_ARG);
        a = args(0); a.nh = 3; a.nkv = 2; expect(W, 28, run(a), Q3_INVALID_ARG); a = args(0); a.qkv = nullptr; expect(W, 29, run(a), Q3_INVALID_ARG); a = args(0); a.out = nullptr; expect(W, 30, run(a), Q3_INVALID_ARG);
    }
    {
        const char* W = "q3_attn_prefill_packed_ex";
        const int NS = 3, nh = 2, nkv = 1, MS = 130, NPG = 2, LDQ = (nh + 2 * nkv) * HD, LDO = nh * HD, ROWS = 1 + 130 + 48;
        Buf<int> len(NS), slots((size_t)NS * NPG), rot((size_t)NS * NPG * nkv), path(2); Buf<long long> stray(2), tail(2);
        Buf<float> qkv((size_t)ROWS * LDQ), rc((size_t)MS * 64), rs((size_t)MS * 64), kc((size_t)NS * nkv * MS * HD), vc((size_t)NS * nkv * MS * HD), out((size_t)ROWS * LDO);
        auto reset = [&] { len[0] = 1; len[1] = 130; len[2] = 48; for (int i = 0; i < NS * NPG; ++i) slots[(size_t)i] = 31 - i; };
        auto args = [&](int layout) {
            q3_attn_prefill_packed_ex_args a; memset(&a, 0, sizeof a);
            a.n_seq = NS; a.nh = nh; a.nkv = nkv; a.max_seq = MS; a.ld_qkv = LDQ; a.ld_out = LDO; a.kernel = -1; a.eps = 1e-6f; a.seq_len = len; a.path = path; a.plane_tail = tail;
            a.qkv = qkv; a.q_norm_w = qw; a.k_norm_w = kw; a.rope_cos = rc; a.rope_sin = rs; a.kcache = kc; a.vcache = vc; a.out = out;
            a.layout = layout; a.n_layers = 1; a.layer = 0; a.n_slabs = 1; a.page_slots = slots; a.rot_used = rot; a.stray = stray;
            return a;
        };
        auto run = [&](const q3_attn_prefill_packed_ex_args& a) { Buf<q3_attn_prefill_packed_ex_args> bb(1); bb[0] = a; return (int)q3_attn_prefill_packed_ex(0, bb); };
        reset(); expect_no_device(W, run(args(0))); expect_no_device(W, run(args(1)));
        len[1] = 131; expect(W, 0, run(args(0)), Q3_INVALID_ARG); len[1] = 0; expect(W, 1, run(args(0)), Q3_INVALID_ARG); len[1] = INT_MAX; expect(W, 2, run(args(0)), Q3_INVALID_ARG); len[1] = INT_MIN; expect(W, 3, run(args(0)), Q3_INVALID_ARG); reset();
        slots[5] = slots[0]; expect(W, 4, run(args(1)), Q3_INVALID_ARG); slots[5] = 32; expect(W, 5, run(args(1)), Q3_INVALID_ARG); slots[5] = -1; expect(W, 6, run(args(1)), Q3_INVALID_ARG); reset();
        q3_attn_prefill_packed_ex_args a = args(2); expect(W, 7, run(a), Q3_UNSUPPORTED); a = args(-1); expect(W, 8, run(a), Q3_INVALID_ARG); a = args(0); a.kernel = 0; expect(W, 9, run(a), Q3_INVALID_ARG);
        a = args(0); a.kernel = 1; expect(W, 10, run(a), Q3_INVALID_ARG); a = args(0); a.n_seq = 0; expect(W, 11, run(a), Q3_INVALID_ARG); a = args(0); a.n_seq = 65; expect(W, 12, run(a), Q3_INVALID_ARG);
        a = args(0); a.max_seq = 8193; expect(W, 13, run(a), Q3_INVALID_ARG); a = args(0); a.max_seq = 0; expect(W, 14, run(a), Q3_INVALID_ARG); a = args(0); a.nh = 8; expect(W, 15, run(a), Q3_INVALID_ARG);
        a = args(0); a.ld_qkv = LDQ - 4; expect(W, 16, run(a), Q3_INVALID_ARG); a = args(0); a.ld_out = LDO + 2; expect(W, 17, run(a), Q3_INVALID_ARG);
        a = args(1); a.n_layers = 5; expect(W, 18, run(a), Q3_INVALID_ARG); a = args(1); a.layer = 1; expect(W, 19, run(a), Q3_INVALID_ARG); a = args(1); a.page_slots = nullptr; expect(W, 20, run(a), Q3_INVALID_ARG);
        a = args(0); a.seq_len = nullptr; expect(W, 21, run(a), Q3_INVALID_ARG); a = args(0); a.qkv = nullptr; expect(W, 22, run(a), Q3_INVALID_ARG);
        // more than 16384 rows together: three sequences of 8192 (the arrays are never reached)
        { Buf<int> big(3); big[0] = big[1] = big[2] = 8192; a = args(0); a.max_seq = 8192; a.seq_len = big; expect(W, 23, run(a), Q3_INVALID_ARG); }
    }
}

}  // namespace

int cmd_refusals() {
    refusals_sampler_and_seam();
    refusals_conv_gemm();
    refusals_attention();
    refusals_null_handles();
    refusals_row_move();
    refusals_ref_audio();
    refusals_movers();
    refusals_prompt_rows();
    return finish("refusals");
}
