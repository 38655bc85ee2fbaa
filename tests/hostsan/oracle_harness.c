/* Host-sanitizer harness of the CPU oracle (built by tests/hostsan/build.sh oracle, run by
 * tests/test_host_sanitizers.py).
 *
 * The oracle is the referee of every parity test; here its three C files are compiled with AddressSanitizer +
 * UndefinedBehaviorSanitizer (the flags of oracle/Makefile otherwise, OpenMP kept, two threads) and linked with this program.
 *   oracle_harness primitives       the stand-alone pieces at their edges
 *   oracle_harness e2e <job file>   a model, four sessions of four frames (preset, VoiceDesign, x-vector, ICL), the decodes of their
 *                                   codes, and one clip through each voice-clone encoder, at the tiny configurations
 * Every buffer is a heap block of exactly the size the oracle's header states. No result is compared — the suite does that
 * elsewhere; the run has to be sanitizer-clean and leak-free. Each sub-command ends with "<name>: N cases, M accepted, K refused".
 *
 * The job file (text, written by the test from the library's manifest-only handles and tests/oracle.py's structures):
 *   config <hex bytes of q3o_config> | spk_config <hex> | mimi_config <hex>
 *   tensor | spk_tensor | mimi_tensor  <name> <elements> <scale> <offset>      values are drawn here: offset + scale * z
 */
#include "q3_oracle.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static long g_cases = 0, g_ok = 0, g_refused = 0;

static void die(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    fprintf(stdout, "HARNESS FAILURE: "); vfprintf(stdout, fmt, ap); fprintf(stdout, "\n");
    va_end(ap);
    fflush(stdout);
    exit(1);
}
static void tally(int accepted) { ++g_cases; if (accepted) ++g_ok; else ++g_refused; }
static int finish(const char* name) {
    printf("%s: %ld cases, %ld accepted, %ld refused\n", name, g_cases, g_ok, g_refused);
    fflush(stdout);
    return 0;
}
/* exactly `bytes` bytes (0 bytes: a block every access to which is reported) */
static void* xalloc(size_t bytes) {
    void* p = malloc(bytes);
    if (!p) die("out of memory (%zu bytes)", bytes);
    memset(p, 0, bytes);
    return p;
}
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static float rnd(void) {                                   /* roughly N(0, 1): twelve uniforms */
    float s = 0.0f;
    for (int i = 0; i < 12; ++i) { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; s += (float)(g_rng >> 40) / 16777216.0f; }
    return s - 6.0f;
}
static float* fvec(size_t n, float scale, float offset) {
    float* p = (float*)xalloc(n * sizeof(float));
    for (size_t i = 0; i < n; ++i) p[i] = offset + scale * rnd();
    return p;
}

/* ================================================================================================================================ */
static void prim_linear_norm(void) {
    const int shapes[][3] = {{1, 1, 1}, {1, 7, 5}, {3, 64, 33}, {9, 17, 128}, {2, 1, 257}};
    for (size_t s = 0; s < sizeof shapes / sizeof shapes[0]; ++s) {
        const int M = shapes[s][0], N = shapes[s][1], K = shapes[s][2];
        float *x = fvec((size_t)M * K, 1, 0), *w = fvec((size_t)N * K, 0.1f, 0), *b = fvec((size_t)N, 0.1f, 0), *y = fvec((size_t)M * N, 0, 0);
        q3o_linear(x, w, b, y, M, N, K); tally(1);
        q3o_linear(x, w, NULL, y, M, N, K); tally(1);
        free(x); free(w); free(b); free(y);
        /* the norms over [rows][cols] */
        const int rows = M, cols = K;
        float *a = fvec((size_t)rows * cols, 1, 0), *r = fvec((size_t)rows * cols, 1, 0), *g = fvec((size_t)cols, 0.02f, 1), *o = fvec((size_t)rows * cols, 0, 0),
              *sum = fvec((size_t)rows * cols, 0, 0);
        q3o_rms_norm(a, g, o, rows, cols, 1e-6f); tally(1);
        q3o_fused_residual_rmsnorm(a, r, g, rows, cols, 1e-6f, o, sum); tally(1);
        memset(a, 0, (size_t)rows * cols * sizeof(float));          /* a zero row: 1 / sqrt(eps) */
        q3o_rms_norm(a, g, o, rows, cols, 1e-6f); tally(1);
        free(a); free(r); free(g); free(o); free(sum);
    }
    const int rope[][3] = {{128, 0, 1}, {128, 0, 17}, {64, 4095, 3}, {2, 0, 1}, {128, 7, 0}};
    for (size_t s = 0; s < sizeof rope / sizeof rope[0]; ++s) {
        const int hd = rope[s][0], pos0 = rope[s][1], np = rope[s][2];
        float *c = fvec((size_t)np * (hd / 2), 0, 0), *sn = fvec((size_t)np * (hd / 2), 0, 0);
        q3o_rope_table(1e6f, hd, pos0, np, c, sn); tally(1);
        q3o_rope_table(1e4f, hd, pos0, np, c, sn); tally(1);
        free(c); free(sn);
    }
}

static void prim_sampling(void) {
    const int vocabs[] = {1, 2, 7, 1024, 1025, 3072};
    for (size_t vi = 0; vi < sizeof vocabs / sizeof vocabs[0]; ++vi) {
        const int V = vocabs[vi];
        for (int kind = 0; kind < 4; ++kind) {                    /* random / all equal / all -inf / one finite among -inf */
            float* base = fvec((size_t)V, 3, 0);
            for (int i = 0; i < V; ++i) base[i] = kind == 0 ? base[i] : kind == 1 ? 0.5f : (kind == 3 && i == V / 2) ? 1.0f : -INFINITY;
            float* l = (float*)xalloc((size_t)V * sizeof(float));
            uint8_t* seen = (uint8_t*)xalloc((size_t)V);
            for (int i = 0; i < V; i += 3) seen[i] = 1;
            const int ks[] = {0, 1, V, V + 1, -1, 50};
            for (size_t k = 0; k < sizeof ks / sizeof ks[0]; ++k) { memcpy(l, base, (size_t)V * sizeof(float)); q3o_top_k_filter(l, V, ks[k]); tally(1); }
            const double ps[] = {0.0, 1.0, 0.9, 1e-9, 0.999999};
            for (size_t k = 0; k < sizeof ps / sizeof ps[0]; ++k) { memcpy(l, base, (size_t)V * sizeof(float)); q3o_top_p_filter(l, V, ps[k]); tally(1); }
            const double reps[] = {1.0, 1.05, 1.5, 0.5};
            const int eos[] = {-1, 0, V - 1, V, 2150};
            for (size_t r = 0; r < sizeof reps / sizeof reps[0]; ++r)
                for (size_t e = 0; e < sizeof eos / sizeof eos[0]; ++e)
                    for (int tc = 0; tc < 4; tc += 3) { memcpy(l, base, (size_t)V * sizeof(float)); q3o_apply_penalties(l, V, seen, reps[r], tc, 2, eos[e]); tally(1); }
            uint8_t* mask = (uint8_t*)xalloc((size_t)V);
            for (size_t e = 0; e < sizeof eos / sizeof eos[0]; ++e) { q3o_build_suppression_mask(V, eos[e], mask); tally(1); }
            free(mask);
            uint64_t* st = (uint64_t*)xalloc(sizeof(uint64_t));
            q3o_rng_seed(42, st);
            const double temps[] = {0.0, 0.005, 0.9, 1.0, 100.0};
            for (size_t t = 0; t < sizeof temps / sizeof temps[0]; ++t)
                for (size_t k = 0; k < sizeof ks / sizeof ks[0]; ++k)
                    for (size_t p = 0; p < sizeof ps / sizeof ps[0]; ++p) {
                        const uint32_t tok = q3o_sample(base, V, temps[t], ks[k], ps[p], st);
                        if (tok >= (uint32_t)V) die("q3o_sample: token %u of %d", tok, V);
                        tally(1);
                    }
            for (int i = 0; i < 1000; ++i) { const float u = q3o_rng_next(st); if (!(u >= 0.0f && u <= 1.0f)) die("q3o_rng_next: %g", (double)u); }
            tally(1);
            free(st); free(seen); free(l); free(base);
        }
    }
    for (int n = 0; n < 9; n += 4) {
        uint32_t* fr = (uint32_t*)xalloc((size_t)n * 16 * sizeof(uint32_t)); int64_t* t = (int64_t*)xalloc((size_t)n * 16 * sizeof(int64_t));
        q3o_codes_to_tensor(fr, n, t); tally(1);
        free(fr); free(t);
    }
}

static void prim_convs(void) {
    /* cin, cout, L, k, dil, groups: L below the kernel and below the dilated reach, dilation 9, groups, depthwise */
    const int cc[][6] = {{4, 6, 1, 7, 1, 1}, {4, 6, 3, 7, 9, 1}, {4, 6, 64, 7, 9, 1}, {8, 8, 5, 7, 1, 8}, {8, 4, 33, 3, 2, 2}, {1, 1, 1, 1, 1, 1}, {16, 16, 100, 1, 1, 1}, {6, 6, 55, 7, 3, 3}};
    for (size_t s = 0; s < sizeof cc / sizeof cc[0]; ++s) {
        const int cin = cc[s][0], cout = cc[s][1], L = cc[s][2], k = cc[s][3], dil = cc[s][4], g = cc[s][5];
        float *x = fvec((size_t)cin * L, 1, 0), *w = fvec((size_t)cout * (cin / g) * k, 0.2f, 0), *b = fvec((size_t)cout, 0.1f, 0), *y = fvec((size_t)cout * L, 0, 0);
        q3o_causal_conv1d(x, w, b, y, cin, cout, L, k, dil, g); tally(1);
        q3o_causal_conv1d(x, w, NULL, y, cin, cout, L, k, dil, g); tally(1);
        free(x); free(w); free(b); free(y);
    }
    /* cin, cout, L, k, stride: k = 2 stride (the decoder's), k = stride, k < stride, one column */
    const int tc[][5] = {{4, 6, 1, 16, 8}, {4, 6, 9, 16, 8}, {3, 2, 7, 2, 2}, {3, 2, 7, 3, 5}, {8, 4, 13, 6, 3}, {1, 1, 1, 1, 1}, {2, 2, 5, 7, 2}};
    for (size_t s = 0; s < sizeof tc / sizeof tc[0]; ++s) {
        const int cin = tc[s][0], cout = tc[s][1], L = tc[s][2], k = tc[s][3], st = tc[s][4];
        const int trim = k > st ? k - st : 0, Lout = (L - 1) * st + k - trim;
        float *x = fvec((size_t)cin * L, 1, 0), *w = fvec((size_t)cin * cout * k, 0.2f, 0), *b = fvec((size_t)cout, 0.1f, 0), *y = fvec((size_t)cout * Lout, 0, 0);
        q3o_causal_trans_conv1d(x, w, b, y, cin, cout, L, k, st); tally(1);
        q3o_causal_trans_conv1d(x, w, NULL, y, cin, cout, L, k, st); tally(1);
        free(x); free(w); free(b); free(y);
    }
    const int sb[][2] = {{1, 1}, {3, 17}, {96, 5}, {7, 1}};
    for (size_t s = 0; s < sizeof sb / sizeof sb[0]; ++s) {
        const int C = sb[s][0], L = sb[s][1];
        for (int kind = 0; kind < 3; ++kind) {                    /* ordinary / beta very negative (the 1e-9 guard) / large alpha */
            float *x = fvec((size_t)C * L, 2, 0), *a = fvec((size_t)C, 0.1f, kind == 2 ? 80.0f : 0.0f), *be = fvec((size_t)C, 0.1f, kind == 1 ? -100.0f : 0.0f), *y = fvec((size_t)C * L, 0, 0);
            q3o_snake_beta(x, a, be, y, C, L); tally(1);
            free(x); free(a); free(be); free(y);
        }
    }
}

static void prim_speaker(void) {
    /* C, T, pl, pr: the widest pads a reflect padding admits (T - 1), none, one column cannot be padded */
    const int rp[][4] = {{1, 2, 1, 1}, {3, 9, 8, 8}, {3, 9, 0, 0}, {2, 5, 4, 0}, {2, 5, 0, 4}, {4, 1, 0, 0}};
    for (size_t s = 0; s < sizeof rp / sizeof rp[0]; ++s) {
        const int C = rp[s][0], T = rp[s][1], pl = rp[s][2], pr = rp[s][3];
        float *x = fvec((size_t)C * T, 1, 0), *o = fvec((size_t)C * (T + pl + pr), 0, 0);
        q3o_reflect_pad_1d(x, C, T, pl, pr, o); tally(1);
        free(x); free(o);
    }
    /* the mel front end: clips shorter than one frame, the shortest with one (256 samples), frame boundaries */
    const int ns[] = {1, 2, 255, 256, 383, 384, 385, 511, 512, 4000};
    for (size_t s = 0; s < sizeof ns / sizeof ns[0]; ++s) {
        const int n = ns[s], T = q3o_mel_frames(n, 1024, 256);
        if (T < 0 || T != (n + 768 < 1024 ? 0 : (n + 768 - 1024) / 256 + 1)) die("q3o_mel_frames(%d) = %d", n, T);
        float *x = fvec((size_t)n, 0.3f, 0), *mel = fvec((size_t)128 * T, 0, 0);
        const int got = q3o_mel_speaker(x, n, mel, T);
        if (got != T) die("q3o_mel_speaker(%d) = %d, %d frames expected", n, got, T);
        tally(1);
        if (T > 0) { float* shrt = fvec((size_t)128 * (T - 1), 0, 0); if (q3o_mel_speaker(x, n, shrt, T - 1) != -1) die("q3o_mel_speaker took a short buffer"); tally(0); free(shrt); }
        free(x); free(mel);
    }
    { float* x = fvec(4, 1, 0); if (q3o_mel_speaker(x, 0, x, 0) != -1) die("q3o_mel_speaker(0 samples)"); tally(0); free(x); }
    { float* w = fvec(1024, 0, 0); q3o_hann_window(1024, w); tally(1); free(w); w = fvec(1, 0, 0); q3o_hann_window(1, w); tally(1); free(w); }
    { float* fb = fvec((size_t)128 * 513, 0, 0); q3o_mel_filterbank(24000, 1024, 128, 0.0f, 12000.0f, fb); tally(1); free(fb); }
    /* frame counts of the speech encoder */
    q3o_mimi_config* mc = (q3o_mimi_config*)xalloc(sizeof *mc);
    mc->ratios[0] = 4; mc->ratios[1] = 5; mc->ratios[2] = 6; mc->ratios[3] = 8;
    const int64_t lens[] = {0, -1, 1, 1919, 1920, 1921, 24000 * 120, 1ll << 40};
    for (size_t s = 0; s < sizeof lens / sizeof lens[0]; ++s) {
        const int T = q3o_mimi_frames(mc, lens[s]);
        if (lens[s] >= 1 && (int64_t)T != (lens[s] + 1919) / 1920) die("q3o_mimi_frames(%lld) = %d", (long long)lens[s], T);
        tally(T > 0);
    }
    free(mc);
}

static int cmd_primitives(void) {
    prim_linear_norm();
    prim_sampling();
    prim_convs();
    prim_speaker();
    return finish("primitives");
}

/* ================================================================================================================================ */
typedef struct { char kind[16]; char name[240]; long long n; double scale, offset; } job_tensor;
typedef struct { unsigned char cfg[256], spk[256], mimi[256]; size_t n_cfg, n_spk, n_mimi; job_tensor* t; size_t nt; } job;

static size_t unhex(const char* s, unsigned char* out, size_t cap) {
    size_t n = 0;
    while (s[0] && s[1] && s[0] != '\n') {
        unsigned v; if (sscanf(s, "%2x", &v) != 1) die("bad hex in the job file");
        if (n >= cap) die("config of the job file too long");
        out[n++] = (unsigned char)v; s += 2;
    }
    return n;
}
static void job_read(const char* path, job* j) {
    memset(j, 0, sizeof *j);
    FILE* f = fopen(path, "r");
    if (!f) die("cannot open the job file %s", path);
    size_t cap = 0; char line[1024];
    while (fgets(line, sizeof line, f)) {
        char kind[32] = "", rest[900] = "";
        if (sscanf(line, "%31s %899[^\n]", kind, rest) < 2) continue;
        if (!strcmp(kind, "config")) j->n_cfg = unhex(rest, j->cfg, sizeof j->cfg);
        else if (!strcmp(kind, "spk_config")) j->n_spk = unhex(rest, j->spk, sizeof j->spk);
        else if (!strcmp(kind, "mimi_config")) j->n_mimi = unhex(rest, j->mimi, sizeof j->mimi);
        else if (!strcmp(kind, "tensor") || !strcmp(kind, "spk_tensor") || !strcmp(kind, "mimi_tensor")) {
            if (j->nt == cap) { cap = cap ? 2 * cap : 256; j->t = (job_tensor*)realloc(j->t, cap * sizeof(job_tensor)); if (!j->t) die("out of memory"); }
            job_tensor* t = &j->t[j->nt];
            snprintf(t->kind, sizeof t->kind, "%s", kind);
            if (sscanf(rest, "%239s %lld %lf %lf", t->name, &t->n, &t->scale, &t->offset) != 4 || t->n < 1 || t->n > (1ll << 28)) die("bad tensor line: %s", line);
            ++j->nt;
        } else die("unknown line in the job file: %s", line);
    }
    fclose(f);
    if (j->n_cfg != sizeof(q3o_config) || j->n_spk != sizeof(q3o_spk_config) || j->n_mimi != sizeof(q3o_mimi_config))
        die("the job file's structures have %zu / %zu / %zu bytes, the oracle's %zu / %zu / %zu", j->n_cfg, j->n_spk, j->n_mimi, sizeof(q3o_config),
            sizeof(q3o_spk_config), sizeof(q3o_mimi_config));
}
/* a tensor of the job, drawn here; usage counts are divisors and stay positive */
static float* job_values(const job_tensor* t) {
    float* v = fvec((size_t)t->n, (float)t->scale, (float)t->offset);
    const size_t ln = strlen(t->name);
    if (ln >= 13 && !strcmp(t->name + ln - 13, "cluster_usage")) for (long long i = 0; i < t->n; ++i) v[i] = 0.5f + fabsf(v[i]);
    return v;
}

static void e2e_model(const job* j) {
    q3o_config* cfg = (q3o_config*)xalloc(sizeof *cfg);
    memcpy(cfg, j->cfg, sizeof *cfg);
    q3o_model* m = q3o_model_new(cfg);
    if (!m) die("q3o_model_new: %s", q3o_last_error());
    size_t loaded = 0;
    for (size_t i = 0; i < j->nt; ++i) {
        if (strcmp(j->t[i].kind, "tensor")) continue;
        float* v = job_values(&j->t[i]);
        if (q3o_model_set_tensor(m, j->t[i].name, v, j->t[i].n) != 0) die("q3o_model_set_tensor(%s, %lld): %s", j->t[i].name, j->t[i].n, q3o_last_error());
        free(v); ++loaded; tally(1);
    }
    if (!loaded) die("the job file names no model tensor");
    if (q3o_model_finalize(m, 3) != 0) die("q3o_model_finalize: %s", q3o_last_error());
    tally(1);
    const int H = cfg->hidden, V = cfg->codec_vocab, CPV = cfg->cp_vocab;
    for (int kind = 0; kind < 4; ++kind) {                        /* preset, VoiceDesign, x-vector, ICL */
        const int n_text = 5 + kind, n_ins = 11, n_ref = 3, n_ref_text = 4;
        uint32_t* text = (uint32_t*)xalloc((size_t)n_text * 4); for (int i = 0; i < n_text; ++i) text[i] = (uint32_t)(100 + 37 * i);
        uint32_t* ins = (uint32_t*)xalloc((size_t)n_ins * 4); for (int i = 0; i < n_ins; ++i) ins[i] = (uint32_t)(5000 + 11 * i);
        uint32_t* ref = (uint32_t*)xalloc((size_t)n_ref * 16 * 4); for (int i = 0; i < n_ref * 16; ++i) ref[i] = (uint32_t)((i * 53) % 2048);
        uint32_t* ref_text = (uint32_t*)xalloc((size_t)n_ref_text * 4); for (int i = 0; i < n_ref_text; ++i) ref_text[i] = (uint32_t)(900 + i);
        float* xvec = fvec((size_t)H, 0.5f, 0);
        q3o_request* r = (q3o_request*)xalloc(sizeof *r);
        r->text_ids = text; r->n_text = n_text; r->speaker_id = 3000; r->language_id = 2050;
        r->opts.temperature = 0.9; r->opts.top_p = 0.9; r->opts.repetition_penalty = 1.05; r->opts.seed = 42 + (uint64_t)kind; r->opts.has_seed = 1;
        r->opts.max_length = 4; r->opts.top_k = 50; r->opts.eos_token_id = -1; r->opts.chunk_frames = 10; r->opts.min_new_tokens = 2;
        if (kind == 0) r->mode = Q3O_MODE_CUSTOM_VOICE;
        else if (kind == 1) { r->mode = Q3O_MODE_VOICE_DESIGN; r->instruct_ids = ins; r->n_instruct = n_ins; }
        else { r->mode = Q3O_MODE_VOICE_CLONE; r->xvector = xvec; if (kind == 3) { r->ref_codes = ref; r->n_ref = n_ref; r->ref_text_ids = ref_text; r->n_ref_text = n_ref_text; } }
        q3o_session* s = q3o_session_new(m, r);
        if (!s) die("q3o_session_new (prompt kind %d): %s", kind, q3o_last_error());
        tally(1);
        const int P = q3o_session_prefill_len(s), TT = q3o_session_trailing_len(s);
        double rep = 0; int max_len = 0;
        q3o_session_effective(s, &rep, &max_len);
        if (P < 1 || TT < 1 || max_len != 4) die("session of prompt kind %d: prefill %d, trailing %d, max_length %d", kind, P, TT, max_len);
        float *lh = fvec((size_t)H, 0, 0), *lg = fvec((size_t)V, 0, 0), *emb = fvec((size_t)P * H, 0, 0), *tr = fvec((size_t)TT * H, 0, 0), *pad = fvec((size_t)H, 0, 0);
        q3o_session_prefill_out(s, lh, lg); q3o_session_prefill_embeds(s, emb); q3o_session_trailing(s, tr, pad);
        tally(1);
        uint32_t* codes = (uint32_t*)xalloc((size_t)max_len * 16 * 4);
        float *tl = fvec((size_t)(max_len + 1) * V, 0, 0), *cl = fvec((size_t)max_len * 15 * CPV, 0, 0);
        const int nf = q3o_session_generate(s, codes, tl, cl);
        if (nf != 4) die("prompt kind %d generated %d frames, 4 expected (no EOS id)", kind, nf);
        tally(1);
        /* the teacher-forced single steps and the frame glue */
        float *hid = fvec((size_t)H, 0, 0), *sem = fvec((size_t)H, 0.1f, 0), *cpl = fvec((size_t)15 * CPV, 0, 0), *fe = fvec((size_t)H, 0, 0);
        uint32_t* c15 = (uint32_t*)xalloc(15 * 4);
        q3o_session_talker_step(s, sem, hid, lg); q3o_session_cp_generate(s, hid, sem, c15, cpl); q3o_session_cp_generate(s, hid, sem, c15, NULL);
        q3o_frame_embed(m, codes[0] % (uint32_t)V, c15, tr, fe);
        tally(1);
        q3o_session_free(s);
        /* decode the four frames, plain and with every tap */
        int64_t* ct = (int64_t*)xalloc((size_t)nf * 16 * 8);
        q3o_codes_to_tensor(codes, nf, ct);
        float* pcm = fvec((size_t)1920 * nf, 0, 0);
        if (q3o_decode(m, ct, nf, pcm) != 1920 * nf) die("q3o_decode: %s", q3o_last_error());
        tally(1);
        float** taps = (float**)xalloc(Q3O_DEC_N * sizeof(float*));
        {
            const int LAT = cfg->dec_latent, Q = cfg->dec_q_dim;
            int L = nf, C = cfg->dec_dim, at = 0;
            taps[at++] = fvec((size_t)Q * L, 0, 0); taps[at++] = fvec((size_t)LAT * L, 0, 0); taps[at++] = fvec((size_t)LAT * L, 0, 0);
            for (int u = 0; u < 2; ++u) { L *= cfg->dec_up_ratios[u]; taps[at++] = fvec((size_t)LAT * L, 0, 0); }
            taps[at++] = fvec((size_t)C * L, 0, 0);
            for (int u = 0; u < 4; ++u) { L *= cfg->dec_up_rates[u]; C /= 2; taps[at++] = fvec((size_t)C * L, 0, 0); }
            if (at != Q3O_DEC_N) die("tap count");
        }
        if (q3o_decode_taps(m, ct, nf, pcm, taps) != 1920 * nf) die("q3o_decode_taps: %s", q3o_last_error());
        tally(1);
        { float* keep = taps[3]; taps[3] = NULL; if (q3o_decode_taps(m, ct, nf, pcm, taps) != 1920 * nf) die("q3o_decode_taps with a null tap"); taps[3] = keep; tally(1); }
        if (q3o_decode_taps(m, ct, nf, pcm, NULL) != 1920 * nf) die("q3o_decode_taps without taps");
        tally(1);
        for (int i = 0; i < Q3O_DEC_N; ++i) free(taps[i]);
        free(taps); free(pcm); free(ct); free(c15); free(fe); free(cpl); free(sem); free(hid); free(cl); free(tl); free(codes);
        free(pad); free(tr); free(emb); free(lg); free(lh); free(r); free(xvec); free(ref_text); free(ref); free(ins); free(text);
    }
    { int64_t* one = (int64_t*)xalloc(16 * 8); float* pcm = fvec(1920, 0, 0); if (q3o_decode(m, one, 1, pcm) != 1920) die("q3o_decode of one frame"); tally(1); free(one); free(pcm); }
    q3o_model_free(m);
    free(cfg);
}

static void e2e_encoders(const job* j) {
    q3o_spk_config* sc = (q3o_spk_config*)xalloc(sizeof *sc);
    memcpy(sc, j->spk, sizeof *sc);
    q3o_spk* sp = q3o_spk_new(sc);
    if (!sp) die("q3o_spk_new: %s", q3o_spk_last_error());
    size_t loaded = 0;
    for (size_t i = 0; i < j->nt; ++i) {
        if (strcmp(j->t[i].kind, "spk_tensor")) continue;
        float* v = job_values(&j->t[i]);
        if (q3o_spk_set_tensor(sp, j->t[i].name, v, j->t[i].n) != 0) die("q3o_spk_set_tensor(%s, %lld): %s", j->t[i].name, j->t[i].n, q3o_spk_last_error());
        free(v); ++loaded; tally(1);
    }
    if (!loaded) die("the job file names no speaker-encoder tensor");
    {
        const int n = 6000;
        float *x = fvec((size_t)n, 0.2f, 0), *out = fvec((size_t)sc->enc_dim, 0, 0);
        if (q3o_spk_encode(sp, x, n, out) != 0) die("q3o_spk_encode: %s", q3o_spk_last_error());
        tally(1);
        const int T = q3o_mel_frames(n, 1024, 256);
        float* mel = fvec((size_t)sc->mel_dim * T, 0, 0);
        if (q3o_mel_speaker(x, n, mel, T) != T) die("q3o_mel_speaker");
        float** taps = (float**)xalloc(6 * sizeof(float*));
        for (int i = 0; i < 4; ++i) taps[i] = fvec((size_t)sc->channels[i] * T, 0, 0);
        taps[4] = fvec((size_t)sc->channels[4] * T, 0, 0); taps[5] = fvec((size_t)2 * sc->channels[4], 0, 0);
        if (q3o_spk_forward(sp, mel, T, out, taps) != 0) die("q3o_spk_forward: %s", q3o_spk_last_error());
        tally(1);
        if (q3o_spk_forward(sp, mel, T, out, NULL) != 0) die("q3o_spk_forward without taps");
        tally(1);
        /* a clip too short for the reflect padding is refused */
        if (q3o_spk_encode(sp, x, 300, out) == 0) die("q3o_spk_encode took a clip of one mel frame");
        tally(0);
        for (int i = 0; i < 6; ++i) free(taps[i]);
        free(taps); free(mel); free(x); free(out);
    }
    q3o_spk_free(sp);
    free(sc);

    q3o_mimi_config* mc = (q3o_mimi_config*)xalloc(sizeof *mc);
    memcpy(mc, j->mimi, sizeof *mc);
    q3o_mimi* mm = q3o_mimi_new(mc);
    if (!mm) die("q3o_mimi_new failed");
    loaded = 0;
    for (size_t i = 0; i < j->nt; ++i) {
        if (strcmp(j->t[i].kind, "mimi_tensor")) continue;
        float* v = job_values(&j->t[i]);
        if (q3o_mimi_set_tensor(mm, j->t[i].name, v, j->t[i].n) != 0) die("q3o_mimi_set_tensor(%s, %lld): %s", j->t[i].name, j->t[i].n, q3o_mimi_last_error(mm));
        free(v); ++loaded; tally(1);
    }
    if (!loaded) die("the job file names no speech-encoder tensor");
    const int64_t lens[] = {1, 95, 96, 97, 1000};
    for (size_t s = 0; s < sizeof lens / sizeof lens[0]; ++s) {
        const int64_t n = lens[s];
        const int T = q3o_mimi_frames(mc, n);
        int64_t T25 = n; for (int i = 0; i < 4; ++i) T25 = (T25 + mc->ratios[i] - 1) / mc->ratios[i];
        float* x = fvec((size_t)n, 0.2f, 0);
        uint32_t* codes = (uint32_t*)xalloc((size_t)T * (size_t)mc->n_q * 4);
        int got = q3o_mimi_encode(mm, x, n, codes, NULL);
        if (got != T) die("q3o_mimi_encode(%lld) = %d, %d frames expected: %s", (long long)n, got, T, q3o_mimi_last_error(mm));
        tally(1);
        float** taps = (float**)xalloc(4 * sizeof(float*));
        taps[0] = fvec((size_t)mc->hidden * (size_t)T25, 0, 0); taps[1] = fvec((size_t)mc->hidden * (size_t)T25, 0, 0); taps[2] = fvec((size_t)mc->hidden * (size_t)T, 0, 0);
        taps[3] = fvec((size_t)T * (size_t)mc->n_q, 0, 0);
        got = q3o_mimi_encode(mm, x, n, codes, taps);
        if (got != T) die("q3o_mimi_encode with taps");
        tally(1);
        for (int i = 0; i < 4; ++i) free(taps[i]);
        free(taps); free(codes); free(x);
    }
    q3o_mimi_free(mm);
    free(mc);
}

static int cmd_e2e(const char* path) {
    job j;
    job_read(path, &j);
    e2e_model(&j);
    e2e_encoders(&j);
    free(j.t);
    return finish("e2e");
}

int main(int argc, char** argv) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    q3o_set_threads(2);
    if (argc > 1 && !strcmp(argv[1], "primitives")) return cmd_primitives();
    if (argc > 2 && !strcmp(argv[1], "e2e")) return cmd_e2e(argv[2]);
    fprintf(stderr, "usage: %s primitives | e2e <job file>\n", argv[0]);
    return 2;
}
