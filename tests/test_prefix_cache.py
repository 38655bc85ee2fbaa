"""Prefix cache (-m gpu): the prefilled K/V pages of a VoiceDesign instruction are linked
into later requests with the same instruction and the prefill starts at the first position that is not cached. A hit must be
invisible except in time, so every comparison is np.array_equal — first logits, 6 frames of codes, PCM where named — against
the SAME request with the cache OFF (today's code, held to the oracle elsewhere), never against another cached run. Every
request under test hits pages a DONOR inserted: the same instruction with another text, language and seed."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import api, synth
from common import synthetic_prompt, gqa_config

pytestmark = pytest.mark.gpu
F = 6
OPTS = q.SynthesisOptions(max_length=F, eos_token_id=None, seed=7)


def ins(n, index=50):
    return [int(x) for x in synthetic_prompt(n, index)]


def req(instr, k=0):
    """the request under test (k = 0) or a donor (k > 0): same instruction, other text, language and seed"""
    lang = [q.Language.German, q.Language.English, q.Language.French][k % 3]
    return q.Utterance(synthetic_prompt(9 + 2 * k, 3 + k), language=lang, instruct_ids=list(instr), seed=40 + k)


def run(m, utts, frames=F, pcm=False, opts=OPTS, embeds=False, **kw):
    """prefill + frames of one session: per row (first logits, codes, reused positions[, prompt embeddings]), PCM of row 0 if asked"""
    s = m.session(utts, opts, **kw)
    s.prefill()
    lg = [s.get(2, (m.config.codec_vocab,), b) for b in range(len(utts))]
    re = [s.prefix_info(b) for b in range(len(utts))]
    em = [s.get(0, (s.prefill_len(b)[0], m.config.hidden), b) for b in range(len(utts))] if embeds else None
    s.generate(frames)
    out = [(lg[b], s.codes(b), re[b]) + ((em[b],) if embeds else ()) for b in range(len(utts))]
    wave = s.decode(0) if pcm else None
    s.close()
    return (out, wave) if pcm else out


def same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[1].shape == (F, 16)


@pytest.fixture(scope="module")
def models():
    """tiny models by heads / kv-heads ratio (2 = q.tiny()), built on first use; each test leaves the cache off and empty"""
    made = {}

    def get(ratio=2):
        if ratio not in made:
            made[ratio] = q.Qwen3TTS.from_synthetic(q.tiny() if ratio == 2 else gqa_config(ratio), device=0, seed=1234)
        return made[ratio]
    yield get
    for m in made.values():
        m.prefix_cache(0)
        assert m.kv_pool_info()["pages_in_use"] == 0
        m.close()


@pytest.fixture
def gm(models):
    m = models(2)
    assert m.prefix_cache_info()["pages_cached"] == 0 and m.kv_pool_info()["pages_in_use"] == 0
    yield m
    m.prefix_cache(0)
    assert m.kv_pool_info()["pages_in_use"] == 0


def hit_miss_off(m, instr, pcm=False):
    """the request with the cache off, as a miss (nothing cached) and as a hit on the donor's pages"""
    u, donor = req(instr), req(instr, 1)
    m.prefix_cache(0)
    off = run(m, [u], pcm=pcm)
    m.prefix_cache(64)
    miss = run(m, [u], pcm=pcm)
    m.prefix_cache(0); m.prefix_cache(64)              # empty again: the hit below is on the DONOR's pages
    assert m.prefix_cache_info()["pages_cached"] == 0
    run(m, [donor])
    assert m.prefix_cache_info()["pages_cached"] == len(instr) // 128
    hit = run(m, [u], pcm=pcm)
    m.prefix_cache(0)
    return off, miss, hit


# N instruct tokens -> S = N + 9 prefill positions. 150: below 256 positions (the first-generation attention kernel); 300: bf16x3
# attention without key halves; 1200: key halves + merge, every position a GEMM position; 1160: 1169 positions = 1152 GEMM
# positions, all cached (no GEMM pass runs), + the 17-position decode-step tail
@pytest.mark.parametrize("N,reused", [(150, 128), (300, 256), (1200, 1152), (1160, 1152)])
def test_kernel_regimes(gm, N, reused):
    pcm = N == 300
    off, miss, hit = hit_miss_off(gm, ins(N), pcm=pcm)
    if pcm:
        (off, w_off), (miss, w_miss), (hit, w_hit) = off, miss, hit
        np.testing.assert_array_equal(w_miss, w_off); np.testing.assert_array_equal(w_hit, w_off)
    assert off[0][2] == 0 and miss[0][2] == 0 and hit[0][2] == reused
    same(miss[0], off[0]); same(hit[0], off[0])


def test_gqa_ratio_1_rounds_to_a_query_block(models):
    """256-row query blocks: 1152 cached positions are no block boundary, the passes start at one"""
    m = models(1)
    off, miss, hit = hit_miss_off(m, ins(1200))
    assert hit[0][2] >= 1024 and hit[0][2] % 128 == 0 and miss[0][2] == 0
    same(miss[0], off[0]); same(hit[0], off[0])


def test_gqa_ratio_4_decode_step_schedule(models):
    m = models(4)
    off, miss, hit = hit_miss_off(m, ins(300))
    assert hit[0][2] == 256 and miss[0][2] == 0
    same(miss[0], off[0]); same(hit[0], off[0])


def test_longest_prefix(gm):
    common, a, b = ins(256, 60), ins(100, 61), ins(100, 62)
    ua, ub = req(common + a, 1), req(common + b)
    other = list(common + a); other[5] = (other[5] + 1) % 1000
    uo, short = req(other), req(ins(100, 63))
    off = {k: run(gm, [u])[0] for k, u in (("b", ub), ("o", uo), ("s", short))}
    gm.prefix_cache(64)
    assert run(gm, [ua])[0][2] == 0
    assert gm.prefix_cache_info()["pages_cached"] == 2           # 356 tokens: two whole pages
    hb = run(gm, [ub])[0]
    assert hb[2] == 256; same(hb, off["b"])
    assert gm.prefix_cache_info()["pages_cached"] == 2           # nothing new: both pages were there
    ho = run(gm, [uo])[0]
    assert ho[2] == 0; same(ho, off["o"])                        # differs at token 5: another chain from block 0 on
    n = gm.prefix_cache_info()["pages_cached"]
    hs = run(gm, [short])[0]
    assert hs[2] == 0 and gm.prefix_cache_info()["pages_cached"] == n      # fewer than one eligible page: not looked up, not inserted
    same(hs, off["s"])


def test_longest_prefix_across_lengths_with_key_halves(gm):
    """1000+ positions at GQA ratio 2: a query block is one page, so a cached page's key-half boundary does not depend on the prompt
    length and instructions of different lengths share their common pages"""
    long_ = ins(1300, 64)
    short = long_[:1152] + ins(48, 65)
    off = run(gm, [req(short)])[0]
    gm.prefix_cache(64)
    assert run(gm, [req(long_, 1)])[0][2] == 0
    h = run(gm, [req(short)])[0]
    assert h[2] == 1152; same(h, off)


def test_weights_change_drops_the_cache(gm):
    A = ins(300, 66)
    off = run(gm, [req(A)])[0]
    gm.prefix_cache(64)
    run(gm, [req(A, 1)])
    assert gm.prefix_cache_info()["pages_cached"] == 2
    gm.mark_loaded()                                            # the arena may have been rewritten: cached K/V is stale
    assert gm.prefix_cache_info()["pages_cached"] == 0 and gm.kv_pool_info()["pages_in_use"] == 0
    h = run(gm, [req(A)])[0]
    assert h[2] == 0; same(h, off)


def test_prefill_retried_after_a_failure_links_again(gm):
    """two rows hit, the second row's own page is refused by the pool limit: the failed prefill's linked pages go back, the retry
    links them again (nothing is computed into shared pages) and equals the cache-off session"""
    from qwen3_tts_rs_amd import _lib
    A = ins(300, 67)
    utts = [req(A), req(A, 2)]
    off = run(gm, utts)
    gm.prefix_cache(64)
    run(gm, [req(A, 1)])
    gm.kv_pool_limit(3)                                         # 2 cached + one row's own page; the other row's does not fit
    s = gm.session(utts, OPTS)
    try:
        with pytest.raises(_lib.Q3Error, match="KV page pool exhausted"):
            s.prefill()
        gm.kv_pool_limit(0)
        s.prefill()
        assert [s.prefix_info(b) for b in range(2)] == [256, 256] and gm.kv_pool_info()["pages_in_use"] == 4
        lg = [s.get(2, (gm.config.codec_vocab,), b) for b in range(2)]
        s.generate(F)
        for b in range(2):
            same((lg[b], s.codes(b), 256), off[b])
    finally:
        gm.kv_pool_limit(0); s.close()


def test_batched_rows_with_unequal_hits(gm):
    """one session, three rows of one prefill length: a full hit, a 128-position hit and a miss; each row = its own batch-1 run"""
    A = ins(300, 70)
    half = A[:128] + ins(172, 71)
    C = ins(300, 72)
    utts = [req(A), req(half, 2), req(C, 3)]
    off = [run(gm, [u], embeds=True)[0] for u in utts]
    gm.prefix_cache(64)
    run(gm, [req(A, 1)])                                        # donor
    got = run(gm, utts, embeds=True)
    assert [g[2] for g in got] == [256, 128, 0]
    for g, o in zip(got, off):
        same(g, o)
        np.testing.assert_array_equal(g[3], o[3])               # Q3_GET_PREFILL_EMBEDS of a row prefilled in its own group


def test_ragged_session_with_a_hit(gm):
    """VoiceDesign hit + CustomVoice + x-vector rows in one session. The yardstick of every row is the same session with the
    cache off (first logits and codes), and each row's codes also equal its batch-1 run. First logits against the batch-1 run
    are asserted for the VoiceDesign row, the one the cache touches: a ragged session prefills rows of EQUAL length together
    (the CustomVoice and the x-vector prompt are both 10 positions, one group of two), and the decode-step prefill of a
    two-row group tiles its passes differently from a one-row session's — their logits differ from the batch-1 run's in the
    last bits with the cache off just the same (measured: 3.3e-6 absolute, codes equal)."""
    A = ins(300, 73)
    rng = np.random.default_rng(5)
    utts = [req(A),
            q.Utterance(synthetic_prompt(12, 4), q.Speaker.Ryan, q.Language.English, seed=41),
            q.Utterance(synthetic_prompt(10, 5), language=q.Language.English, xvector=rng.standard_normal(gm.config.hidden).astype(np.float32), seed=42)]
    off1 = [run(gm, [u])[0] for u in utts]
    off = run(gm, utts)                                         # the same session shape, cache off
    gm.prefix_cache(64)
    run(gm, [req(A, 1)])
    got = run(gm, utts)
    assert [g[2] for g in got] == [256, 0, 0]
    for g, o, o1 in zip(got, off, off1):
        same(g, o)
        np.testing.assert_array_equal(g[1], o1[1])
    same(got[0], off1[0])


def test_lifetime(gm):
    A = ins(300, 74)
    before = gm.kv_pool_info()["pages_in_use"]
    o40 = q.SynthesisOptions(max_length=40, eos_token_id=None, seed=7)
    u1, u2 = req(A), req(A, 2)
    off = [run(gm, [u], frames=40, opts=o40)[0] for u in (u1, u2)]
    off6 = run(gm, [u1])[0]
    gm.prefix_cache(64)
    donor = gm.session([req(A, 1)], OPTS); donor.prefill(); donor.close()      # the donor is gone before the hit
    h = run(gm, [u1])[0]
    assert h[2] == 256; same(h, off6)
    # two live sessions on the same pages, frames interleaved
    s1 = gm.session([u1], o40); s2 = gm.session([u2], o40)
    s1.prefill(); s2.prefill()
    assert s1.prefix_info(0) == 256 and s2.prefix_info(0) == 256
    np.testing.assert_array_equal(s1.get(2, (gm.config.codec_vocab,)), off[0][0])
    np.testing.assert_array_equal(s2.get(2, (gm.config.codec_vocab,)), off[1][0])
    info = gm.prefix_cache_info()
    assert info["pages_cached"] == 2 and info["pages_shared"] == 2
    for _ in range(5):
        s1.generate(8); s2.generate(8)
    np.testing.assert_array_equal(s1.codes(0), off[0][1]); np.testing.assert_array_equal(s2.codes(0), off[1][1])
    s1.close(); s2.close()
    info = gm.prefix_cache_info()
    assert info["pages_shared"] == 0 and gm.kv_pool_info()["pages_in_use"] == info["pages_cached"] == 2
    gm.prefix_cache(0)
    assert gm.kv_pool_info()["pages_in_use"] == before
    gm.kv_pool_trim()


def test_eviction_lru(gm):
    instrs = [ins(300, 80 + i) for i in range(3)]
    off = [run(gm, [req(x)])[0] for x in instrs]
    gm.prefix_cache(2)
    for x, o in zip(instrs, off):
        run(gm, [req(x, 1)])                                    # donor of x
        assert gm.prefix_cache_info()["pages_cached"] <= 2
        h = run(gm, [req(x)])[0]
        assert h[2] == 256; same(h, o)
        assert gm.prefix_cache_info()["pages_cached"] <= 2
    assert gm.prefix_cache_info()["evictions"] >= 4
    h = run(gm, [req(instrs[0])])[0]                            # the least recently used one is gone
    assert h[2] == 0; same(h, off[0])
    assert gm.prefix_cache_info()["pages_cached"] <= 2


def test_pool_limit_reclaims_cached_pages(gm):
    A, Bi = ins(300, 84), ins(300, 85)
    off = run(gm, [req(Bi)])[0]
    gm.prefix_cache(64)
    run(gm, [req(A, 1)])
    assert gm.kv_pool_info()["pages_in_use"] == 2               # only the cache holds them
    ev0 = gm.prefix_cache_info()["evictions"]
    gm.kv_pool_limit(4)                                         # the request needs 3 pages: 2 + 3 > 4
    try:
        h = run(gm, [req(Bi)])[0]
    finally:
        gm.kv_pool_limit(0)
    assert gm.prefix_cache_info()["evictions"] > ev0
    assert h[2] == 0; same(h, off)


def test_switching_off_under_a_running_row(gm):
    A = ins(300, 86)
    off = run(gm, [req(A)])[0]
    gm.prefix_cache(64)
    run(gm, [req(A, 1)])
    s = gm.session([req(A)], OPTS); s.prefill()
    assert s.prefix_info(0) == 256
    lg = s.get(2, (gm.config.codec_vocab,))
    s.generate(3)
    gm.prefix_cache(0)                                          # the row keeps the pages it holds
    assert gm.prefix_cache_info()["pages_cached"] == 0 and gm.kv_pool_info()["pages_in_use"] == 3
    s.generate(3)
    same((lg, s.codes(0), 0), off)
    s.close()
    assert gm.kv_pool_info()["pages_in_use"] == 0


def test_bf16_kv_session(gm):
    A = ins(300, 87)
    off = run(gm, [req(A)], kv_bf16=True)[0]
    gm.prefix_cache(64)
    run(gm, [req(A, 1)])
    s = gm.session([req(A)], OPTS, kv_bf16=True); s.prefill()
    assert s.prefix_info(0) == 256
    # 2 cached f32 pages + the row's 3 bf16 pages (half a page each): the row's own f32 page went back, the linked ones stayed cached
    assert gm.kv_pool_info()["pages_in_use"] == 4 and gm.prefix_cache_info()["pages_shared"] == 0
    s.generate(F)
    np.testing.assert_array_equal(s.codes(0), off[1])
    s.close()
    assert gm.kv_pool_info()["pages_in_use"] == gm.prefix_cache_info()["pages_cached"] == 2


def _drain(b, tickets, steps=200):
    for _ in range(steps):
        running, queued, _ = b.step(4)
        if running == 0 and queued == 0:
            break
    return [b.poll(t)[0] for t in tickets]


@pytest.mark.parametrize("limit", [0, 7])
def test_batcher_alternating_instructions(gm, limit):
    """six tickets, two instructions, two slots; limit 7 = two 3-page rows + the page a swap holds for a moment: the cached pages
    of a finished row must not stand in the next request's way"""
    o12 = q.SynthesisOptions(max_length=12, eos_token_id=None, seed=7)
    A, Bi = ins(300, 88), ins(300, 89)
    utts = [req(A if i % 2 == 0 else Bi, i) for i in range(6)]
    off = [run(gm, [u], frames=12, opts=o12)[0] for u in utts]
    gm.prefix_cache(64)
    hp0 = gm.prefix_cache_info()["hit_positions"]
    gm.kv_pool_limit(limit)
    b = q.Batcher(gm, slots=2, frame_budget=12, prompt_budget=320, options=o12)
    try:
        tickets = [b.submit(u, want_pcm=False) for u in utts]
        assert _drain(b, tickets) == [q.Batcher.DONE] * 6
        got = [b.fetch(t)[0] for t in tickets]
    finally:
        b.close(); gm.kv_pool_limit(0)
    for g, o in zip(got, off):
        np.testing.assert_array_equal(g, o[1])
    assert gm.prefix_cache_info()["hit_positions"] - hp0 == 4 * 256


def test_batcher_open_ticket(gm):
    o12 = q.SynthesisOptions(max_length=12, eos_token_id=None, seed=7)
    A = ins(300, 90)
    u = req(A)
    off = run(gm, [u], frames=12, opts=o12)[0]
    gm.prefix_cache(64)
    run(gm, [req(A, 1)])
    hp0 = gm.prefix_cache_info()["hit_positions"]
    b = q.Batcher(gm, slots=2, frame_budget=12, prompt_budget=320, options=o12)
    try:
        text = [int(x) for x in u.text_ids]
        first = q.Utterance(text[:2], language=u.language, instruct_ids=A, seed=u.seed)
        t = b.submit_open(first, want="codes")
        b.append_text(t, text[2:5]); b.step(4)
        b.append_text(t, text[5:], last=True)
        assert _drain(b, [t]) == [q.Batcher.DONE]
        got = b.fetch(t)[0]
    finally:
        b.close()
    np.testing.assert_array_equal(got, off[1])
    assert gm.prefix_cache_info()["hit_positions"] - hp0 == 256


def test_debug_session_bypasses(gm):
    A = ins(300, 91)
    gm.prefix_cache(64)
    s = gm.session([req(A, 1)], OPTS, debug=True); s.prefill()
    assert s.prefix_info(0) == 0; s.close()
    assert gm.prefix_cache_info()["pages_cached"] == 0          # inserted nothing
    run(gm, [req(A, 1)])
    s = gm.session([req(A)], OPTS, debug=True); s.prefill()
    assert s.prefix_info(0) == 0; s.close()                     # and reuses nothing


def test_full_size_4k_prompt():
    """1.7B, the benchmark's 4105-position prompt: 4096 cached positions, a 9-position decode-step tail"""
    m = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    try:
        A = ins(4096, 77)
        m.prefix_cache(64)
        miss = run(m, [req(A)])[0]
        assert miss[2] == 0 and m.prefix_cache_info()["pages_cached"] == 32
        m.prefix_cache(0); m.prefix_cache(64)
        run(m, [req(A, 1)])
        hit = run(m, [req(A)])[0]
        assert hit[2] == 4096
        same(hit, miss)
        m.prefix_cache(0)
        assert m.kv_pool_info()["pages_in_use"] == 0
    finally:
        m.close()
