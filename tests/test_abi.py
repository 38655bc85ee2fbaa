"""C-ABI surface (no GPU needed): the library loads, exports every symbol include/q3tts.h declares,
host-only helpers work, and compute entry points fail loudly (never silently fall back) without a GPU."""
import ctypes
import os
import re

import numpy as np

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(q3_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    names = _header_functions()
    assert len(names) >= 35
    for n in names:
        assert hasattr(_lib.lib, n), f"libq3tts.so does not export {n}"
        assert n in _lib.SYMBOLS, f"python binding missing for {n}"
    assert _lib.lib.q3_abi_version() == 1


def test_struct_layouts_match_header_sizes():
    assert ctypes.sizeof(q.config.CConfig) == 36 * 4
    assert ctypes.sizeof(_lib.COptions) == 3 * 8 + 8 + 6 * 4
    assert ctypes.sizeof(_lib.CTiming) == 32


def test_manifest_only_handle_lists_reference_tensor_names():
    cfg = q.qwen3_tts_1_7b()
    h = ctypes.c_void_p(); c = cfg.to_c()
    _lib.check(_lib.lib.q3_model_create(ctypes.byref(c), -1, ctypes.byref(h)))
    items = {n: (cnt, dt) for n, cnt, dt in synth.manifest(h)}
    assert items["talker.model.layers.27.self_attn.q_proj.weight"] == (2048 * 2048, 1)
    assert items["talker.code_predictor.small_to_mtp_projection.weight"] == (1024 * 2048, 1)
    assert items["talker.code_predictor.lm_head.14.weight"] == (2048 * 1024, 1)
    assert items["decoder.decoder.1.block.1.conv.weight"] == (1536 * 768 * 16, 0)
    assert items["decoder.decoder.6.conv.weight"] == (96 * 7, 0)
    lm = sum(cnt for n, (cnt, dt) in items.items() if n.startswith("talker."))
    assert abs(lm / 1e9 - 1.92) < 0.03          # ≈1.92 B parameters (README.md:115-121 of the reference)
    # a manifest-only handle holds no weights and says so
    a = np.zeros(2048, dtype=np.float32)
    st = _lib.lib.q3_model_set_tensor(h, b"talker.model.norm.weight", 0, a.ctypes.data_as(ctypes.c_void_p), 2048)
    assert st == 7 and b"manifest-only" in _lib.lib.q3_last_error()
    _lib.lib.q3_model_free(h)
    cfg6 = q.qwen3_tts_0_6b()
    h = ctypes.c_void_p(); c = cfg6.to_c()
    _lib.check(_lib.lib.q3_model_create(ctypes.byref(c), -1, ctypes.byref(h)))
    names = [n for n, _, _ in synth.manifest(h)]
    assert "talker.code_predictor.small_to_mtp_projection.weight" not in names     # 0.6B has no projection
    _lib.lib.q3_model_free(h)


def test_unsupported_configs_are_rejected():
    cfg = q.tiny(); cfg.head_dim = 64
    h = ctypes.c_void_p(); c = cfg.to_c()
    assert _lib.lib.q3_model_create(ctypes.byref(c), -1, ctypes.byref(h)) == 7
    assert b"head_dim" in _lib.lib.q3_last_error()


def test_synth_fill_is_deterministic_and_normalish():
    a = synth._fill(5, "some.tensor", 0, 1.0, 0.0, 200000)
    b = synth._fill(5, "some.tensor", 0, 1.0, 0.0, 200000)
    c = synth._fill(5, "other.tensor", 0, 1.0, 0.0, 200000)
    assert (a == b).all() and not (a == c).all()
    assert abs(a.mean()) < 0.01 and abs(a.std() - 1.0) < 0.01
    h = synth._fill(5, "some.tensor", 1, 1.0, 0.0, 1000)
    assert (h == synth.f32_to_bf16(a[:1000])).all()       # bf16 output = RNE of the f32 stream


def test_rng_matches_reference_formula():
    st = ctypes.c_uint64(); _lib.lib.q3_rng_seed(42, ctypes.byref(st))
    assert st.value == (42 * 2685821657736338717 + 1442695040888963407) & ((1 << 64) - 1)
    v = [_lib.lib.q3_rng_next(ctypes.byref(st)) for _ in range(4)]
    assert all(0.0 <= x <= 1.0 for x in v) and len(set(v)) == 4


def test_codes_to_tensor_layout():
    frames = np.arange(32, dtype=np.uint32).reshape(2, 16)
    t = q.codes_to_tensor(frames)
    assert t.shape == (1, 16, 2) and t.dtype == np.int64
    assert (t[0, :, 0] == np.arange(16)).all() and (t[0, :, 1] == np.arange(16, 32)).all()


def test_no_cpu_fallback():
    """Without a GPU the product must fail loudly, not route to a CPU path."""
    if _lib.lib.q3_device_count() > 0:
        return
    cfg = q.tiny()
    try:
        q.Qwen3TTS(cfg, device=0)
    except _lib.Q3Error as e:
        assert e.status == 5 or e.status == 1
    else:
        raise AssertionError("model creation succeeded without a GPU")
    try:
        q.linear(np.zeros((1, 8), np.float32), np.zeros((8, 8), np.uint16))
    except _lib.Q3Error as e:
        assert e.status == 5
    else:
        raise AssertionError("q3_linear succeeded without a GPU")
    try:
        q.linear_ex(np.zeros((1, 8), np.float32), np.zeros((8, 8), np.uint16))
    except _lib.Q3Error as e:
        assert e.status == 5
    else:
        raise AssertionError("q3_linear_ex succeeded without a GPU")
    try:
        q.attn_step(0, np.zeros((1, 4 * 128), np.float32), [0], np.ones(128, np.float32), np.ones(128, np.float32), 1e-6,
                    np.ones((4, 64), np.float32), np.zeros((4, 64), np.float32), np.zeros((1, 1, 4, 128), np.float32),
                    np.zeros((1, 1, 4, 128), np.float32), 2, 1, 1)
    except _lib.Q3Error as e:
        assert e.status == 5
    else:
        raise AssertionError("q3_attn_step succeeded without a GPU")
    for call, name in ((lambda: q.attn_step_ex(0, [0], np.ones(128, np.float32), np.ones(128, np.float32), 1e-6, np.ones((4, 64), np.float32),
                                               np.zeros((4, 64), np.float32), np.zeros((1, 1, 4, 128), np.float32), np.zeros((1, 1, 4, 128), np.float32), 2, 1,
                                               qkv=np.zeros((1, 4 * 128), np.float32)), "q3_attn_step_ex"),
                       (lambda: q.kv_pages_to_bf16_ex(np.zeros((1, 1, 2, 1, 128, 128), np.float32), [0], [1]), "q3_kv_pages_to_bf16_ex"),
                       (lambda: q.conv_ex(0, np.zeros((16, 8), np.float32), np.zeros((32, 16, 1), np.float32)), "q3_conv_ex"),
                       (lambda: q.gemm_ex(np.zeros((1, 64), np.float32), np.zeros((64, 64), np.uint16)), "q3_gemm_ex"),
                       (lambda: q.attn_prefill_ex(np.zeros((2, 4 * 128), np.float32), 1, 0, np.ones(128, np.float32), np.ones(128, np.float32), 1e-6,
                                                  np.ones((4, 64), np.float32), np.zeros((4, 64), np.float32), np.zeros((1, 1, 4, 128), np.float32),
                                                  np.zeros((1, 1, 4, 128), np.float32), 2, 1), "q3_attn_prefill_ex"),
                       (lambda: q.attn_prefill_ex(np.zeros((2, 4 * 128), np.float32), 1, 0, np.ones(128, np.float32), np.ones(128, np.float32), 1e-6,
                                                  np.ones((4, 64), np.float32), np.zeros((4, 64), np.float32), np.zeros((1, 1, 4, 128), np.float32),
                                                  np.zeros((1, 1, 4, 128), np.float32), 2, 1, layout=1, page_slots=[[5]]), "q3_attn_prefill_ex (paged)"),
                       (lambda: q.prompt_rows_ex(q.api.ROWS_COPY, src=np.zeros((2, 8), np.float32), out=np.zeros(64 + 16 + 64, np.float32), cols=8),
                        "q3_prompt_rows_ex"),
                       (lambda: q.attn_c_ex(0, np.zeros((128, 8), np.float32), np.zeros((128, 8), np.float32), nh=2, k=np.zeros((128, 8), np.float32),
                                            v=np.zeros((128, 8), np.float32)), "q3_attn_c_ex"),
                       (lambda: q.attn_c_ex(1, np.zeros((128, 8), np.float32), np.zeros((128, 8), np.float32), nh=2, rows=[(0, 4, 0)],
                                            caches=np.zeros((1, 1, 2, 128, 32), np.float32)), "q3_attn_c_ex (stream)"),
                       (lambda: q.attn_c_ex(2, np.zeros((128, 8), np.float32), np.zeros((128, 8), np.float32), nh=2, rows=[(0, 4, 0)],
                                            caches=np.zeros((1, 1, 2, 128, 32), np.float32), tabs=[0], tab0=[0], tab_n=[1]), "q3_attn_c_ex (blocked)"),
                       (lambda: q.rope_c_ex(np.zeros((128, 4), np.float32), np.zeros((128, 4), np.float32), np.ones((4, 32), np.float32),
                                            np.zeros((4, 32), np.float32), 2), "q3_rope_c_ex"),
                       (lambda: q.copy_cols_ex(np.zeros(16, np.float32), np.zeros(16, np.float32), 4, [0], [0], [4], [4]), "q3_copy_cols_ex"),
                       (lambda: q.copy_segs_ex(np.zeros(16, np.float32), np.zeros(16, np.float32), [(0, 0, 8)]), "q3_copy_segs_ex"),
                       (lambda: q.gather_frames_ex(np.zeros(32, np.uint32), [3], np.zeros(16, np.uint32)), "q3_gather_frames_ex"),
                       (lambda: q.rvq_embed_ex(np.zeros((2, 16), np.uint32), np.zeros((4, 8), np.float32), np.zeros((15, 4, 8), np.float32),
                                               np.zeros(16, np.float32), np.zeros(16, np.float32)), "q3_rvq_embed_ex"),
                       (lambda: q.silu_mul_ex(np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32)), "q3_silu_mul_ex"),
                       (lambda: q.spk_op_ex(q.api.SPK_PAD, np.zeros((2, 5), np.float32), np.zeros(18, np.float32), C=2, T=5, pl=2, Tp=9), "q3_spk_op_ex (pad)"),
                       (lambda: q.spk_op_ex(q.api.SPK_COLS, np.zeros((2, 9), np.float32), np.zeros(10, np.float32), C=2, T=5, ld=9, off=4), "q3_spk_op_ex (cols)"),
                       (lambda: q.spk_op_ex(q.api.SPK_MEAN, np.zeros((2, 5), np.float32), np.zeros(2, np.float32), C=2, T=5), "q3_spk_op_ex (mean)"),
                       (lambda: q.spk_op_ex(q.api.SPK_SE_APPLY, np.zeros((2, 5), np.float32), np.zeros(10, np.float32), C=2, T=5, b=np.zeros(2, np.float32)),
                        "q3_spk_op_ex (se_apply)"),
                       (lambda: q.spk_op_ex(q.api.SPK_ASP_IN, np.zeros((2, 5), np.float32), np.zeros(30, np.float32), C=2, T=5), "q3_spk_op_ex (asp_in)"),
                       (lambda: q.spk_op_ex(q.api.SPK_ASP_POOL, np.zeros((2, 5), np.float32), np.zeros(4, np.float32), C=2, T=5, b=np.zeros((2, 5), np.float32)),
                        "q3_spk_op_ex (asp_pool)"),
                       (lambda: q.mimi_op_ex(q.api.MIMI_ELU, np.zeros(8, np.float32), np.zeros(8, np.float32), L=8), "q3_mimi_op_ex (elu)"),
                       (lambda: q.mimi_op_ex(q.api.MIMI_FOLD, np.zeros((2, 7), np.float32), np.zeros(16, np.float32), L=7, C=2, r=2, Lf=4), "q3_mimi_op_ex (fold)"),
                       (lambda: q.mimi_op_ex(q.api.MIMI_CODEBOOK, np.zeros((3, 8), np.float32), np.zeros(24, np.float32), L=8, C=3, b=np.ones(3, np.float32)),
                        "q3_mimi_op_ex (codebook)"),
                       (lambda: q.mimi_rvq_ex(np.zeros((8, 3), np.float32), np.zeros((2, 4, 8), np.float32), np.zeros((3, 4), np.uint32)), "q3_mimi_rvq_ex"),
                       (lambda: q.sample_ex(np.zeros((2, 8), np.float32), np.zeros(2, np.float32), 8, np.zeros(2, np.uint32), q.sample_row(q.SynthesisOptions())),
                        "q3_sample_ex"),
                       (lambda: q.frame_embed_ex(np.zeros((4, 8), np.uint16), np.zeros((15, 5, 8), np.uint16), [0], np.zeros((1, 5), np.float32),
                                                 np.zeros(16, np.uint32), [0], 1, np.zeros((2, 8), np.float32), [0], [1], [1], np.zeros(8, np.float32)),
                        "q3_frame_embed_ex"),
                       (lambda: q.cp_gather_ex(0, np.zeros(8, np.float32), 8, 1, 8, last_hidden=np.zeros((1, 8), np.float32)), "q3_cp_gather_ex"),
                       (lambda: q.rmsnorm_ex(np.zeros(8, np.float32), np.ones(8, np.float32), np.zeros(8, np.float32), 1, 8), "q3_rmsnorm_ex"),
                       (lambda: q.norm_c(np.zeros((16, 8), np.float32), np.ones(16, np.float32)), "q3_norm_c"),
                       (lambda: q.dwconv7(np.zeros((16, 8), np.float32), np.zeros((16, 7), np.float32), np.zeros(16, np.float32)), "q3_dwconv7")):
        try:
            call()
        except _lib.Q3Error as e:
            assert e.status == 5, name
        else:
            raise AssertionError(f"{name} succeeded without a GPU")


def test_conv_path_is_host_only():
    """kernel selection of the conv family answers without a GPU: a code, its text, and 0 for what the launchers refuse"""
    code = q.conv_path(96, 96, 4096, 7, 9)
    assert code == 5 and q.conv_path_name(code).startswith("k_conv_bf16x3<96co x 128t, 3 waves")
    assert q.conv_path(1, 96, 1920, 7) == 2 and q.conv_path(1, 96, 1920, 7, aligned16=False) == 1
    assert q.conv_path(64, 16, 100, 9) == 0 and q.conv_path_name(0) == "none" and q.conv_path_name(-1) == "invalid"
    assert q.resunit_path(96, 4096, 3) == 15 and q.resunit_path(96, 4096, 3, planes=2) == 15 + 256 and q.resunit_path(96, 4095, 3) == 0
    assert ctypes.sizeof(_lib.CConvEx) == 16 * 4 + 16 * 8


def test_prefill_paths_are_host_only():
    """kernel selection of the prefill GEMM and attention answers without a GPU; None for what the launchers refuse"""
    assert q.gemm_path(4105, 2048, 2048) == (3, 8, 1, 1) and q.gemm_path(509, 2048, 6144) == (3, 8, 8, 1)
    assert q.gemm_path(130, 384, 128) == (2, 1, 1, 1) and q.gemm_path(130, 64, 40) == (1, 1, 1, 1) and q.gemm_path(130, 64, 36, planes=False) == (0, 1, 1, 1)
    assert q.gemm_path(130, 96, 128) is None and q.gemm_path(0, 64, 128) is None
    # sizes whose tile roundings would leave int are refused at the entry (they used to overflow inside the decision functions)
    L = _lib.lib
    assert L.q3_gemm_path(1 << 24, 64, 128, 0, 0, 0, 1, None) >= 0 and L.q3_gemm_path(130, 64, (1 << 24) + 4, 0, 0, 0, 1, None) == -1
    assert L.q3_gemm_path(130, 64, 2147483644, 0, 0, 0, 1, None) == -1 and L.q3_gemm_path(2147483647, 64, 128, 0, 0, 0, 1, None) == -1
    assert L.q3_conv_path(64, 64, 1 << 30, 7, 1, 1, 1, 0, 3, 1) != 0 and L.q3_conv_path(64, 64, (1 << 30) + 1, 7, 1, 1, 1, 0, 3, 1) == 0
    assert L.q3_conv_path(64, 64, 2147483647, 7, 1, 1, 1, 0, 3, 1) == 0 and L.q3_conv_path(64, 64, 640, 7, -2147483648, 1, 1, 0, 3, 1) == 0
    assert L.q3_resunit_path(96, 1 << 30, 9, 1, 0, 3) != 0 and L.q3_resunit_path(96, 2147483647, 9, 1, 0, 3) == 0
    assert q.attn_prefill_path(16, 8, True, 2) == (3, 2) and q.attn_prefill_path(16, 8, False) == (2, 1) and q.attn_prefill_path(16, 2, False) is None
    assert ctypes.sizeof(_lib.CGemmEx) == 14 * 4 + 8 * 8 and ctypes.sizeof(_lib.CAttnPrefillEx) == 16 * 4 + 12 * 8 and \
        ctypes.sizeof(_lib.CPromptRowsEx) == 10 * 4 + 14 * 8


def test_codec_attn_entries_are_host_checked():
    """kernel selection of launch_attn_c answers without a GPU, and q3_attn_c_ex refuses a bad shape with Q3_INVALID_ARG before it
    touches a device (the full list: tests/test_codec_attn_reference.py)"""
    assert q.attn_c_path() == 1 and q.attn_c_path(0) == 0 and q.attn_c_path(2) is None and q.attn_c_path(1, hd=128) is None
    assert ctypes.sizeof(_lib.CAttnCEx) == 14 * 4 + 9 * 8
    z = lambda *s: np.zeros(s, np.float32)
    bad = [lambda: q.attn_c_ex(0, z(64, 8), z(64, 8), nh=2, hd=32, k=z(64, 8), v=z(64, 8)),                                    # hd != 64
           lambda: q.attn_c_ex(1, z(128, 8), z(128, 8), nh=2, rows=[(5, 5, 0)], caches=z(1, 1, 2, 128, 64)),                   # e <= a0
           lambda: q.attn_c_ex(1, z(128, 8), z(128, 8), nh=2, rows=[(60, 65, 0)], caches=z(1, 1, 2, 128, 64)),                 # e > cap
           lambda: q.attn_c_ex(2, z(128, 8), z(128, 8), nh=2, rows=[(0, 4, 0)], caches=z(2, 1, 2, 128, 48), tabs=[0], tab0=[0], tab_n=[1]),      # bf % 32
           lambda: q.attn_c_ex(2, z(128, 8), z(128, 8), nh=2, rows=[(30, 34, 0)], caches=z(2, 1, 2, 128, 32), tabs=[0], tab0=[0], tab_n=[1])]    # short block list
    for k, call in enumerate(bad):
        try:
            call()
        except _lib.Q3Error as e:
            assert e.status == 1, k
        else:
            raise AssertionError(f"bad shape {k} accepted")


def test_sampler_and_seam_entries_are_host_checked():
    """struct sizes of the sampler / frame-seam test entries, and q3_sample_row answering without a GPU (the refusals of each entry:
    tests/test_sampler_reference.py, tests/test_frame_seam_reference.py)"""
    assert ctypes.sizeof(_lib.CSampleRow) == 12 * 4
    assert ctypes.sizeof(_lib.CSampleEx) == 12 * 4 + 12 * 4 + 12 * 8
    assert ctypes.sizeof(_lib.CFrameEmbedEx) == 8 * 4 + 12 * 8
    assert ctypes.sizeof(_lib.CCpGatherEx) == 12 * 4 + 11 * 8
    r = q.sample_row(q.SynthesisOptions())
    assert (r.apply_temp, r.greedy, r.top_k, r.use_top_p, r.use_rep, r.eos_id, r.min_new_tokens, r.pad) == (1, 0, 50, 1, 1, 2150, 2, 0)
    assert r.inv_temp == np.float32(1.0 / 0.9) and r.top_p == np.float32(0.9) and r.rep_inv == np.float32(1.0) / np.float32(1.05)


def test_speaker_language_tables():
    assert q.Speaker.from_str("ryan").token_id() == 3061 and q.Speaker.from_str("uncle_fu") is q.Speaker.UncleFu
    assert q.Language.from_str("en").token_id() == 2050 and q.Language.from_str("Chinese").token_id() == 2055
    assert q.Speaker.Sohee.native_language() is q.Language.Korean
    o = q.SynthesisOptions()
    assert (o.max_length, o.temperature, o.top_k, o.top_p, o.repetition_penalty, o.eos_token_id, o.chunk_frames, o.min_new_tokens) == \
        (2048, 0.9, 50, 0.9, 1.05, 2150, 10, 2)
    assert q.CODEC_EOS_TOKEN_ID == 2150 and q.SAMPLES_PER_FRAME == 1920


def test_integration_doc_covers_every_symbol():
    """INTEGRATION.md maps every exported symbol to the reference interface it replaces (or marks it new)."""
    import re
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = sorted(set(re.findall(r"\b(q3_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 70
    assert [n for n in names if n not in doc] == []


def test_null_handles_return_status_not_crash():
    """"Never abort / unwind across the ABI" (Errors): every entry point checks its handles before it
    touches the GPU, so misuse from a host without a device still comes back as a status + message."""
    import ctypes
    from qwen3_tts_rs_amd import _lib
    L = _lib.lib
    null = ctypes.c_void_p(None)
    i = ctypes.c_int(); sz = ctypes.c_size_t(); d = ctypes.c_double(); t64 = ctypes.c_int64()
    calls = [
        lambda: L.q3_model_create(None, 0, ctypes.byref(null)),
        lambda: L.q3_model_set_tensor(None, b"x", 0, None, 0),
        lambda: L.q3_model_finalize(None),
        lambda: L.q3_model_arena(None, None, None),
        lambda: L.q3_session_create(None, None, 1, ctypes.byref(null)),
        lambda: L.q3_session_prefill(None),
        lambda: L.q3_session_generate(None, 1, 1),
        lambda: L.q3_session_frames(None, 0, ctypes.byref(i), ctypes.byref(i)),
        lambda: L.q3_session_codes(None, 0, None, 0, ctypes.byref(i)),
        lambda: L.q3_session_decode(None, 0, 0, 0, None, 0, ctypes.byref(sz)),
        lambda: L.q3_session_run(None, 1, None, None, None, None),
        lambda: L.q3_session_next_chunk(None, None, 0, ctypes.byref(sz), ctypes.byref(i)),
        lambda: L.q3_session_set_stream_mode(None, 1),
        lambda: L.q3_session_set_kv_dtype(None, 1),
        lambda: L.q3_model_set_codec_planes(None, 2),
        lambda: L.q3_session_create_reserved(None, None, 1, 8, 16, ctypes.byref(null)),
        lambda: L.q3_session_replace(None, 0, None),
        lambda: L.q3_session_next_chunk_row(None, 0, None, 0, ctypes.byref(sz), ctypes.byref(i)),
        lambda: L.q3_batcher_create(None, 8, 64, 0, ctypes.byref(null)),
        lambda: L.q3_batcher_submit(None, None, 0, ctypes.byref(t64)),
        lambda: L.q3_batcher_step(None, 8, 1, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)),
        lambda: L.q3_batcher_poll(None, 1, ctypes.byref(i), ctypes.byref(i), ctypes.byref(sz)),
        lambda: L.q3_batcher_fetch(None, 1, None, 0, None, 0),
        lambda: L.q3_decode_codes(None, None, 0, None, None),
        lambda: L.q3_spk_create(None, 0, ctypes.byref(null)),
        lambda: L.q3_spk_finalize(None),
        lambda: L.q3_spk_encode(None, None, 0, 24000, None),
        lambda: L.q3_spk_load_safetensors(None, b"/nonexistent"),
        lambda: L.q3_dp_init(0, 1, None, 0, ctypes.byref(null)),
        lambda: L.q3_dp_broadcast_weights(None, None, 0),
        lambda: L.q3_config_from_json(b"/nonexistent/config.json", None, None),
        lambda: L.q3_model_load(b"/nonexistent", -1, ctypes.byref(null), ctypes.byref(i)),
        lambda: L.q3_wav_read(b"/nonexistent.wav", None, 0, None, None),
        lambda: L.q3_resample(None, 1, 16000, 24000, None, 0, None),
        lambda: L.q3_linear_ex(0, None),
        lambda: L.q3_linear_ex(0, ctypes.byref(_lib.CLinearEx())),
        lambda: L.q3_attn_step(0, None),
        lambda: L.q3_attn_step(0, ctypes.byref(_lib.CAttnStep())),
        lambda: L.q3_attn_step_ex(0, None),
        lambda: L.q3_attn_step_ex(0, ctypes.byref(_lib.CAttnStepEx())),
        lambda: L.q3_kv_pages_to_bf16_ex(0, 1, 1, 1, None, None, None, None, None, None),
        lambda: L.q3_conv_ex(0, None),
        lambda: L.q3_conv_ex(0, ctypes.byref(_lib.CConvEx())),
        lambda: L.q3_gemm_ex(0, None),
        lambda: L.q3_gemm_ex(0, ctypes.byref(_lib.CGemmEx())),
        lambda: L.q3_attn_prefill_ex(0, None),
        lambda: L.q3_attn_prefill_ex(0, ctypes.byref(_lib.CAttnPrefillEx())),
        lambda: L.q3_prompt_rows_ex(0, None),
        lambda: L.q3_prompt_rows_ex(0, ctypes.byref(_lib.CPromptRowsEx())),
        lambda: L.q3_attn_c_ex(0, None),
        lambda: L.q3_attn_c_ex(0, ctypes.byref(_lib.CAttnCEx())),
        lambda: L.q3_rope_c_ex(0, None, None, None, None, None, 2, 64, 8, 8),
        lambda: L.q3_copy_cols_ex(0, None, 16, None, 16, 1, 1, None, None, None, None, 0, 0),
        lambda: L.q3_copy_segs_ex(0, None, 16, None, 16, 1, None),
        lambda: L.q3_gather_frames_ex(0, None, 16, None, 1, None, 16),
        lambda: L.q3_rvq_embed_ex(0, None, 1, None, None, 8, 16, None, None, 0, 8),
        lambda: L.q3_silu_mul_ex(0, None, None, None, 8, 8),
        lambda: L.q3_spk_op_ex(0, None),
        lambda: L.q3_spk_op_ex(0, ctypes.byref(_lib.CSpkOpEx())),
        lambda: L.q3_mimi_op_ex(0, None),
        lambda: L.q3_mimi_op_ex(0, ctypes.byref(_lib.CMimiOpEx())),
        lambda: L.q3_mimi_rvq_ex(0, None, 1, None, 1, 4, 8, None, 1, 0),
        lambda: L.q3_spk_tables(None, None, None),
        lambda: L.q3_sample_row(None, None),
        lambda: L.q3_prompt_shape(None, 0, None, None, None, 0),
        lambda: L.q3_sample_ex(0, None),
        lambda: L.q3_sample_ex(0, ctypes.byref(_lib.CSampleEx())),
        lambda: L.q3_frame_embed_ex(0, None),
        lambda: L.q3_frame_embed_ex(0, ctypes.byref(_lib.CFrameEmbedEx())),
        lambda: L.q3_cp_gather_ex(0, None),
        lambda: L.q3_cp_gather_ex(0, ctypes.byref(_lib.CCpGatherEx())),
        lambda: L.q3_rmsnorm_ex(0, None, 8, 0, 8, None, None, 8, 0, 8, 1, 8, 1e-6, None, None),
        lambda: L.q3_norm_c(0, 0, None, None, None, 16, 8, 1e-6, None, 0, 128),
        lambda: L.q3_dwconv7(0, None, None, None, 16, 8, None, 0, 128),
    ]
    for k, f in enumerate(calls):
        st = f()
        assert st != 0, k
        assert len(L.q3_last_error()) > 0, k
    L.q3_model_free(None); L.q3_session_free(None); L.q3_spk_free(None); L.q3_dp_free(None); L.q3_batcher_free(None)     # free(NULL) is a no-op
