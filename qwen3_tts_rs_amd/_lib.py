"""ctypes binding of libq3tts.so (include/q3tts.h). The product has NO CPU fallback: if the HIP
library is missing this module raises, and every compute entry point fails loudly without a GPU."""
import ctypes
import os

from .config import CConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("Q3TTS_LIB") or os.path.join(_HERE, "libq3tts.so")   # env override: kernel-ablation builds (dev aid)

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: the gfx950 HIP library is not built. Run "
        "`python -c 'import __graft_entry__ as g; g.build()'` (or qwen3_tts_rs_amd/csrc/build.sh).")

lib = ctypes.CDLL(LIB_PATH)


class COptions(ctypes.Structure):
    _fields_ = [
        ("temperature", ctypes.c_double), ("top_p", ctypes.c_double), ("repetition_penalty", ctypes.c_double),
        ("seed", ctypes.c_uint64), ("max_length", ctypes.c_int32), ("top_k", ctypes.c_int32),
        ("eos_token_id", ctypes.c_int32), ("chunk_frames", ctypes.c_int32), ("min_new_tokens", ctypes.c_int32),
        ("has_seed", ctypes.c_int32),
    ]


class CRequest(ctypes.Structure):
    _fields_ = [
        ("mode", ctypes.c_int32),
        ("text_ids", ctypes.POINTER(ctypes.c_uint32)), ("n_text", ctypes.c_int32),
        ("instruct_ids", ctypes.POINTER(ctypes.c_uint32)), ("n_instruct", ctypes.c_int32),
        ("speaker_id", ctypes.c_uint32), ("language_id", ctypes.c_uint32),
        ("xvector", ctypes.POINTER(ctypes.c_float)),
        ("opts", COptions),
        ("ref_codes", ctypes.POINTER(ctypes.c_uint32)), ("n_ref", ctypes.c_int32),
        ("ref_text_ids", ctypes.POINTER(ctypes.c_uint32)), ("n_ref_text", ctypes.c_int32),
    ]


class CSpkConfig(ctypes.Structure):      # q3_spk_config (SpeakerEncoderConfig, config.rs:100-174)
    _fields_ = [("mel_dim", ctypes.c_int32), ("enc_dim", ctypes.c_int32), ("channels", ctypes.c_int32 * 5),
                ("kernel_sizes", ctypes.c_int32 * 5), ("dilations", ctypes.c_int32 * 5), ("attention_channels", ctypes.c_int32),
                ("res2net_scale", ctypes.c_int32), ("se_channels", ctypes.c_int32), ("sample_rate", ctypes.c_int32)]


class CMimiConfig(ctypes.Structure):     # q3_mimi_config (mimi::Config::v0_1(Some(16)), encoder_12hz.rs:73)
    _fields_ = [("n_filters", ctypes.c_int32), ("hidden", ctypes.c_int32), ("ratios", ctypes.c_int32 * 4), ("kernel", ctypes.c_int32),
                ("res_kernel", ctypes.c_int32), ("last_kernel", ctypes.c_int32), ("compress", ctypes.c_int32), ("n_layers", ctypes.c_int32),
                ("n_heads", ctypes.c_int32), ("head_dim", ctypes.c_int32), ("inter", ctypes.c_int32), ("window", ctypes.c_int32),
                ("cb_size", ctypes.c_int32), ("cb_dim", ctypes.c_int32), ("n_q", ctypes.c_int32), ("n_sem", ctypes.c_int32),
                ("norm_eps", ctypes.c_float), ("rope_theta", ctypes.c_float)]


class CLinearEx(ctypes.Structure):       # q3_linear_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("M", "N", "K", "ldx", "ldy", "ldr", "M_alloc", "epi", "tiled", "ksplit", "use_ws",
                                              "zero_n", "zero_guard")] + [("eps", ctypes.c_float)] + \
               [(n, ctypes.c_void_p) for n in ("x", "w", "w2", "bias", "norm_w", "resid", "y", "zero_buf")]


class CAttnStep(ctypes.Structure):       # q3_attn_step_args
    _fields_ = [(n, ctypes.c_int32) for n in ("variant", "B", "nh", "nkv", "n_splits", "max_seq")] + \
               [("eps", ctypes.c_float), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("pos", "qkv", "q_norm_w", "k_norm_w", "rope_cos", "rope_sin", "kcache", "vcache", "out")]


class CAttnStepEx(ctypes.Structure):     # q3_attn_step_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("variant", "layout", "B", "nh", "nkv", "n_splits", "max_seq", "rows_per_seq", "n_layers", "layer",
                                              "n_slabs", "kv_row_pages", "qkv_S", "qkv_K", "g_vocab", "g_proj_dim", "g_ldx", "g_max_frames",
                                              "g_code_slot", "zero_n", "zero_guard")] + \
               [("eps", ctypes.c_float), ("qkv_eps", ctypes.c_float), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("pos", "qkv", "q_norm_w", "k_norm_w", "rope_cos", "rope_sin", "kcache", "vcache", "out", "page_slots",
                                               "rot_used", "stray", "qkv_part", "qkv_ssq", "g_logits", "g_tok", "g_qkv_tab", "g_proj_tab", "g_x",
                                               "g_codes", "g_frame_idx", "zero_buf")]


class CConvEx(ctypes.Structure):         # q3_conv_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "cin", "cout", "L", "k", "dil", "stride", "act", "planes", "packed", "resid_in_place",
                                              "snake_raw", "y2_is_x", "y_front", "y_elems")] + [("path", ctypes.POINTER(ctypes.c_int32))] + \
               [(n, ctypes.c_void_p) for n in ("x", "w", "b", "snake_a", "snake_b", "resid", "scale", "post_a", "post_ib", "w2", "b2", "mid_a",
                                               "mid_ib", "y", "y2")]


class CGemmEx(ctypes.Structure):         # q3_gemm_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("M", "N", "K", "ldx", "ldy", "ldr", "M_alloc", "epi", "geometry", "k_split", "sup_m",
                                              "sup_n")] + [("eps", ctypes.c_float), ("path", ctypes.POINTER(ctypes.c_int32))] + \
               [(n, ctypes.c_void_p) for n in ("x", "w", "w2", "bias", "norm_w", "resid", "y")]


class CAttnPrefillEx(ctypes.Structure):  # q3_attn_prefill_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("n_seq", "rps", "base_pos", "nh", "nkv", "max_seq", "ld_qkv", "ld_out", "kernel", "halves",
                                              "use_planes")] + [("eps", ctypes.c_float), ("path", ctypes.POINTER(ctypes.c_int32))] + \
               [(n, ctypes.c_void_p) for n in ("qkv", "q_norm_w", "k_norm_w", "rope_cos", "rope_sin", "kcache", "vcache", "out")] + \
               [(n, ctypes.c_int32) for n in ("layout", "n_layers", "layer", "n_slabs")] + \
               [(n, ctypes.c_void_p) for n in ("page_slots", "rot_used", "stray")]


class CAttnPrefillPackedEx(ctypes.Structure):  # q3_attn_prefill_packed_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("n_seq", "nh", "nkv", "max_seq", "ld_qkv", "ld_out", "kernel")] + [("eps", ctypes.c_float)] + \
               [(n, ctypes.c_void_p) for n in ("seq_len", "path", "plane_tail", "qkv", "q_norm_w", "k_norm_w", "rope_cos", "rope_sin", "kcache", "vcache",
                                               "out")] + \
               [(n, ctypes.c_int32) for n in ("layout", "n_layers", "layer", "n_slabs")] + \
               [(n, ctypes.c_void_p) for n in ("page_slots", "rot_used", "stray")]


class CPromptRowsEx(ctypes.Structure):   # q3_prompt_rows_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("mode", "n", "cols", "n_table", "n_rows", "n_ref", "cp_vocab", "lds", "ldd", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("table", "ids", "src", "text_row", "codec_id", "xvec", "ref_codes", "cp_embs", "dst_row", "ent", "out",
                                               "trail_len", "text_ready", "limit")]


class CAttnCEx(ctypes.Structure):        # q3_attn_c_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("mode", "nh", "hd", "L", "kernel", "window", "N", "n_rows", "layers", "layer", "cap", "n_blocks",
                                              "n_tabs")] + [("scale", ctypes.c_float)] + \
               [(n, ctypes.c_void_p) for n in ("q", "k", "v", "rows", "caches", "tabs", "tab0", "tab_n", "o")]


class CSpkOpEx(ctypes.Structure):        # q3_spk_op_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("op", "C", "T", "pl", "Tp", "ld", "off", "reserved")] + \
               [(n, ctypes.c_longlong) for n in ("a_elems", "b_elems", "out_front", "out_elems")] + \
               [(n, ctypes.c_void_p) for n in ("a", "b", "out")]


class CMimiOpEx(ctypes.Structure):       # q3_mimi_op_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("op", "C", "L", "r", "Lf", "elu", "replicate", "reserved")] + \
               [(n, ctypes.c_longlong) for n in ("a_elems", "b_elems", "out_front", "out_elems")] + \
               [(n, ctypes.c_void_p) for n in ("a", "b", "out")]


class CSampleRow(ctypes.Structure):      # q3_sample_rec (the sampler's per-row record)
    _fields_ = [("inv_temp", ctypes.c_float), ("apply_temp", ctypes.c_int32), ("greedy", ctypes.c_int32), ("top_k", ctypes.c_int32),
                ("top_p", ctypes.c_float), ("use_top_p", ctypes.c_int32), ("rep_pen", ctypes.c_float), ("rep_inv", ctypes.c_float),
                ("use_rep", ctypes.c_int32), ("eos_id", ctypes.c_int32), ("min_new_tokens", ctypes.c_int32), ("pad", ctypes.c_int32)]


class CPromptShape(ctypes.Structure):    # q3_prompt_shape_rec (the prompt layout of a request)
    _fields_ = [(n, ctypes.c_int32) for n in ("icl", "n_ins", "n_ref_text", "n_icl", "overlay", "prefill_len", "n_rows", "trailing_len", "n_trail",
                                              "limit", "open_need", "prefix_pages", "r_role", "r_pad", "r_bos", "r_text", "r_eos", "trail_base")]


class CSampleEx(ctypes.Structure):       # q3_sample_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "vocab", "ld", "u_stride", "u_elems", "advance", "token_count_static", "hist_stride_b",
                                              "hist_cap", "codec_eos", "use_suppress", "guard")] + [("scalar", CSampleRow)] + \
               [(n, ctypes.c_void_p) for n in ("logits", "u", "draw_idx", "rows", "limit", "text_ready", "tok", "seen", "token_count",
                                               "frame_idx", "pos", "logits_hist")]


class CFrameEmbedEx(ctypes.Structure):   # q3_frame_embed_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "H", "n_sem", "cp_vocab", "max_frames", "n_text_rows", "guard", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("codec_emb", "cp_embs", "tok", "cp_logits_last", "frame_idx", "text_rows", "trail_base",
                                               "trail_len", "pad_row", "text_ready", "codes", "out")]


class CCpGatherEx(ctypes.Structure):     # q3_cp_gather_ex_args
    _fields_ = [(n, ctypes.c_int32) for n in ("pass_", "B", "H", "n_sem", "cp_vocab", "max_frames", "proj_dim", "qkv_dim", "ld_out",
                                              "ld_qkv_out", "guard", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("last_hidden", "codec_emb", "tok", "cp_emb", "cp_logits", "proj_tab", "qkv_tab", "frame_idx",
                                               "codes", "out", "qkv_out")]


class CClip(ctypes.Structure):           # q3_clip
    _fields_ = [("data", ctypes.c_void_p), ("frames", ctypes.c_int64), ("channels", ctypes.c_int32), ("sample_rate", ctypes.c_uint32),
                ("format", ctypes.c_int32)]


class CMimiPackClip(ctypes.Structure):   # q3_mimi_pack_clip
    _fields_ = [("frames", ctypes.c_int32), ("pass_", ctypes.c_int32), ("start", ctypes.c_int64)]


class CWavDesc(ctypes.Structure):        # q3_wav_desc
    _fields_ = [("format", ctypes.c_int32), ("channels", ctypes.c_int32), ("bits", ctypes.c_int32), ("sample_rate", ctypes.c_uint32),
                ("frames", ctypes.c_int64), ("data_offset", ctypes.c_int64), ("data_bytes", ctypes.c_int64)]


class CTiming(ctypes.Structure):
    _fields_ = [("prefill_ms", ctypes.c_double), ("generation_ms", ctypes.c_double), ("decode_ms", ctypes.c_double),
                ("generation_frames", ctypes.c_int32)]


c_void_p, c_int, c_char_p = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p
P = ctypes.POINTER

# every symbol include/q3tts.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "q3_abi_version": (c_int, []),
    "q3_last_error": (c_char_p, []),
    "q3_device_count": (c_int, []),
    "q3_model_create": (c_int, [P(CConfig), c_int, P(c_void_p)]),
    "q3_model_free": (None, [c_void_p]),
    "q3_model_set_tensor": (c_int, [c_void_p, c_char_p, c_int, c_void_p, ctypes.c_int64]),
    "q3_model_n_tensors": (c_int, [c_void_p]),
    "q3_model_tensor_info": (c_int, [c_void_p, c_int, P(c_char_p), P(ctypes.c_int64), P(c_int)]),
    "q3_model_arena": (c_int, [c_void_p, P(c_void_p), P(ctypes.c_size_t)]),
    "q3_model_kv_pool_limit": (c_int, [c_void_p, c_int]),
    "q3_model_set_codec_planes": (c_int, [c_void_p, c_int]),
    "q3_model_kv_pool_trim": (c_int, [c_void_p, P(ctypes.c_size_t)]),
    "q3_model_kv_pool_info": (c_int, [c_void_p, P(c_int), P(ctypes.c_size_t), P(c_int), P(c_int), P(c_int)]),
    "q3_model_prefix_cache": (c_int, [c_void_p, c_int]),
    "q3_model_prefix_cache_info": (c_int, [c_void_p, P(c_int), P(c_int), P(c_int), P(ctypes.c_longlong), P(ctypes.c_longlong), P(ctypes.c_longlong)]),
    "q3_session_prefix_info": (c_int, [c_void_p, c_int, P(c_int)]),
    "q3_model_mark_loaded": (c_int, [c_void_p]),
    "q3_model_finalize": (c_int, [c_void_p]),
    "q3_synth_fill": (c_int, [ctypes.c_uint64, c_char_p, c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int64, c_void_p]),
    "q3_session_create": (c_int, [c_void_p, P(CRequest), c_int, P(c_void_p)]),
    "q3_session_create_reserved": (c_int, [c_void_p, P(CRequest), c_int, c_int, c_int, P(c_void_p)]),
    "q3_session_free": (None, [c_void_p]),
    "q3_session_prefill": (c_int, [c_void_p]),
    "q3_session_generate": (c_int, [c_void_p, c_int, c_int]),
    "q3_session_frames": (c_int, [c_void_p, c_int, P(c_int), P(c_int)]),
    "q3_session_codes": (c_int, [c_void_p, c_int, c_void_p, c_int, P(c_int)]),
    "q3_session_decode": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, ctypes.c_size_t, P(ctypes.c_size_t)]),
    "q3_session_set_kv_dtype": (c_int, [c_void_p, c_int]),
    "q3_session_run": (c_int, [c_void_p, c_int, P(c_void_p), P(ctypes.c_size_t), P(ctypes.c_size_t), P(CTiming)]),
    "q3_session_next_chunk": (c_int, [c_void_p, c_void_p, ctypes.c_size_t, P(ctypes.c_size_t), P(c_int)]),
    "q3_session_next_chunk_row": (c_int, [c_void_p, c_int, c_void_p, ctypes.c_size_t, P(ctypes.c_size_t), P(c_int)]),
    "q3_session_next_chunks": (c_int, [c_void_p, P(c_void_p), P(ctypes.c_size_t), P(ctypes.c_size_t), P(c_int)]),
    "q3_codec_stream_create": (c_int, [c_void_p, c_int, c_int, P(c_void_p)]),
    "q3_codec_stream_create_blocked": (c_int, [c_void_p, c_int, c_int, c_int, c_int, P(c_void_p)]),
    "q3_codec_stream_info": (c_int, [c_void_p, P(c_int), P(ctypes.c_size_t), P(c_int), P(c_int), P(c_int)]),
    "q3_codec_stream_prime": (c_int, [c_void_p, c_int, c_void_p, c_int]),
    "q3_codec_stream_free": (None, [c_void_p]),
    "q3_codec_stream_reset": (c_int, [c_void_p, c_int]),
    "q3_codec_stream_pos": (c_int, [c_void_p, c_int, P(c_int)]),
    "q3_codec_stream_push": (c_int, [c_void_p, c_int, P(c_int), P(c_void_p), P(c_int), P(c_void_p), P(ctypes.c_size_t)]),
    "q3_pcm_stage_create": (c_int, [c_int, c_int, ctypes.c_size_t, P(c_void_p)]),
    "q3_pcm_stage_free": (None, [c_void_p]),
    "q3_pcm_stage_set": (c_int, [c_void_p, c_int, ctypes.c_uint32, c_int]),
    "q3_pcm_stage_reset": (c_int, [c_void_p, c_int]),
    "q3_pcm_stage_push": (c_int, [c_void_p, c_int, P(c_int), P(c_void_p), P(ctypes.c_size_t), P(c_int), P(c_void_p), P(ctypes.c_size_t),
                                  P(ctypes.c_size_t)]),
    "q3_pcm_stage_bound": (c_int, [ctypes.c_uint32, ctypes.c_size_t, P(ctypes.c_size_t)]),
    "q3_pcm_stage_taps": (c_int, [ctypes.c_uint32, c_void_p, ctypes.c_size_t, P(c_int), P(c_int)]),
    "q3_pcm_stage_set_tempo": (c_int, [c_void_p, c_int, c_int]),
    "q3_pcm_stage_tempo_count": (c_int, [c_int, ctypes.c_size_t, c_int, P(ctypes.c_size_t), P(ctypes.c_size_t)]),
    "q3_pcm_stage_bound_tempo": (c_int, [ctypes.c_uint32, c_int, ctypes.c_size_t, P(ctypes.c_size_t)]),
    "q3_pcm_stage_tempo_lags": (c_int, [c_void_p, c_int, P(ctypes.c_int64), c_void_p, ctypes.c_size_t, P(ctypes.c_size_t)]),
    "q3_session_set_tempo": (c_int, [c_void_p, c_int, c_int]),
    "q3_batcher_ticket_tempo": (c_int, [c_void_p, ctypes.c_int64, c_int]),
    "q3_pcm_stage_set_pitch": (c_int, [c_void_p, c_int, c_int]),
    "q3_pcm_stage_pitch_plan": (c_int, [c_int, c_int, P(c_int), P(ctypes.c_double)]),
    "q3_pcm_stage_pitch_tables": (c_int, [c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t, P(c_int), P(c_int)]),
    "q3_pcm_stage_pitch_count": (c_int, [c_int, c_int, ctypes.c_size_t, c_int, P(ctypes.c_size_t)]),
    "q3_pcm_stage_bound_pitch": (c_int, [ctypes.c_uint32, c_int, c_int, c_int, ctypes.c_size_t, P(ctypes.c_size_t)]),
    "q3_session_set_pitch": (c_int, [c_void_p, c_int, c_int]),
    "q3_batcher_ticket_pitch": (c_int, [c_void_p, ctypes.c_int64, c_int]),
    "q3_pcm_stage_set_silence": (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    "q3_pcm_stage_silence": (c_int, [c_void_p, c_int] + [P(ctypes.c_int64)] * 5),
    "q3_pcm_stage_silence_hold": (c_int, [c_int, c_int, P(ctypes.c_size_t)]),
    "q3_pcm_stage_bound_silence": (c_int, [ctypes.c_uint32, c_int, c_int, c_int, c_int, c_int, ctypes.c_size_t, P(ctypes.c_size_t)]),
    "q3_silence_trim": (c_int, [c_void_p, ctypes.c_size_t, c_int, c_int, c_int, c_void_p, ctypes.c_size_t, P(ctypes.c_size_t), P(ctypes.c_int64)]),
    "q3_session_set_silence": (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    "q3_session_silence": (c_int, [c_void_p, c_int] + [P(ctypes.c_int64)] * 5),
    "q3_batcher_ticket_silence": (c_int, [c_void_p, ctypes.c_int64, c_int, c_int, c_int]),
    "q3_batcher_ticket_silence_read": (c_int, [c_void_p, ctypes.c_int64] + [P(ctypes.c_int64)] * 5),
    "q3_pcm_stage_set_mark": (c_int, [c_void_p, c_int, ctypes.c_uint64, c_int]),
    "q3_mark_carrier": (c_int, [ctypes.c_uint64, c_void_p]),
    "q3_mark_embed": (c_int, [c_void_p, ctypes.c_size_t, ctypes.c_uint64, c_int, c_void_p]),
    "q3_mark_score_detect": (ctypes.c_double, []),
    "q3_mark_detect": (c_int, [c_void_p, ctypes.c_size_t, ctypes.c_uint64, P(ctypes.c_double), P(c_int)]),
    "q3_session_set_mark": (c_int, [c_void_p, c_int, ctypes.c_uint64, c_int]),
    "q3_batcher_ticket_mark": (c_int, [c_void_p, ctypes.c_int64, ctypes.c_uint64, c_int]),
    "q3_ref_audio_mark_score": (c_int, [c_void_p, ctypes.c_uint64, P(ctypes.c_double), P(c_int)]),
    "q3_pcm_stage_set_level": (c_int, [c_void_p, c_int, c_int, c_int]),
    "q3_pcm_stage_level_coeffs": (c_int, [c_int, c_int, P(ctypes.c_float), P(ctypes.c_float)]),
    "q3_pcm_stage_level_count": (c_int, [ctypes.c_size_t, c_int, P(ctypes.c_size_t)]),
    "q3_pcm_stage_bound_level": (c_int, [ctypes.c_uint32, c_int, ctypes.c_size_t, P(ctypes.c_size_t)]),
    "q3_session_set_level": (c_int, [c_void_p, c_int, c_int, c_int]),
    "q3_batcher_ticket_level": (c_int, [c_void_p, ctypes.c_int64, c_int, c_int]),
    "q3_loudness_kweight": (c_int, [ctypes.c_uint32, P(ctypes.c_double), P(ctypes.c_double)]),
    "q3_pcm_stage_loudness_consts": (c_int, [c_int, c_int, P(ctypes.c_float), P(ctypes.c_float), P(ctypes.c_float), P(ctypes.c_float), P(ctypes.c_float)]),
    "q3_pcm_stage_set_loudness": (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    "q3_pcm_stage_loudness": (c_int, [c_void_p, c_int, P(ctypes.c_float), P(ctypes.c_float), P(c_int), P(c_int)]),
    "q3_pcm_stage_loudness_blocks": (c_int, [c_void_p, c_int, c_void_p, ctypes.c_size_t, P(ctypes.c_size_t)]),
    "q3_session_set_loudness": (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    "q3_session_loudness": (c_int, [c_void_p, c_int, P(ctypes.c_float), P(ctypes.c_float), P(c_int), P(c_int)]),
    "q3_batcher_ticket_loudness": (c_int, [c_void_p, ctypes.c_int64, c_int, c_int, c_int]),
    "q3_batcher_ticket_loudness_read": (c_int, [c_void_p, ctypes.c_int64, P(ctypes.c_float), P(ctypes.c_float), P(c_int), P(c_int)]),
    "q3_codec_stream_push_out": (c_int, [c_void_p, c_int, P(c_int), P(c_void_p), P(c_int), c_void_p, P(c_int), P(c_int), P(c_void_p),
                                         P(ctypes.c_size_t), P(ctypes.c_size_t)]),
    "q3_session_set_output": (c_int, [c_void_p, ctypes.c_uint32, c_int]),
    "q3_session_next_chunks_out": (c_int, [c_void_p, P(c_void_p), P(ctypes.c_size_t), P(ctypes.c_size_t), P(c_int)]),
    "q3_batcher_ticket_output": (c_int, [c_void_p, ctypes.c_int64, ctypes.c_uint32, c_int]),
    "q3_batcher_read_out": (c_int, [c_void_p, ctypes.c_int64, c_void_p, ctypes.c_size_t, P(ctypes.c_size_t), P(c_int)]),
    "q3_session_replace": (c_int, [c_void_p, c_int, c_void_p]),
    "q3_session_park_row": (c_int, [c_void_p, c_int, P(c_void_p)]),
    "q3_session_resume_row": (c_int, [c_void_p, c_int, c_void_p]),
    "q3_parked_free": (None, [c_void_p]),
    "q3_parked_info": (c_int, [c_void_p, P(c_int), P(c_int), P(c_int), P(c_int), P(ctypes.c_size_t)]),
    "q3_row_move": (c_int, [c_int, c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t, c_int, P(ctypes.c_size_t), P(ctypes.c_size_t),
                            P(ctypes.c_size_t), P(c_int)]),
    "q3_batcher_create": (c_int, [c_void_p, c_int, c_int, c_int, P(c_void_p)]),
    "q3_batcher_free": (None, [c_void_p]),
    "q3_batcher_submit": (c_int, [c_void_p, c_void_p, c_int, P(ctypes.c_int64)]),
    "q3_batcher_submit_streamed": (c_int, [c_void_p, c_void_p, P(ctypes.c_int64)]),
    "q3_batcher_read": (c_int, [c_void_p, ctypes.c_int64, c_void_p, ctypes.c_size_t, P(ctypes.c_size_t), P(c_int)]),
    "q3_batcher_stream_info": (c_int, [c_void_p, P(c_int), P(ctypes.c_size_t), P(c_int), P(c_int), P(c_int)]),
    "q3_batcher_submit_open": (c_int, [c_void_p, c_void_p, c_int, P(ctypes.c_int64)]),
    "q3_batcher_append_text": (c_int, [c_void_p, ctypes.c_int64, c_void_p, c_int, c_int]),
    "q3_batcher_text_state": (c_int, [c_void_p, ctypes.c_int64, P(c_int), P(c_int), P(c_int), P(c_int)]),
    "q3_batcher_cancel": (c_int, [c_void_p, ctypes.c_int64]),
    "q3_batcher_set_parking": (c_int, [c_void_p, c_int, c_int, c_int]),
    "q3_batcher_park": (c_int, [c_void_p, ctypes.c_int64]),
    "q3_batcher_unpark": (c_int, [c_void_p, ctypes.c_int64]),
    "q3_batcher_park_info": (c_int, [c_void_p, P(c_int), P(c_int), P(ctypes.c_longlong), P(ctypes.c_longlong), P(ctypes.c_longlong), P(c_int)]),
    "q3_batcher_step": (c_int, [c_void_p, c_int, c_int, P(c_int), P(c_int), P(c_int)]),
    "q3_batcher_poll": (c_int, [c_void_p, ctypes.c_int64, P(c_int), P(c_int), P(ctypes.c_size_t)]),
    "q3_batcher_fetch": (c_int, [c_void_p, ctypes.c_int64, c_void_p, c_int, c_void_p, ctypes.c_size_t]),
    "q3_session_set_debug": (c_int, [c_void_p, c_int]),
    "q3_session_prefill_len": (c_int, [c_void_p, c_int, P(c_int), P(c_int)]),
    "q3_session_get": (c_int, [c_void_p, c_int, c_int, c_void_p, ctypes.c_size_t]),
    "q3_talker_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "q3_cp_generate": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "q3_frame_embed": (c_int, [c_void_p, ctypes.c_uint32, c_void_p, c_void_p, c_void_p]),
    "q3_sample": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, P(COptions), c_int, c_void_p]),
    "q3_rng_seed": (None, [ctypes.c_uint64, P(ctypes.c_uint64)]),
    "q3_rng_next": (ctypes.c_float, [P(ctypes.c_uint64)]),
    "q3_fused_residual_rmsnorm": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_void_p, c_void_p]),
    "q3_linear": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "q3_linear_ex": (c_int, [c_int, P(CLinearEx)]),
    "q3_attn_step": (c_int, [c_int, P(CAttnStep)]),
    "q3_attn_step_ex": (c_int, [c_int, P(CAttnStepEx)]),
    "q3_kv_pages_to_bf16_ex": (c_int, [c_int] * 4 + [c_void_p] * 6),
    "q3_conv_path": (c_int, [c_int] * 10),
    "q3_resunit_path": (c_int, [c_int] * 6),
    "q3_conv_path_name": (c_char_p, [c_int]),
    "q3_conv_ex": (c_int, [c_int, P(CConvEx)]),
    "q3_test_conv_resident": (c_int, [c_int, P(CConvEx), c_int, P(ctypes.c_int32)]),
    "q3_gemm_path": (c_int, [c_int] * 7 + [P(ctypes.c_int32)]),
    "q3_gemm_ex": (c_int, [c_int, P(CGemmEx)]),
    "q3_attn_prefill_path": (c_int, [c_int] * 4 + [P(ctypes.c_int32)]),
    "q3_attn_prefill_ex": (c_int, [c_int, P(CAttnPrefillEx)]),
    "q3_attn_prefill_packed_ex": (c_int, [c_int, P(CAttnPrefillPackedEx)]),
    "q3_prefill_pack_plan": (c_int, [P(ctypes.c_int32), P(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P(ctypes.c_int32),
                                     P(ctypes.c_int32), P(ctypes.c_int32)]),
    "q3_session_prefill_info": (c_int, [c_void_p, P(ctypes.c_int32)]),
    "q3_prompt_rows_ex": (c_int, [c_int, P(CPromptRowsEx)]),
    "q3_attn_c_path": (c_int, [c_int, c_int]),
    "q3_attn_c_ex": (c_int, [c_int, P(CAttnCEx)]),
    "q3_rope_c_ex": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int]),
    "q3_copy_cols_ex": (c_int, [c_int, c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                ctypes.c_size_t, ctypes.c_size_t]),
    "q3_copy_segs_ex": (c_int, [c_int, c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t, c_int, c_void_p]),
    "q3_gather_frames_ex": (c_int, [c_int, c_void_p, ctypes.c_size_t, c_void_p, c_int, c_void_p, ctypes.c_size_t]),
    "q3_rvq_embed_ex": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int]),
    "q3_silu_mul_ex": (c_int, [c_int, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, ctypes.c_longlong]),
    "q3_spk_op_ex": (c_int, [c_int, P(CSpkOpEx)]),
    "q3_mimi_op_ex": (c_int, [c_int, P(CMimiOpEx)]),
    "q3_mimi_rvq_ex": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int]),
    "q3_spk_tables": (c_int, [c_void_p, c_void_p, c_void_p]),
    "q3_sample_row": (c_int, [P(COptions), P(CSampleRow)]),
    "q3_prompt_shape": (c_int, [P(CRequest), c_int, P(CPromptShape), c_void_p, c_void_p, c_int]),
    "q3_sample_ex": (c_int, [c_int, P(CSampleEx)]),
    "q3_frame_embed_ex": (c_int, [c_int, P(CFrameEmbedEx)]),
    "q3_cp_gather_ex": (c_int, [c_int, P(CCpGatherEx)]),
    "q3_rmsnorm_ex": (c_int, [c_int, c_void_p, ctypes.c_longlong, ctypes.c_longlong, c_int, c_void_p, c_void_p, ctypes.c_longlong,
                              ctypes.c_longlong, c_int, c_int, c_int, ctypes.c_float, c_void_p, c_void_p]),
    "q3_norm_c": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_void_p, c_int, c_int]),
    "q3_dwconv7": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int]),
    "q3_decode_codes": (c_int, [c_void_p, c_void_p, c_int, c_void_p, P(c_void_p)]),
    "q3_codes_to_tensor": (None, [c_void_p, c_int, c_void_p]),
    "q3_session_set_profile": (c_int, [c_void_p, c_int]),
    "q3_session_profile_read": (c_int, [c_void_p, P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_long), c_int]),
    "q3_session_profile_shapes": (c_int, [c_void_p, P(c_int), c_int, P(c_int), c_int]),
    "q3_bench_linear": (c_int, [c_int] * 9 + [P(ctypes.c_double)]),
    "q3_session_stream": (c_int, [c_void_p, P(c_void_p)]),
    "q3_session_frame_bytes": (c_int, [c_void_p, c_int, P(ctypes.c_double), P(ctypes.c_double)]),
    "q3_session_submit_info": (c_int, [c_void_p, P(c_int), P(c_int)]),
    "q3_session_submit_fences": (c_int, [c_void_p, P(c_int), P(c_int)]),
    "q3_session_set_stream_mode": (c_int, [c_void_p, c_int]),
    "q3_session_open_text": (c_int, [c_void_p, c_int]),
    "q3_session_append_text": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int]),
    "q3_session_text_state": (c_int, [c_void_p, c_int, P(c_int), P(c_int), P(c_int), P(c_int), P(c_int)]),
    "q3_model_config": (c_int, [c_void_p, P(CConfig)]),
    "q3_config_default": (c_int, [c_int, P(CConfig)]),
    "q3_config_from_json": (c_int, [c_char_p, P(CConfig), P(c_int)]),
    "q3_model_load": (c_int, [c_char_p, c_int, P(c_void_p), P(c_int)]),
    "q3_model_load_safetensors": (c_int, [c_void_p, c_char_p, P(c_int)]),
    "q3_safetensors_info": (c_int, [c_char_p, c_char_p, P(c_int), P(ctypes.c_int64), c_int, P(c_int)]),
    "q3_pcm16_from_f32": (c_int, [c_void_p, ctypes.c_int64, c_void_p]),
    "q3_wav_write_pcm16": (c_int, [c_char_p, c_void_p, ctypes.c_int64, ctypes.c_uint32]),
    "q3_g711_from_pcm16": (c_int, [c_void_p, ctypes.c_int64, c_int, c_void_p]),
    "q3_wav_write_g711": (c_int, [c_char_p, c_void_p, ctypes.c_int64, ctypes.c_uint32, c_int]),
    "q3_wav_read": (c_int, [c_char_p, c_void_p, ctypes.c_int64, P(ctypes.c_int64), P(ctypes.c_uint32)]),
    "q3_codes_write_bin": (c_int, [c_char_p, c_void_p, c_int, c_int]),
    "q3_codes_read_bin": (c_int, [c_char_p, c_void_p, c_int, c_int, P(c_int)]),
    "q3_audio_write_bin": (c_int, [c_char_p, c_void_p, ctypes.c_int64]),
    "q3_audio_read_bin": (c_int, [c_char_p, c_void_p, ctypes.c_int64, P(ctypes.c_int64)]),
    "q3_resample": (c_int, [c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, c_void_p, ctypes.c_int64, P(ctypes.c_int64)]),
    "q3_dp_unique_id": (c_int, [c_void_p]),
    "q3_dp_init": (c_int, [c_int, c_int, c_void_p, c_int, P(c_void_p)]),
    "q3_dp_free": (None, [c_void_p]),
    "q3_dp_info": (c_int, [c_void_p, P(c_int), P(c_int)]),
    "q3_dp_broadcast_weights": (c_int, [c_void_p, c_void_p, c_int]),
    "q3_dp_allgather_f64": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "q3_spk_config_default": (c_int, [P(CSpkConfig)]),
    "q3_spk_config_from_json": (c_int, [c_char_p, P(CSpkConfig), P(c_int)]),
    "q3_spk_create": (c_int, [P(CSpkConfig), c_int, P(c_void_p)]),
    "q3_spk_free": (None, [c_void_p]),
    "q3_spk_get_config": (c_int, [c_void_p, P(CSpkConfig)]),
    "q3_spk_n_tensors": (c_int, [c_void_p]),
    "q3_spk_tensor_info": (c_int, [c_void_p, c_int, P(c_char_p), P(ctypes.c_int64)]),
    "q3_spk_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, c_int, ctypes.c_int64]),
    "q3_spk_finalize": (c_int, [c_void_p]),
    "q3_spk_load_safetensors": (c_int, [c_void_p, c_char_p]),
    "q3_spk_mel_frames": (c_int, [ctypes.c_int64]),
    "q3_spk_mel": (c_int, [c_void_p, c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, P(c_int)]),
    "q3_spk_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, P(c_void_p)]),
    "q3_spk_encode": (c_int, [c_void_p, c_void_p, ctypes.c_int64, ctypes.c_uint32, c_void_p]),
    "q3_mimi_config_default": (c_int, [P(CMimiConfig)]),
    "q3_mimi_create": (c_int, [P(CMimiConfig), c_int, P(c_void_p)]),
    "q3_mimi_free": (None, [c_void_p]),
    "q3_mimi_get_config": (c_int, [c_void_p, P(CMimiConfig)]),
    "q3_mimi_n_tensors": (c_int, [c_void_p]),
    "q3_mimi_tensor_info": (c_int, [c_void_p, c_int, P(c_char_p), P(ctypes.c_int64)]),
    "q3_mimi_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, c_int, ctypes.c_int64]),
    "q3_mimi_finalize": (c_int, [c_void_p]),
    "q3_mimi_load_safetensors": (c_int, [c_void_p, c_char_p]),
    "q3_mimi_frames": (c_int, [P(CMimiConfig), ctypes.c_int64]),
    "q3_mimi_encode": (c_int, [c_void_p, c_void_p, ctypes.c_int64, ctypes.c_uint32, c_void_p, c_int, P(c_int), P(c_void_p)]),
    "q3_wav_info": (c_int, [c_char_p, P(CWavDesc)]),
    "q3_g711_to_pcm16": (c_int, [c_void_p, ctypes.c_int64, c_int, c_void_p]),
    "q3_intake_taps": (c_int, [ctypes.c_uint32, c_void_p, ctypes.c_size_t, P(c_int), P(c_int)]),
    "q3_intake_count": (c_int, [ctypes.c_uint32, ctypes.c_int64, P(ctypes.c_int64)]),
    "q3_ref_audio_create_many": (c_int, [c_int, c_int, P(CClip), P(c_void_p)]),
    "q3_ref_audio_create": (c_int, [c_int, P(CClip), P(c_void_p)]),
    "q3_ref_audio_from_wav": (c_int, [c_char_p, c_int, P(c_void_p)]),
    "q3_ref_audio_info": (c_int, [c_void_p, P(ctypes.c_int64), P(c_int), P(ctypes.c_uint32), P(c_int), P(c_int)]),
    "q3_ref_audio_read": (c_int, [c_void_p, c_void_p, ctypes.c_int64, P(ctypes.c_int64)]),
    "q3_ref_audio_free": (None, [c_void_p]),
    "q3_spk_encode_ref": (c_int, [c_void_p, c_void_p, c_void_p]),
    "q3_mimi_encode_ref": (c_int, [c_void_p, c_void_p, c_void_p, c_int, P(c_int), P(c_void_p)]),
    "q3_mimi_pack_plan": (c_int, [P(CMimiConfig), P(ctypes.c_int64), c_int, ctypes.c_int64, P(CMimiPackClip), P(ctypes.c_int64), P(c_int), P(c_int)]),
    "q3_mimi_encode_refs": (c_int, [c_void_p, P(c_void_p), c_int, c_void_p, c_int, P(c_int), P(c_void_p)]),
    "q3_spk_encode_refs": (c_int, [c_void_p, P(c_void_p), c_int, c_void_p, P(c_void_p)]),
}

for _name, (_res, _args) in SYMBOLS.items():
    _f = getattr(lib, _name)      # AttributeError here = header/library mismatch
    _f.restype = _res
    _f.argtypes = _args


class Q3Error(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"q3 status {status}: {msg}")
        self.status = status


def check(status):
    if status != 0:
        raise Q3Error(status, lib.q3_last_error().decode("utf-8", "replace"))
