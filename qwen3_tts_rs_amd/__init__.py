"""qwen3_tts_rs_amd — MI355X-native (gfx950) hot path of Qwen3-TTS behind the reference's
generation/session API. See DESIGN.md / INTEGRATION.md; the C ABI is include/q3tts.h."""
from .config import Q3Config, qwen3_tts_0_6b, qwen3_tts_1_7b, tiny, tiny_same_width
from .api import (Qwen3TTS, Session, Parked, Batcher, StreamingSession, TextStreamingSession, SynthesisOptions, SynthesisTiming, AudioBuffer, Utterance,
                  Speaker, Language, CODEC_EOS_TOKEN_ID, SAMPLES_PER_FRAME, codes_to_tensor, auto_device,
                  fused_residual_rmsnorm, linear, linear_ex, attn_step, attn_step_ex, kv_pages_to_bf16_ex, gemm_ex, gemm_path, attn_prefill_ex, attn_prefill_packed_ex, prefill_pack_plan, attn_prefill_path, prompt_rows_ex, conv_ex, conv_path, conv_path_name, resunit_path, norm_c, dwconv7, sample, row_move,
                  attn_c_ex, attn_c_path, rope_c_ex, copy_cols_ex, copy_segs_ex, gather_frames_ex, rvq_embed_ex, silu_mul_ex, spk_op_ex, mimi_op_ex, mimi_rvq_ex, RefAudio,
                  prompt_shape, sample_row, sample_ex, frame_embed_ex, cp_gather_ex, rmsnorm_ex)
from .speaker import SpeakerEncoder, SpeakerEncoderConfig, VoiceClonePrompt, tiny_speaker_config
from .speech_encoder import SpeechEncoder, SpeechEncoderConfig, tiny_speech_config

__all__ = ["Q3Config", "qwen3_tts_0_6b", "qwen3_tts_1_7b", "tiny", "tiny_same_width", "Qwen3TTS", "Session", "Parked", "row_move",
           "StreamingSession", "TextStreamingSession", "SynthesisOptions", "SynthesisTiming", "AudioBuffer", "Utterance", "Speaker", "Language",
           "CODEC_EOS_TOKEN_ID", "SAMPLES_PER_FRAME", "codes_to_tensor", "auto_device", "fused_residual_rmsnorm",
           "linear", "linear_ex", "attn_step", "attn_step_ex", "kv_pages_to_bf16_ex", "gemm_ex", "gemm_path", "attn_prefill_ex", "attn_prefill_packed_ex", "prefill_pack_plan", "attn_prefill_path", "prompt_rows_ex", "conv_ex", "conv_path", "conv_path_name", "resunit_path", "norm_c", "dwconv7", "sample",
           "attn_c_ex", "attn_c_path", "rope_c_ex", "copy_cols_ex", "copy_segs_ex", "gather_frames_ex", "rvq_embed_ex", "silu_mul_ex", "spk_op_ex", "mimi_op_ex", "mimi_rvq_ex", "SpeakerEncoder", "SpeakerEncoderConfig", "VoiceClonePrompt", "tiny_speaker_config",
           "SpeechEncoder", "SpeechEncoderConfig", "tiny_speech_config", "RefAudio",
           "prompt_shape", "sample_row", "sample_ex", "frame_embed_ex", "cp_gather_ex", "rmsnorm_ex"]
