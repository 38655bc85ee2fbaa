"""Many reference clips per encoder pass, the parts that need no device: the slot plan of the packed speech-encoder
pass (q3_mimi_pack_plan) against q3_mimi_frames and a by-hand count, a configuration it reports as not packable, and the refusals
of the two entry points that are decided before the device is touched."""
import ctypes

import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
from qwen3_tts_rs_amd.speech_encoder import pack_plan

NEW = ["q3_mimi_pack_plan", "q3_mimi_encode_refs", "q3_spk_encode_refs"]
CONFIGS = {"production": q.SpeechEncoderConfig, "tiny": q.tiny_speech_config}


def test_new_symbols_exported_bound_and_layered():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert ctypes.sizeof(_lib.CMimiPackClip) == 16
    assert callable(q.SpeechEncoder.encode_refs) and callable(q.SpeakerEncoder.encode_refs) and callable(q.Qwen3TTS.create_voice_clone_prompts)


def frames_of(cfg, n):
    c = cfg.to_c()
    return _lib.lib.q3_mimi_frames(ctypes.byref(c), n)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_plan_slots(name):
    cfg = CONFIGS[name]()
    S = 2
    for r in cfg.ratios:
        S *= r
    assert S == {"production": 1920, "tiny": 96}[name]
    lengths = [1, S - 1, S, S + 1, 3 * S + 7]
    p = pack_plan(cfg, lengths)
    assert p.frame_samples == S and p.packable and p.n_passes == 1 and p.passes == [0] * 5
    assert p.frames == [frames_of(cfg, n) for n in lengths] == [1, 1, 1, 2, 4]
    at = 0
    for T, start in zip(p.frames, p.starts):
        assert start % S == 0 and start == at              # whole frames, and each slot is its clip's frames plus one guard frame
        at += (T + 1) * S
    # any order: the plan follows the list
    pr = pack_plan(cfg, lengths[::-1])
    assert pr.frames == p.frames[::-1] and pr.starts[0] == 0 and pr.starts[1] == 5 * S


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_plan_passes_by_hand(name):
    cfg = CONFIGS[name]()
    S = pack_plan(cfg, [1]).frame_samples
    lengths = [1, S - 1, S, S + 1, 3 * S + 7]              # slots of 2, 2, 2, 3, 5 frames
    p = pack_plan(cfg, lengths, max_pass_samples=6 * S)
    assert p.passes == [0, 0, 0, 1, 2] and p.n_passes == 3  # 2 + 2 + 2 | 3 (+ 5 > 6) | 5
    assert p.starts == [0, 2 * S, 4 * S, 0, 0]
    p = pack_plan(cfg, lengths, max_pass_samples=5 * S)
    assert p.passes == [0, 0, 1, 1, 2] and p.starts == [0, 2 * S, 0, 2 * S, 0]
    # a slot larger than a pass gets a pass to itself
    p = pack_plan(cfg, lengths, max_pass_samples=2 * S)
    assert p.passes == [0, 1, 2, 3, 4] and p.starts == [0] * 5 and p.n_passes == 5
    # the library's own limit: 120 s of slots
    p = pack_plan(cfg, [24000 * 70, 24000 * 70])
    assert p.passes == [0, 1] and p.n_passes == 2
    p = pack_plan(cfg, [24000 * 50, 24000 * 50])
    assert p.passes == [0, 0]


def test_plan_not_packable():
    """One guard frame is 2 columns at 25 Hz: a last conv of 5 taps reaches 4 back. And 16 samples at stage 0 of a small S."""
    cfg = q.tiny_speech_config(); cfg.last_kernel = 5
    p = pack_plan(cfg, [100, 200])
    assert not p.packable and p.frames == [frames_of(cfg, 100), frames_of(cfg, 200)]
    cfg = q.tiny_speech_config(); cfg.ratios = [1, 1, 2, 2]; cfg.kernel = 11           # S = 8 < 10
    assert not pack_plan(cfg, [100]).packable
    cfg = q.tiny_speech_config(); cfg.ratios = [2, 3, 2, 1]; cfg.res_kernel = 5         # stage 3: 2 columns per frame < 4
    assert not pack_plan(cfg, [100]).packable
    assert pack_plan(q.tiny_speech_config(), [100]).packable and pack_plan(q.SpeechEncoderConfig(), [100]).packable


def test_plan_refusals():
    L = _lib.lib
    c = q.tiny_speech_config().to_c()
    ns = (ctypes.c_int64 * 3)(5, 0, 7)
    clips = (_lib.CMimiPackClip * 65)()
    assert L.q3_mimi_pack_plan(None, ns, 3, 1000, clips, None, None, None) == 1
    assert L.q3_mimi_pack_plan(ctypes.byref(c), None, 3, 1000, clips, None, None, None) == 1
    assert L.q3_mimi_pack_plan(ctypes.byref(c), ns, 3, 1000, None, None, None, None) == 1
    assert L.q3_mimi_pack_plan(ctypes.byref(c), ns, 0, 1000, clips, None, None, None) == 1
    assert L.q3_mimi_pack_plan(ctypes.byref(c), ns, 65, 1000, clips, None, None, None) == 1
    assert L.q3_mimi_pack_plan(ctypes.byref(c), ns, 3, 0, clips, None, None, None) == 1
    assert L.q3_mimi_pack_plan(ctypes.byref(c), ns, 3, 1000, clips, None, None, None) == 1 and b"clip 1" in L.q3_last_error()
    ns[1] = 9
    assert L.q3_mimi_pack_plan(ctypes.byref(c), ns, 3, 1000, clips, None, None, None) == 0      # the outputs beside the clips are optional


def test_entry_points_refuse_before_the_device():
    """Manifest-only encoders (device -1): every refusal below is decided before a handle's device matters."""
    L = _lib.lib
    mimi = q.SpeechEncoder(q.tiny_speech_config(), device=-1); spk = q.SpeakerEncoder(q.tiny_speaker_config(), device=-1)
    nulls = (ctypes.c_void_p * 65)()
    nf = (ctypes.c_int * 65)(); out = (ctypes.c_float * (65 * 64))()
    for name, call in (("q3_mimi_encode_refs", lambda e, refs, n: L.q3_mimi_encode_refs(e, refs, n, None, 0, nf, None)),
                       ("q3_spk_encode_refs", lambda e, refs, n: L.q3_spk_encode_refs(e, refs, n, out, None))):
        e = mimi._h if "mimi" in name else spk._h
        assert call(None, nulls, 1) == 1 and b"null argument" in L.q3_last_error(), name
        assert call(e, None, 1) == 1 and b"null argument" in L.q3_last_error(), name
        assert call(e, nulls, 0) == 1 and b"0 clips" in L.q3_last_error(), name
        assert call(e, nulls, 65) == 1 and b"65 clips" in L.q3_last_error(), name
        assert call(e, nulls, -3) == 1, name
        assert call(e, nulls, 4) == 1 and name.encode() + b": clip 0: null entry" in L.q3_last_error(), name
    assert L.q3_mimi_encode_refs(mimi._h, nulls, 1, None, 0, None, None) == 1                  # n_frames is not optional
    assert L.q3_spk_encode_refs(spk._h, nulls, 1, None, None) == 1                             # nor is the output
    assert all(v == 0 for v in nf) and all(v == 0.0 for v in out)                              # a refusal writes nothing
    mimi.close(); spk.close()


def test_frames_and_plan_out_of_range():
    """q3_mimi_frames: 0 for a stride outside 1 .. 16 (a stride of 0 used to divide by zero), -1 (no count) for n_samples above 2^48
    or a count beyond INT32_MAX (it used to add the stride to any n_samples and to truncate); q3_mimi_pack_plan refuses such a clip."""
    L = _lib.lib
    cfg = CONFIGS["production"]()
    c = cfg.to_c()
    assert L.q3_mimi_frames(ctypes.byref(c), 1 << 40) == ((1 << 40) + 1919) // 1920 and L.q3_mimi_frames(ctypes.byref(c), 1 << 48) == -1
    assert [L.q3_mimi_frames(ctypes.byref(c), n) for n in ((1 << 48) + 1, (1 << 63) - 1)] == [-1, -1]
    assert [L.q3_mimi_frames(ctypes.byref(c), n) for n in (0, -1, -(1 << 63))] == [0, 0, 0]
    for bad in (0, -4, 17):
        b = cfg.to_c(); b.ratios[2] = bad
        assert L.q3_mimi_frames(ctypes.byref(b), 24000) == 0
    one = cfg.to_c(); one.ratios[0] = one.ratios[1] = one.ratios[2] = one.ratios[3] = 1
    assert L.q3_mimi_frames(ctypes.byref(one), (1 << 32) - 2) == (1 << 31) - 1 and L.q3_mimi_frames(ctypes.byref(one), (1 << 32) - 1) == -1
    ns = (ctypes.c_int64 * 2)(24000, 1 << 48)
    clips = (_lib.CMimiPackClip * 2)()
    assert L.q3_mimi_pack_plan(ctypes.byref(c), ns, 2, 24000 * 120, clips, None, None, None) == 1 and b"clip 1" in L.q3_last_error()
