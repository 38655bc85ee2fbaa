"""encode_refs through the layers above it: create_voice_clone_prompts against the per-clip call for a mix of ICL and
x-vector-only clips, a session started from a prompt of the batch, and the CLI's --tokenize. Tiny configurations, clips under 0.5 s."""
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api, cli
from intake_cases import clip_samples, encode, write_wav

pytestmark = pytest.mark.gpu
SEED = 99


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    """three clips in three formats and rates: 0.3 s 44.1 kHz s16 stereo, 0.21 s 24 kHz f32 mono, 0.4 s 16 kHz u-law mono"""
    d = tmp_path_factory.mktemp("encode_refs")
    out = []
    for name, n, ch, rate, fmt, f0 in (("alpha", 13230, 2, 44100, "s16", 220.0), ("beta", 5003, 1, 24000, "f32", 140.0),
                                       ("gamma", 6400, 1, 16000, "ulaw", 310.0)):
        t = np.arange(n) / float(rate)
        x = clip_samples(n, ch, seed=len(out) + 5, sigma=0.05)
        x[:, 0] += 0.4 * np.sin(2 * np.pi * f0 * t)
        out.append(write_wav(d / f"{name}.wav", encode(np.clip(x, -1, 1), fmt), fmt, ch, rate))
    return out


@pytest.fixture(scope="module")
def model():
    cfg = q.tiny_speech_config(); cfg.n_q = 16               # the talker's ICL prompt takes 16 codebooks
    spk = q.SpeakerEncoder.from_synthetic(q.tiny_speaker_config(q.tiny().hidden), seed=SEED)
    mimi = q.SpeechEncoder.from_synthetic(cfg, seed=SEED)
    m = q.Qwen3TTS.from_synthetic(q.tiny())
    m.attach_speaker_encoder(spk); m.attach_speech_encoder(mimi)
    yield m
    m.speaker_encoder = None; m.speech_encoder = None
    m.close(); spk.close(); mimi.close()


def same_prompt(a, b):
    np.testing.assert_array_equal(a.speaker_embedding.view(np.uint32), b.speaker_embedding.view(np.uint32))
    for x, y in ((a.ref_codes, b.ref_codes), (a.ref_text_ids, b.ref_text_ids)):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape
            np.testing.assert_array_equal(x, y)


def test_prompts_equal_the_per_clip_call(model, wavs):
    refs = [api.RefAudio.from_wav(p) for p in wavs]
    texts = [[5, 6, 7], None, [9, 8]]
    batch = model.create_voice_clone_prompts(refs, texts)
    assert len(batch) == 3 and batch[1].ref_codes is None and batch[0].ref_codes.shape[1] == 16
    for p, r, t in zip(batch, refs, texts):
        same_prompt(p, model.create_voice_clone_prompt(r, ref_text_ids=t))
    for p, r in zip(model.create_voice_clone_prompts(refs), refs):      # all x-vector-only: the speech encoder is not called
        same_prompt(p, model.create_voice_clone_prompt(r))
    assert model.create_voice_clone_prompts([]) == []
    with pytest.raises(ValueError):
        model.create_voice_clone_prompts(refs, texts[:2])
    with pytest.raises(TypeError):
        model.create_voice_clone_prompts([api.AudioBuffer(refs[0].samples(), 24000)])
    # a session started from prompt 2 of the batch generates what the single prompt's session generates
    opts = q.SynthesisOptions(max_length=4, seed=4, eos_token_id=None)
    _, c_batch = model.synthesize_voice_clone_prompt([3, 4, 5, 6], batch[2], q.Language.English, opts)
    _, c_single = model.synthesize_voice_clone_prompt([3, 4, 5, 6], model.create_voice_clone_prompt(refs[2], ref_text_ids=texts[2]),
                                                      q.Language.English, opts)
    assert c_batch.shape == (4, 16)
    np.testing.assert_array_equal(c_batch, c_single)
    for r in refs:
        r.close()


def test_cli_tokenize(tmp_path, wavs, capsys):
    out_dir = tmp_path / "codes"
    assert cli.build_parser().parse_args([]).tokenize is None
    assert cli.main(["--synthetic", "tiny", "--tokenize"] + wavs + ["--output-dir", str(out_dir)]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Tokenized:")]
    assert len(lines) == 3 and "alpha.wav (0.30s, 44100 Hz)" in lines[0]
    enc = q.SpeechEncoder.from_synthetic(q.tiny_speech_config())      # the seeded tokenizer --synthetic tiny builds
    assert sorted(os.listdir(out_dir)) == ["alpha.codes.bin", "beta.codes.bin", "gamma.codes.bin"]
    for p, line in zip(wavs, lines):
        ref = api.RefAudio.from_wav(p)
        want = enc.encode_ref(ref)
        stem = os.path.splitext(os.path.basename(p))[0]
        got = api.load_codes_binary(str(out_dir / f"{stem}.codes.bin"), n_groups=enc.config.n_q)
        np.testing.assert_array_equal(got, want)
        assert line.endswith(f"({want.shape[0]} frames)")
        ref.close()
    enc.close()
    # two clips of one name would overwrite each other
    assert cli.main(["--synthetic", "tiny", "--tokenize", wavs[0], wavs[0], "--output-dir", str(out_dir)]) == 2
