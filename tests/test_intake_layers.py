"""The intake through the layers above it: both encoders read a RefAudio where it lies and give the bits they give for
the same samples from the host; the host-side doors stay shut for other rates; create_voice_clone_prompt takes either kind of
reference; the CLI's --ref-intake. Tiny encoder configurations, a 0.3 s clip."""
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api, cli
from intake_cases import clip_samples, encode, write_wav

pytestmark = pytest.mark.gpu
SEED = 99


@pytest.fixture(scope="module")
def encoders():
    spk = q.SpeakerEncoder.from_synthetic(q.tiny_speaker_config(q.tiny().hidden), seed=SEED)
    mimi = q.SpeechEncoder.from_synthetic(q.tiny_speech_config(), seed=SEED)
    yield spk, mimi
    spk.close(); mimi.close()


@pytest.fixture(scope="module")
def clip44k(tmp_path_factory):
    """0.3 s at 44.1 kHz, s16 stereo: a tone with a little noise, the channels different."""
    n = 13230
    t = np.arange(n) / 44100.0
    x = clip_samples(n, 2, seed=44, sigma=0.05)
    x[:, 0] += 0.4 * np.sin(2 * np.pi * 220.0 * t); x[:, 1] += 0.3 * np.sin(2 * np.pi * 331.0 * t + 0.4)
    return write_wav(tmp_path_factory.mktemp("intake") / "clip44k.wav", encode(np.clip(x, -1, 1), "s16"), "s16", 2, 44100)


def test_hand_off_is_bitwise(encoders, clip44k):
    spk, mimi = encoders
    ref = api.RefAudio.from_wav(clip44k)
    x = ref.samples()
    assert x.size == api.intake_count(44100, 13230) == 7200
    np.testing.assert_array_equal(spk.encode_ref(ref).view(np.uint32), spk.encode(x, 24000).view(np.uint32))
    taps = [np.zeros(s, np.float32) for s in mimi.tap_shapes(x.size)]; taps_ref = [np.zeros_like(t) for t in taps]
    codes = mimi.encode(x, 24000, taps=taps)
    np.testing.assert_array_equal(mimi.encode_ref(ref, taps=taps_ref), codes)
    assert codes.shape == (mimi.frames(x.size), mimi.config.n_q)
    for a, b in zip(taps_ref, taps):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_array_equal(ref.samples().view(np.uint32), x.view(np.uint32))      # the encoders left the object as it was
    ref.close()


def test_the_old_doors_stay_shut(encoders):
    spk, mimi = encoders
    x = np.zeros(13230, np.float32)
    with pytest.raises(_lib.Q3Error, match="resample") as e:
        spk.encode(x, 44100)
    assert e.value.status == 7                               # Q3_UNSUPPORTED
    with pytest.raises(_lib.Q3Error, match="q3_resample") as e:
        mimi.encode(x, 44100)
    assert e.value.status == 1                               # Q3_INVALID_ARG


def test_device_mismatch_and_short_clips_are_statuses(encoders, clip44k):
    spk, mimi = encoders
    ref = api.RefAudio.from_wav(clip44k)
    off_spk = q.SpeakerEncoder(q.tiny_speaker_config(), device=-1); off_mimi = q.SpeechEncoder(q.tiny_speech_config(), device=-1)
    with pytest.raises(_lib.Q3Error, match="device") as e:
        off_spk.encode_ref(ref)
    assert e.value.status == 1
    with pytest.raises(_lib.Q3Error, match="device") as e:
        off_mimi.encode_ref(ref)
    assert e.value.status == 1
    off_spk.close(); off_mimi.close()
    if _lib.lib.q3_device_count() > 1:
        far = api.RefAudio.from_wav(clip44k, device=1)
        with pytest.raises(_lib.Q3Error, match="device") as e:
            spk.encode_ref(far)
        assert e.value.status == 1
        far.close()
    ref.close()
    short = api.RefAudio.from_samples(encode(clip_samples(300, 1, seed=3), "s16"), 24000, "s16")      # one mel frame: reflect padding needs more
    with pytest.raises(_lib.Q3Error, match="too short") as e:
        spk.encode_ref(short)
    assert e.value.status == 1
    with pytest.raises(_lib.Q3Error, match="too short") as e2:
        spk.encode(short.samples(), 24000)
    assert e2.value.status == e.value.status
    np.testing.assert_array_equal(mimi.encode_ref(short), mimi.encode(short.samples()))      # (the speech encoder takes any length from one sample)
    short.close()


def test_prompt_takes_either_reference(encoders, clip44k):
    spk, mimi = encoders
    m = q.Qwen3TTS.from_synthetic(q.tiny())
    m.attach_speaker_encoder(spk); m.attach_speech_encoder(mimi)
    ref = api.RefAudio.from_wav(clip44k)
    p = m.create_voice_clone_prompt(ref)
    assert p.ref_codes is None
    np.testing.assert_array_equal(p.speaker_embedding.view(np.uint32), spk.encode_ref(ref).view(np.uint32))
    p = m.create_voice_clone_prompt(ref, ref_text_ids=[5, 6, 7])
    np.testing.assert_array_equal(p.speaker_embedding.view(np.uint32), spk.encode_ref(ref).view(np.uint32))
    np.testing.assert_array_equal(p.ref_codes, mimi.encode_ref(ref))
    assert list(p.ref_text_ids) == [5, 6, 7]
    # an AudioBuffer takes exactly the path it took: the two host-side encode calls
    buf = api.AudioBuffer(ref.samples(), 24000)
    p = m.create_voice_clone_prompt(buf, ref_text_ids=[5, 6, 7])
    np.testing.assert_array_equal(p.speaker_embedding.view(np.uint32), spk.encode(buf.samples, 24000).view(np.uint32))
    np.testing.assert_array_equal(p.ref_codes, mimi.encode(buf.samples, 24000))
    ref.close()
    m.speaker_encoder = None; m.speech_encoder = None      # the fixture owns them
    m.close()


def test_cli_ref_intake(tmp_path, clip44k, capsys):
    base = ["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "5", "--no-eos", "--seed", "7", "--ref-audio", clip44k,
            "--x-vector-only"]
    assert cli.build_parser().parse_args(base).ref_intake == "host"

    def run(tag, extra):
        capsys.readouterr()
        assert cli.main(base + ["--output-dir", str(tmp_path / tag)] + extra) == 0
        out = capsys.readouterr().out
        files = {f: open(tmp_path / tag / f, "rb").read() for f in sorted(os.listdir(tmp_path / tag))}
        # what a run prints, without its wall-clock figures and with its own output directory named alike
        lines = [l.split(" frames in ")[0].replace(str(tmp_path / tag), "<out>") for l in out.splitlines()
                 if not l.startswith(("Loaded model in", "Stages:"))]
        return lines, files
    plain, plain_files = run("a", [])
    host, host_files = run("b", ["--ref-intake", "host"])
    assert any(l.startswith("Reference audio:") and l.endswith("(0.30s, 44100 Hz)") for l in plain)
    assert any(l.startswith("Generated: 0.40s, 9600 samples, 5") for l in plain) and "Saved WAV to: <out>/audio_seed7_frames5.wav" in plain
    assert host == plain                                     # --ref-intake host is the default: the path and the output it was
    assert host_files == plain_files
    dev, dev_files = run("c", ["--ref-intake", "device"])
    assert any(l.startswith("Reference audio:") and l.endswith("(0.30s, 44100 Hz, s16, 2 ch)") for l in dev)
    wavs = [f for f in dev_files if f.endswith(".wav")]
    assert wavs and sorted(dev_files) == sorted(plain_files)
    import wave
    with wave.open(str(tmp_path / "c" / wavs[0])) as w:
        assert (w.getnframes(), w.getframerate()) == (5 * 1920, 24000)
