"""The reference-audio intake in front of both encoders: a 1.7B-width synthetic speaker encoder and the full Mimi
configuration, clips of 10 s — one at 44.1 kHz s16 stereo, one at 8 kHz mu-law mono:
  leg a  today's path: AudioBuffer.load (q3_wav_read) + resample_to_24k (q3_resample) on the host, then both encode calls
         (the mu-law clip is expanded with q3_g711_to_pcm16 first: q3_wav_read does not read G.711)
  leg b  RefAudio.from_wav (k_intake), then both encode_ref calls
  leg c  eight clips through RefAudio.many (four of each kind), conversion alone
Every leg is timed on the host clock around calls that end in a device synchronise, split into conversion and encoders. After a
warm-up of every leg the legs alternate in one process, five repetitions; median (minimum .. maximum). Also checks that leg b's
24 kHz samples are within the rounding bound of leg a's, and prints the largest ratio. Prints a table; `--out PATH` also writes it."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import qwen3_tts_rs_amd as q                       # noqa: E402
from qwen3_tts_rs_amd import api                   # noqa: E402
from intake_cases import encode, error_ratio, write_wav      # noqa: E402

REPS, SECONDS = 5, 10


def make_clips(d):
    rng = np.random.default_rng(7)
    out = {}
    for name, sr, fmt, ch in (("44.1 kHz s16 stereo", 44100, "s16", 2), ("8 kHz mu-law mono", 8000, "ulaw", 1)):
        n = sr * SECONDS
        t = np.arange(n) / sr
        x = np.stack([0.3 * np.sin(2 * np.pi * (180.0 + 40 * c) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.3 * t)) for c in range(ch)], axis=1)
        x += 0.05 * rng.standard_normal((n, ch))
        out[name] = (write_wav(os.path.join(d, f"clip_{sr}.wav"), encode(np.clip(x, -1, 1), fmt), fmt, ch, sr), fmt)
    return out


def host_load(path, fmt):
    if fmt in ("ulaw", "alaw"):
        i = api.wav_info(path)
        raw = np.fromfile(path, np.uint8, count=i.data_bytes, offset=i.data_offset)
        return api.AudioBuffer(api.g711_expand(raw, fmt).astype(np.float32) / np.float32(32768.0), i.sample_rate)
    return api.AudioBuffer.load(path)


def leg_a(spk, mimi, path, fmt):
    t0 = time.perf_counter()
    a = api.resample_to_24k(host_load(path, fmt))
    t1 = time.perf_counter()
    spk.encode(a.samples, 24000); mimi.encode(a.samples, 24000)
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3


def leg_b(spk, mimi, path, fmt):
    t0 = time.perf_counter()
    r = api.RefAudio.from_wav(path)
    t1 = time.perf_counter()
    spk.encode_ref(r); mimi.encode_ref(r)
    t2 = time.perf_counter()
    r.close()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def leg_c(clips):
    raws = []
    for path, fmt in clips.values():
        i = api.wav_info(path)
        raws.append((np.fromfile(path, np.uint8, count=i.data_bytes, offset=i.data_offset), i.sample_rate, fmt, i.channels))
    t0 = time.perf_counter()
    rs = api.RefAudio.many(raws * 4)
    ms = (time.perf_counter() - t0) * 1e3
    for r in rs:
        r.close()
    return ms, 0.0


def fmt_stat(v):
    return f"{np.median(v):9.2f} ({np.min(v):.2f} .. {np.max(v):.2f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    spk = q.SpeakerEncoder.from_synthetic(q.SpeakerEncoderConfig(enc_dim=2048))
    mimi = q.SpeechEncoder.from_synthetic(None)
    lines = [f"intake_ab: {SECONDS} s clips, 1.7B-width speaker encoder + full Mimi, {REPS} repetitions, ms: median (min .. max)",
             f"{'clip':22s} {'leg':34s} {'conversion ms':>28s} {'encoders ms':>28s} {'conversion share':>17s}"]
    with tempfile.TemporaryDirectory() as d:
        clips = make_clips(d)
        for name, (path, fmt) in clips.items():
            if fmt == "s16":                                  # (q3_wav_read reads it: the comparison of tests/test_gpu_intake.py at full length)
                r = api.RefAudio.from_wav(path)
                lines.append(f"# {name}: largest |device - host| / bound over {len(r)} samples = {error_ratio(r.samples(), path):.3f}")
                r.close()
        legs = [("a host: load + resample_to_24k", leg_a), ("b device: RefAudio.from_wav", leg_b)]
        for name, (path, fmt) in clips.items():
            for _, f in legs:
                f(spk, mimi, path, fmt)                       # warm-up: workspaces, code objects, the table cache
        leg_c(clips)
        acc = {(name, leg): ([], []) for name in clips for leg, _ in legs}
        acc_c = []
        for rep in range(REPS):
            for name, (path, fmt) in clips.items():
                for leg, f in legs:
                    conv, enc = f(spk, mimi, path, fmt)
                    acc[(name, leg)][0].append(conv); acc[(name, leg)][1].append(enc)
                    print(f"repetition {rep} {name} leg {leg[0]}: conversion {conv:.2f} ms, encoders {enc:.2f} ms", file=sys.stderr, flush=True)
            acc_c.append(leg_c(clips)[0])
        for (name, leg), (conv, enc) in acc.items():
            share = np.median(conv) / (np.median(conv) + np.median(enc))
            lines.append(f"{name:22s} {leg:34s} {fmt_stat(conv):>28s} {fmt_stat(enc):>28s} {100 * share:16.1f}%")
        lines.append(f"{'4 + 4 clips':22s} {'c device: RefAudio.many (8 clips)':34s} {fmt_stat(acc_c):>28s} {'-':>28s} {'-':>17s}")
    spk.close(); mimi.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
