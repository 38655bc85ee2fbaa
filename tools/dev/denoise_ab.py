"""The spectral noise suppressor beside the two encoders it stands in front of: a 1.7B-width synthetic speaker
encoder and the full Mimi configuration, on the gated-tone-plus-noise probe of the tests at 10 s:
  one clip     RefAudio.denoise, RefAudio.noise, then encode_ref of both encoders on the result
  eight clips  RefAudio.denoise_many in one call, then encode_refs of both encoders on the results
Every figure is a host clock around calls that end in a device synchronise. After a warm-up of every leg, five repetitions;
median (minimum .. maximum). There is no host implementation to race: the figure that matters is the suppressor's share of the
time the encoders take. Prints a table; `--out PATH` also writes it."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import qwen3_tts_rs_amd as q                       # noqa: E402
from qwen3_tts_rs_amd import api                   # noqa: E402
from denoise_cases import probe, snr_db            # noqa: E402

REPS, SECONDS, BATCH = 5, 10, 8


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def fmt_stat(v):
    return f"{np.median(v):9.3f} ({np.min(v):.3f} .. {np.max(v):.3f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    spk = q.SpeakerEncoder.from_synthetic(q.SpeakerEncoderConfig(enc_dim=2048))
    mimi = q.SpeechEncoder.from_synthetic(None)
    n = 24000 * SECONDS
    clips = [probe(n, seed=s) for s in range(BATCH)]
    refs = api.RefAudio.many([(c[0], 24000, "f32") for c in clips])
    acc = {k: [] for k in ("denoise 1", "noise 1", "encoders 1", "denoise 8", "encoders 8")}
    for rep in range(REPS + 1):                                  # repetition 0 is the warm-up
        row = {}
        row["denoise 1"], one = timed(lambda: refs[0].denoise(12.0))
        row["noise 1"], est = timed(refs[0].noise)
        row["encoders 1"], _ = timed(lambda: (spk.encode_ref(one), mimi.encode_ref(one)))
        row["denoise 8"], many = timed(lambda: api.RefAudio.denoise_many(refs, 12.0))
        row["encoders 8"], _ = timed(lambda: (spk.encode_refs(many), mimi.encode_refs(many)))
        if rep == 0:
            y = one.samples()
            head = (f"# clip 0: SNR against the clean tones {snr_db(clips[0][0], clips[0][1]):.2f} dB in, {snr_db(y, clips[0][1]):.2f} dB out; "
                    f"estimated noise {est[0]:.2f} dBFS, estimated SNR {est[1]:.2f} dB")
        else:
            for k, v in row.items():
                acc[k].append(v)
        print(f"repetition {rep}: " + ", ".join(f"{k} {v:.3f} ms" for k, v in row.items()), file=sys.stderr, flush=True)
        one.close()
        for r in many:
            r.close()
    lines = [f"denoise_ab: {SECONDS} s clips at 24 kHz, 1.7B-width speaker encoder + full Mimi, {REPS} repetitions, ms: median (min .. max)", head,
             f"{'clips':6s} {'step':42s} {'ms':>32s} {'of the encoders':>16s}"]
    for cnt in ("1", "8"):
        enc = np.median(acc["encoders " + cnt])
        for k, label in (("denoise " + cnt, "RefAudio.denoise" + ("_many" if cnt == "8" else "")), ("noise " + cnt, "RefAudio.noise"),
                         ("encoders " + cnt, "encode_ref" + ("s" if cnt == "8" else "") + " (speaker + Mimi)")):
            if k in acc:
                lines.append(f"{cnt:6s} {label:42s} {fmt_stat(acc[k]):>32s} {100 * np.median(acc[k]) / enc:15.1f}%")
    for r in refs:
        r.close()
    spk.close(); mimi.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
