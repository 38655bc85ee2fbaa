"""Multi-row streaming at 1.7B, synthetic weights, continuous stream mode, chunk 10, 200 frames, B = 1 / 8 / 64:
  leg a  today's schedule: a loop of next_chunk_row over the rows (one vocoder pass per row and chunk, the front over all frames so far)
  leg b  next_chunks (one pass of the codec stream for all rows, per-row decoder state)
Every chunk round is `generate(chunk)` then the leg's chunk calls, timed apart: ms per round split into generation and vocoder,
streamed frames/s, and the per-round vocoder time at frame 20 and at frame 190 (the cost of leg b does not grow with the position).
After a warm-up the legs alternate in one process, five repetitions; median, minimum and maximum.
`--legs a` runs leg a alone (a build without next_chunks). Prints one JSON object; `--json PATH` also writes it to PATH."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import qwen3_tts_rs_amd as q                       # noqa: E402
from qwen3_tts_rs_amd import synth, _lib           # noqa: E402
from qwen3_tts_rs_amd.synth import synthetic_prompt      # noqa: E402

REPS, CHUNK, FRAMES, PROMPT = 5, 10, 200, 32


def run(model, B, leg, frames=FRAMES):
    utts = [q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    opts = q.SynthesisOptions(max_length=frames, eos_token_id=None, seed=42, chunk_frames=CHUNK)
    s = model.session(utts, opts)
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, 1))
    s.prefill()
    gen, voc = [], []
    for _ in range(frames // CHUNK):
        t0 = time.perf_counter()
        s.generate(CHUNK)
        t1 = time.perf_counter()
        if leg == "a":
            r = [s.next_chunk_row(b) for b in range(B)]
        else:
            r = s.next_chunks()
        t2 = time.perf_counter()
        assert all(a is not None and len(a) == CHUNK * model.config.samples_per_frame for a, _ in r)
        gen.append((t1 - t0) * 1e3); voc.append((t2 - t1) * 1e3)
    s.close()
    return gen, voc


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--legs", default="ab", choices=["ab", "a", "b"])
    ap.add_argument("--batches", default="1,8,64")
    args = ap.parse_args()
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    out = {"chunk_frames": CHUNK, "frames": FRAMES, "reps": REPS, "legs": args.legs}
    for B in [int(x) for x in args.batches.split(",")]:
        for leg in args.legs:
            run(model, B, leg, frames=3 * CHUNK)                     # warm-up: allocations, the captured frame
        acc = {leg: {"gen": [], "voc": [], "round": [], "fps": [], "voc_f20": [], "voc_f190": []} for leg in args.legs}
        for _ in range(REPS):
            for leg in args.legs:
                gen, voc = run(model, B, leg)
                a = acc[leg]
                a["gen"].append(float(np.mean(gen))); a["voc"].append(float(np.mean(voc)))
                a["round"].append(float(np.mean(gen) + np.mean(voc)))
                a["fps"].append(B * FRAMES / ((sum(gen) + sum(voc)) / 1e3))
                a["voc_f20"].append(voc[1]); a["voc_f190"].append(voc[FRAMES // CHUNK - 1])      # the rounds that end at frame 20 / 200
        for leg in args.legs:
            a = acc[leg]
            out[f"b{B}_{leg}"] = {"ms_per_round": stats(a["round"]), "ms_generation": stats(a["gen"]), "ms_vocoder": stats(a["voc"]),
                                  "streamed_frames_per_s": stats(a["fps"]), "ms_vocoder_round_to_frame_20": stats(a["voc_f20"]),
                                  "ms_vocoder_round_from_frame_190": stats(a["voc_f190"])}
    model.close()
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
