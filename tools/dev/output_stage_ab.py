"""The output stage at 1.7B, synthetic weights, continuous stream mode, chunk 10, 200 frames, B = 1 / 8 / 64:
  leg a  next_chunks: 24 kHz f32
  leg b  next_chunks_out at 16 kHz s16 (the stage behind the vocoder's last kernel, in front of the copy to the host)
  leg c  leg a followed by the host helpers on each chunk: q3_resample to 16 kHz + q3_pcm16_from_f32
Every chunk round is `generate(chunk)` then the leg's chunk call, timed apart: ms per round split into generation and the chunk
call (vocoder, and for legs b / c the conversion). After a warm-up the legs alternate in one process, five repetitions; median,
minimum and maximum. `--legs a` runs leg a alone (a build without the stage: the yardstick of leg b is leg a of the commit before
it). Prints one JSON object; `--json PATH` also writes it to PATH."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import qwen3_tts_rs_amd as q                       # noqa: E402
from qwen3_tts_rs_amd import api, synth, _lib      # noqa: E402
from qwen3_tts_rs_amd.synth import synthetic_prompt      # noqa: E402

REPS, CHUNK, FRAMES, PROMPT, RATE = 5, 10, 200, 32, 16000


def run(model, B, leg, frames=FRAMES):
    utts = [q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    opts = q.SynthesisOptions(max_length=frames, eos_token_id=None, seed=42, chunk_frames=CHUNK)
    s = model.session(utts, opts)
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, 1))
    if leg == "b":
        s.set_output(RATE, pcm16=True)
    s.prefill()
    gen, voc = [], []
    n24 = CHUNK * model.config.samples_per_frame
    for k in range(frames // CHUNK):
        t0 = time.perf_counter()
        s.generate(CHUNK)
        t1 = time.perf_counter()
        if leg == "b":
            r = s.next_chunks_out()
        else:
            r = s.next_chunks()
            if leg == "c":
                r = [(api.pcm16(api.resample(a, RATE).samples), d) for a, d in r]
        t2 = time.perf_counter()
        if leg == "a":
            assert all(a is not None and len(a) == n24 for a, _ in r)
        elif leg == "c":
            assert all(len(a) == n24 * RATE // 24000 for a, _ in r)
        else:   # the stage holds 64 input samples back until the row ends
            assert all(a is not None and abs(len(a) - n24 * RATE // 24000) <= 64 for a, _ in r)
        gen.append((t1 - t0) * 1e3); voc.append((t2 - t1) * 1e3)
    s.close()
    return gen, voc


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--legs", default="abc", help="any of a, b, c")
    ap.add_argument("--batches", default="1,8,64")
    args = ap.parse_args()
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    out = {"chunk_frames": CHUNK, "frames": FRAMES, "reps": REPS, "legs": args.legs, "output": f"{RATE} Hz s16"}
    for B in [int(x) for x in args.batches.split(",")]:
        for leg in args.legs:
            run(model, B, leg, frames=3 * CHUNK)                     # warm-up: allocations, the captured frame
        acc = {leg: {"gen": [], "voc": [], "round": []} for leg in args.legs}
        for rep in range(REPS):
            for leg in args.legs:
                gen, voc = run(model, B, leg)
                print(f"B = {B} repetition {rep} leg {leg}: {np.mean(gen) + np.mean(voc):.3f} ms per round", file=sys.stderr, flush=True)
                a = acc[leg]
                a["gen"].append(float(np.mean(gen))); a["voc"].append(float(np.mean(voc)))
                a["round"].append(float(np.mean(gen) + np.mean(voc)))
        for leg in args.legs:
            a = acc[leg]
            out[f"b{B}_{leg}"] = {"ms_per_round": stats(a["round"]), "ms_generation": stats(a["gen"]), "ms_chunk_call": stats(a["voc"])}
    model.close()
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
