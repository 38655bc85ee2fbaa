"""The output stage's time stretcher at 1.7B, synthetic weights, continuous stream mode, chunk 10, 200 frames,
16 kHz s16, B = 1 / 8 / 64:
  leg a  next_chunks_out on a build of the commit before (this tool run from that tree with `--legs a`: it calls nothing new)
  leg b  next_chunks_out, no tempo set: the path of leg a, no new launch
  leg c  every row at 1250
  leg d  every row at 500: the most frames of the stretcher per chunk
Every chunk round is `generate(chunk)` then `next_chunks_out`, timed apart: ms per round split into generation and the chunk call
(vocoder, stretcher, resampler, copy). After a warm-up the legs alternate in one process, five repetitions; median, minimum and
maximum of the repetitions' means. For legs c / d the stretcher's frames per chunk call (from the streaming rule) are reported
with the chunk call's added time over leg b. `stage_*`: the stage alone (no model), pushes of one chunk's 19200 samples to B rows
from the host at tempo 1000 / 1250 / 500 — what the stretcher's launch adds to a push, per frame of its chain.
Prints one JSON object; `--json PATH` also writes it to PATH."""
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
TEMPO = {"a": 1000, "b": 1000, "c": 1250, "d": 500}


def run(model, B, leg, frames=FRAMES):
    utts = [q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    opts = q.SynthesisOptions(max_length=frames, eos_token_id=None, seed=42, chunk_frames=CHUNK)
    s = model.session(utts, opts)
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, 1))
    s.set_output(RATE, pcm16=True)
    if TEMPO[leg] != 1000:
        s.set_tempo(TEMPO[leg])
    s.prefill()
    gen, voc = [], []
    total = 0
    for k in range(frames // CHUNK):
        t0 = time.perf_counter()
        s.generate(CHUNK)
        t1 = time.perf_counter()
        r = s.next_chunks_out()
        t2 = time.perf_counter()
        total += sum(len(a) for a, _ in r if a is not None)
        gen.append((t1 - t0) * 1e3); voc.append((t2 - t1) * 1e3)
    n24 = frames * model.config.samples_per_frame
    want = n24 * 1000 // TEMPO[leg] * RATE // 24000          # (the rows have not ended: the stage still holds their tails)
    assert 0.9 * want * B <= total <= want * B + B, (total, want * B)
    s.close()
    return gen, voc


def stage_alone(B, tempo, pushes=20):
    """ms per push of CHUNK frames' samples to every one of B rows (host in, host out), the first push (allocations) left out."""
    n = CHUNK * 1920
    rng = np.random.default_rng(1)
    x = (0.1 * rng.standard_normal((B, n * (pushes + 1)))).astype(np.float32)
    ps = api.PcmStage(0, B, n)
    for r in range(B):
        ps.set(r, RATE, True)
        if tempo != 1000:
            ps.set_tempo(r, tempo)
    ms = []
    for k in range(pushes + 1):
        t0 = time.perf_counter()
        ps.push({r: x[r, k * n:(k + 1) * n] for r in range(B)})
        ms.append((time.perf_counter() - t0) * 1e3)
    ps.close()
    return ms[1:]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--legs", default="bcd", help="any of a, b, c, d")
    ap.add_argument("--batches", default="1,8,64")
    args = ap.parse_args()
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    spf = model.config.samples_per_frame
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
            e = {"ms_per_round": stats(a["round"]), "ms_generation": stats(a["gen"]), "ms_chunk_call": stats(a["voc"])}
            if TEMPO[leg] != 1000:
                f, _ = api.pcm_stage_tempo_count(TEMPO[leg], FRAMES * spf)
                e["stretcher_frames_per_chunk_call"] = f / (FRAMES // CHUNK)
                if "b" in acc:
                    e["ms_chunk_call_added_over_b"] = float(np.median(a["voc"]) - np.median(acc["b"]["voc"]))
                    e["us_added_per_stretcher_frame"] = 1e3 * e["ms_chunk_call_added_over_b"] / e["stretcher_frames_per_chunk_call"]
            out[f"b{B}_{leg}"] = e
    model.close()
    if "b" in args.legs:
        for B in [int(x) for x in args.batches.split(",")]:
            base = None
            for tempo in (1000, 1250, 500):
                ms = stage_alone(B, tempo)
                e = {"ms_per_push": stats(ms)}
                if tempo == 1000:
                    base = float(np.median(ms))
                else:
                    frames = CHUNK * spf * 1000 / (360 * tempo)
                    e["stretcher_frames_per_push"] = frames
                    e["us_added_per_stretcher_frame"] = 1e3 * (float(np.median(ms)) - base) / frames
                out[f"stage_b{B}_t{tempo}"] = e
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
