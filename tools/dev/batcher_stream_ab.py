"""Streamed batcher tickets at 1.7B, synthetic weights: the `eos_mix` queue of bench.py --full — 4 x slots
requests, 512 prompt tokens, lengths uniform 100 .. 640 frames (seed 2026), steps of 8 frames; bench.py keeps these inside its
main(), so they are restated here — through the native batcher with 8 and 64 slots:
  leg a  tickets with want_pcm = 1 on the PARENT commit (--legs a, this file run from a checkout and build of that commit: its
         package does not bind the streamed entry points and this one does not load a library without them)
  leg b  the same on this build
  leg c  streamed tickets (submit_streamed / read) on this build
Per leg and repetition: useful frames/s (all frames / wall from the first submit until every ticket is finished and fetched) and,
per ticket, the time from submit to its first and to its last sample (legs a / b: both are the moment the ticket polls DONE
after a step; leg c: the first non-empty read and the read that reports done, reads after every step). Leg c also reports the
block figures of the batcher's codec stream at the end, the steps per second and the samples that a step's read found.
After a warm-up the legs of one process alternate, --reps repetitions each. Prints one JSON object; --json PATH also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import qwen3_tts_rs_amd as q                       # noqa: E402
from qwen3_tts_rs_amd import synth                 # noqa: E402
from qwen3_tts_rs_amd.synth import synthetic_prompt      # noqa: E402

# bench.py's eos_mix (its main(), the block under "utterances that END AT DIFFERENT FRAMES": rng seed 2026, n_req = 4 * B, lengths
# rng.integers(min(100, frames), frames + 1), make_utt(i) = synthetic_prompt(--prompt-tokens 512, i) / Ryan / English / seed 42 + i,
# --frames 640, batcher steps of 8, prompt_budget 0) — locals of that function, so they cannot be imported: keep the two in step
FRAMES, PROMPT, POLL, SEED = 640, 512, 8, 2026


def mix(slots):
    rng = np.random.default_rng(SEED)
    lens = [int(x) for x in rng.integers(min(100, FRAMES), FRAMES + 1, size=4 * slots)]
    utts = []
    for i, L in enumerate(lens):
        u = q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i)
        u.max_length = L
        utts.append(u)
    return utts


def run(model, slots, leg, reqs, opts):
    bt = q.Batcher(model, slots=slots, frame_budget=FRAMES, prompt_budget=0, options=opts)
    try:
        t0 = time.perf_counter()
        tickets = [bt.submit_streamed(u) if leg == "c" else bt.submit(u, want_pcm=True) for u in reqs]
        first = {}; last = {}
        open_ = set(tickets)
        steps = 0; found = []
        while True:
            running, queued, _ = bt.step(POLL, True)
            steps += 1
            now = time.perf_counter() - t0
            got = 0
            for t in sorted(open_):
                if leg == "c":
                    a, done = bt.read(t)
                    got += a.size
                    if a.size and t not in first:
                        first[t] = now
                    if done:
                        last[t] = now; open_.discard(t)
                elif bt.poll(t)[0] == q.Batcher.DONE:
                    first[t] = last[t] = now; open_.discard(t)
            found.append(got)
            if running == 0 and queued == 0:
                break
        assert not open_
        info = bt.stream_info() if leg == "c" else None
        frames = sum(int(bt.fetch(t)[0].shape[0]) for t in tickets)
        wall = time.perf_counter() - t0
        r = {"frames": frames, "wall_s": wall, "frames_per_s": frames / wall, "steps": steps, "steps_per_s": steps / wall,
             "first_sample_ms": [1e3 * first[t] for t in tickets], "last_sample_ms": [1e3 * last[t] for t in tickets]}
        if info:
            r["stream_info"] = info
            r["samples_found_per_step_median"] = float(np.median(found))
        return r
    finally:
        bt.close()


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", default="bc", help="legs of this process, e.g. a, bc")
    ap.add_argument("--slots", default="8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args()
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    opts = q.SynthesisOptions(max_length=FRAMES, eos_token_id=None, seed=42)
    out = {"legs": args.legs, "reps": args.reps, "frames_max": FRAMES, "prompt_tokens": PROMPT, "step_frames": POLL,
           "library": os.environ.get("Q3TTS_LIB", "this build")}
    for slots in [int(x) for x in args.slots.split(",")]:
        reqs = mix(slots)
        for leg in args.legs:
            run(model, slots, leg, reqs[:slots + 2], opts)               # warm-up: the captured frame, side-session shapes, workspaces
        acc = {leg: [] for leg in args.legs}
        for _ in range(args.reps):
            for leg in args.legs:
                acc[leg].append(run(model, slots, leg, reqs, opts))
        for leg in args.legs:
            rs = acc[leg]
            o = {"frames_per_s": stats([r["frames_per_s"] for r in rs]), "frames_per_s_reps": [r["frames_per_s"] for r in rs],
                 "steps_per_s": stats([r["steps_per_s"] for r in rs]),
                 "first_sample_ms_median_per_rep": [float(np.median(r["first_sample_ms"])) for r in rs],
                 "last_sample_ms_median_per_rep": [float(np.median(r["last_sample_ms"])) for r in rs],
                 "first_sample_ms": stats(np.concatenate([r["first_sample_ms"] for r in rs])),
                 "last_sample_ms": stats(np.concatenate([r["last_sample_ms"] for r in rs])),
                 # the tickets that entered a row at once (the first `slots` of the queue): no queueing time in their figures
                 "first_sample_ms_first_wave": stats(np.concatenate([r["first_sample_ms"][:slots] for r in rs])),
                 "last_sample_ms_first_wave": stats(np.concatenate([r["last_sample_ms"][:slots] for r in rs]))}
            if "stream_info" in rs[-1]:
                o["stream_info"] = rs[-1]["stream_info"]
                o["samples_found_per_step_median"] = rs[-1]["samples_found_per_step_median"]
            out[f"slots{slots}_{leg}"] = o
    model.close()
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
