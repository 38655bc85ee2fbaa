"""Parked tickets at 1.7B, synthetic weights: a saturated batcher — every row busy with a long streamed ticket — and a
new request. A = today's batcher (the request waits for a row to END), B = the time slice (quantum_frames: the ticket that ran
longest in its row is parked, the request takes the row). Reports, per variant: submit -> first audio of the late request in ms
and in steps, the wall time until everything has finished (what parking costs the running tickets), the scheduler's counts
(q3_batcher_park_info), ms per park + resume pair measured at the session level (Session.park_row / resume_row at a frame
boundary), and whether every ticket's codes equal between A and B. Prints one JSON object; `--json PATH` also writes it to PATH."""
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

STEP = 8


def utterance(i, n_text, frames):
    u = q.Utterance(synthetic_prompt(n_text, i), q.Speaker.Ryan, q.Language.English, seed=42 + i)
    u.max_length = frames
    return u


def saturated(model, slots, frames, late_frames, n_text, **parking):
    """`slots` long tickets, two steps, then one late request: (ms and steps to its first audio, total ms, park_info, codes)"""
    b = q.Batcher(model, slots=slots, frame_budget=frames, prompt_budget=16,
                  options=q.SynthesisOptions(max_length=frames, eos_token_id=None, seed=42), **parking)
    tickets = [b.submit_streamed(utterance(i, n_text, frames)) for i in range(slots)]
    t_all = time.perf_counter()
    b.step(STEP); b.step(STEP)
    for t in tickets:
        b.read(t)
    late = b.submit_streamed(utterance(1000, n_text, late_frames))
    t0 = time.perf_counter(); first_ms, first_steps, steps = None, None, 0
    while True:
        running, queued, _ = b.step(STEP)
        steps += 1
        for t in tickets:
            b.read(t)
        a, _done = b.read(late)
        if a.size and first_ms is None:
            first_ms, first_steps = (time.perf_counter() - t0) * 1000.0, steps
        if running == 0 and queued == 0:
            break
    total_ms = (time.perf_counter() - t_all) * 1000.0
    info = b.park_info()
    codes = [b.fetch(t)[0] for t in tickets + [late]]
    b.close()
    return first_ms, first_steps, total_ms, info, codes


def park_pair_ms(model, rows, n_text, reps=20):
    """ms of one park + resume of a row of a `rows`-row session between two frames (the session's other rows stand still for it)"""
    utts = [utterance(i, n_text, 4 * reps + 16) for i in range(rows)]
    s = model.session(utts, q.SynthesisOptions(max_length=4 * reps + 16, eos_token_id=None, seed=42))
    s.prefill(); s.generate(8)
    ms = []
    for r in range(reps + 1):
        t = time.perf_counter()
        p = s.park_row(r % rows); s.resume_row(r % rows, p)
        ms.append((time.perf_counter() - t) * 1000.0)
        s.generate(2)
    s.close()
    return float(np.median(ms[1:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--frames", type=int, default=640, help="length of the tickets that fill the rows")
    ap.add_argument("--late-frames", type=int, default=64)
    ap.add_argument("--quantum", type=int, default=32)
    ap.add_argument("--text", type=int, default=64, help="text tokens per request")
    ap.add_argument("--tiny", action="store_true", help="the tiny configuration (a quick check of the tool itself)")
    args = ap.parse_args()
    cfg = q.tiny() if args.tiny else q.qwen3_tts_1_7b()
    model = q.Qwen3TTS.from_synthetic(cfg, seed=synth.DEFAULT_SEED)
    saturated(model, args.slots, 32, 8, args.text)                     # warm-up: kernels loaded, the first slab allocated
    a = saturated(model, args.slots, args.frames, args.late_frames, args.text)
    b = saturated(model, args.slots, args.frames, args.late_frames, args.text, max_parked=args.slots, quantum_frames=args.quantum,
                  fresh_first=True)
    out = {"slots": args.slots, "frames": args.frames, "late_frames": args.late_frames, "quantum_frames": args.quantum, "step_frames": STEP,
           "a_first_audio_ms": a[0], "a_first_audio_steps": a[1], "a_total_ms": a[2],
           "b_first_audio_ms": b[0], "b_first_audio_steps": b[1], "b_total_ms": b[2], "b_park_info": b[3],
           "codes_equal": bool(all(np.array_equal(x, y) for x, y in zip(a[4], b[4]))),
           "park_resume_pair_ms": park_pair_ms(model, args.slots, args.text)}
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f)
    model.close()


if __name__ == "__main__":
    main()
