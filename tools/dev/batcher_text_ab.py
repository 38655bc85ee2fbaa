"""Open batcher tickets at 1.7B, synthetic weights, on the queue of tools/dev/batcher_stream_ab.py (bench.py's
`eos_mix`: 4 x slots requests, 512 prompt tokens, lengths uniform 100 .. 640 frames, steps of 8 frames), 8 and 64 slots:
  leg a  closed streamed tickets (submit_streamed / read) on the PARENT commit (--legs a, this file run from a checkout and build
         of that commit: its package does not bind the open entry points and this one does not load a library without them)
  leg b  the same on this build: tickets that are not open must cost nothing
  leg c  open streamed tickets (submit_open / append_text / read): opened with one token, --feed tokens per ticket before every
         step (queued tickets included) until the 512 are in, then closed
Per leg and repetition: useful frames/s (all frames / wall from the first submit until every ticket is finished and fetched), ms
per step and, per ticket, the time from its submit — in leg c the moment its first token arrives — to its first sample. Leg c
also reports the time spent in text flushes per step (the library's Q3_BAT_TEXT_STATS counters, printed when the batcher is
freed) and how many row-steps were held. After a warm-up the legs of one process alternate, --reps repetitions each.
Prints one JSON object; --json PATH also writes it."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import qwen3_tts_rs_amd as q                       # noqa: E402
from qwen3_tts_rs_amd import synth                 # noqa: E402
from qwen3_tts_rs_amd.synth import synthetic_prompt      # noqa: E402

FRAMES, PROMPT, POLL, SEED = 640, 512, 8, 2026     # as tools/dev/batcher_stream_ab.py


def mix(slots):
    rng = np.random.default_rng(SEED)
    lens = [int(x) for x in rng.integers(min(100, FRAMES), FRAMES + 1, size=4 * slots)]
    utts = []
    for i, L in enumerate(lens):
        u = q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i)
        u.max_length = L
        utts.append(u)
    return utts


def first_token(u):
    v = q.Utterance(**{f: getattr(u, f) for f in u.__dataclass_fields__})
    v.text_ids = list(u.text_ids)[:1]
    return v


def close_with_stats(bt):
    """free the batcher with the library's stderr captured: the Q3_BAT_TEXT_STATS line"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            bt.close()
        finally:
            os.dup2(saved, 2); os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(r"(\d+) flushes in (\d+) steps, (\d+) tokens, ([0-9.]+) ms in flushes", text)
    return {"flushes": int(m.group(1)), "tokens": int(m.group(3)), "flush_ms": float(m.group(4))} if m else None


def run(model, slots, leg, reqs, opts, feed):
    bt = q.Batcher(model, slots=slots, frame_budget=FRAMES, prompt_budget=0, options=opts)
    closed = False
    try:
        t0 = time.perf_counter()
        if leg == "c":
            tickets = [bt.submit_open(first_token(u), "stream") for u in reqs]
            pos = {t: 1 for t in tickets}; text = {t: list(u.text_ids) for t, u in zip(tickets, reqs)}
        else:
            tickets = [bt.submit_streamed(u) for u in reqs]
            pos = {}
        first = {}
        open_ = set(tickets)
        steps = 0; held = 0
        while True:
            for t in list(pos):                      # leg c: the next tokens of every ticket whose text is not complete
                p = pos[t]; n = min(feed, len(text[t]) - p)
                bt.append_text(t, text[t][p:p + n], last=p + n == len(text[t]))
                if p + n == len(text[t]):
                    del pos[t]
                else:
                    pos[t] = p + n
            running, queued, _ = bt.step(POLL, True)
            steps += 1
            now = time.perf_counter() - t0
            for t in sorted(open_):
                a, done = bt.read(t)
                if a.size and t not in first:
                    first[t] = now
                if done:
                    open_.discard(t)
                elif leg == "c" and t in pos and bt.text_state(t)["frames_runnable"] == 0 and bt.poll(t)[0] == q.Batcher.RUNNING:
                    held += 1
            if running == 0 and queued == 0:
                break
        assert not open_
        frames = sum(int(bt.fetch(t)[0].shape[0]) for t in tickets)
        wall = time.perf_counter() - t0
        r = {"frames": frames, "wall_s": wall, "frames_per_s": frames / wall, "steps": steps, "ms_per_step": 1e3 * wall / steps,
             "first_sample_ms": [1e3 * first[t] for t in tickets]}
        if leg == "c":
            st = close_with_stats(bt); closed = True
            r["held_row_steps"] = held
            if st:
                r["flush_ms_per_step"] = st["flush_ms"] / steps; r["flushes"] = st["flushes"]; r["tokens_flushed"] = st["tokens"]
        return r
    finally:
        if not closed:
            bt.close()


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", default="bc", help="legs of this process, e.g. a, bc")
    ap.add_argument("--slots", default="8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--feed", type=int, default=10, help="leg c: tokens per ticket before every step")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args()
    os.environ["Q3_BAT_TEXT_STATS"] = "1"
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    opts = q.SynthesisOptions(max_length=FRAMES, eos_token_id=None, seed=42)
    out = {"legs": args.legs, "reps": args.reps, "frames_max": FRAMES, "prompt_tokens": PROMPT, "step_frames": POLL, "feed": args.feed}
    for slots in [int(x) for x in args.slots.split(",")]:
        reqs = mix(slots)
        for leg in args.legs:
            run(model, slots, leg, reqs[:slots + 2], opts, args.feed)       # warm-up: the captured frame, side-session shapes, workspaces
        acc = {leg: [] for leg in args.legs}
        for _ in range(args.reps):
            for leg in args.legs:
                acc[leg].append(run(model, slots, leg, reqs, opts, args.feed))
        for leg in args.legs:
            rs = acc[leg]
            o = {"frames_per_s": stats([r["frames_per_s"] for r in rs]), "frames_per_s_reps": [r["frames_per_s"] for r in rs],
                 "ms_per_step": stats([r["ms_per_step"] for r in rs]),
                 "first_sample_ms": stats(np.concatenate([r["first_sample_ms"] for r in rs])),
                 # the tickets that entered a row at once (the first `slots` of the queue): no queueing time in their figures
                 "first_sample_ms_first_wave": stats(np.concatenate([r["first_sample_ms"][:slots] for r in rs]))}
            if leg == "c":
                o["held_row_steps"] = [r["held_row_steps"] for r in rs]
                if "flush_ms_per_step" in rs[-1]:
                    o["flush_ms_per_step"] = stats([r["flush_ms_per_step"] for r in rs])
                    o["tokens_flushed"] = rs[-1]["tokens_flushed"]; o["flushes"] = rs[-1]["flushes"]
            out[f"slots{slots}_{leg}"] = o
    model.close()
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
