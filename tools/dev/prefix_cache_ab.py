"""Prefix cache at 1.7B, synthetic weights: what a hit saves. VoiceDesign requests with 300 / 1000 / 4096
instruct tokens (309 / 1009 / 4105 prefill positions), three legs in ONE process on one build, alternating per repetition:
  off   cache off (q3_model_prefix_cache(m, 0)): today's path
  miss  cache on, an instruction nobody has sent yet (a fresh one per repetition): the lookup and the insert on top of `off`
  hit   cache on, the instruction of the `miss` just before with another text, language and seed
Batch 1: wall time of q3_session_prefill (it returns once the prompt's kernels have landed) and time to first audio = session
creation to the first 10-frame chunk of a StreamingSession. Batcher: 8 slots, idle; one streamed ticket, submit to its first
sample (steps of 2 frames). After a warm-up of every leg and length, --reps repetitions; median (min .. max) per cell.
Prints a table and one JSON object; --out PATH writes the table, --json PATH the object.
profiles/prefix_cache_ab.txt is the table of `python tools/dev/prefix_cache_ab.py --reps 5 --out profiles/prefix_cache_ab.txt`."""
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

LENGTHS = (300, 1000, 4096)
_fresh = [5000]


def fresh_instruction(n):
    _fresh[0] += 1
    return [int(x) for x in synthetic_prompt(n, _fresh[0])]


def utt(instr, k):
    return q.Utterance(synthetic_prompt(32, k), language=[q.Language.English, q.Language.German][k % 2], instruct_ids=instr, seed=42 + k)


def prefill_ms(model, u, opts):
    s = model.session([u], opts)
    t0 = time.perf_counter(); s.prefill(); dt = 1e3 * (time.perf_counter() - t0)
    reused = s.prefix_info(0)
    s.close()
    return dt, reused


def ttfa_ms(model, u, opts):
    t0 = time.perf_counter()
    ss = q.StreamingSession(model, u, opts)
    c = ss.next_chunk()
    dt = 1e3 * (time.perf_counter() - t0)
    assert c is not None
    ss.close()
    return dt


def batcher_first_sample_ms(bt, u):
    t0 = time.perf_counter()
    t = bt.submit_streamed(u)
    first = None
    while True:
        running, queued, _ = bt.step(2, True)
        a, done = bt.read(t)
        if a.size and first is None:
            first = 1e3 * (time.perf_counter() - t0)
        if done or (running == 0 and queued == 0):
            break
    while not bt.read(t)[1]:
        bt.step(2, True)
    bt.fetch(t)
    return first


def cell(v):
    return f"{np.median(v):8.2f} ({np.min(v):.2f} .. {np.max(v):.2f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lengths", default=",".join(str(n) for n in LENGTHS))
    ap.add_argument("--pages", type=int, default=256, help="capacity of the cache in the miss / hit legs")
    ap.add_argument("--out", default=None); ap.add_argument("--json", default=None)
    args = ap.parse_args()
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    opts = q.SynthesisOptions(max_length=20, eos_token_id=None, seed=42, chunk_frames=10)
    bt = q.Batcher(model, slots=8, frame_budget=20, prompt_budget=4200, options=opts)
    measures = {"prefill_ms": lambda u: prefill_ms(model, u, opts)[0], "ttfa_ms": lambda u: ttfa_ms(model, u, opts),
                "batcher_first_sample_ms": lambda u: batcher_first_sample_ms(bt, u)}
    out = {"reps": args.reps, "pages": args.pages}
    lines = [f"prefix cache A/B, 1.7B synthetic weights, median (min .. max) of {args.reps}, ms",
             f"{'':34s}{'off':>28s}{'miss':>28s}{'hit':>28s}"]
    for n in [int(x) for x in args.lengths.split(",")]:
        for name, fn in measures.items():
            acc = {"off": [], "miss": [], "hit": []}
            for rep in range(-2, args.reps):                    # two warm-up rounds: side-session shapes, workspaces, the captured frame
                model.prefix_cache(0)
                a = fn(utt(fresh_instruction(n), 0))
                model.prefix_cache(args.pages)
                instr = fresh_instruction(n)
                b = fn(utt(instr, 1))
                c = fn(utt(instr, 2))
                if rep >= 0:
                    acc["off"].append(a); acc["miss"].append(b); acc["hit"].append(c)
            model.prefix_cache(args.pages)
            instr = fresh_instruction(n); prefill_ms(model, utt(instr, 1), opts)
            reused = prefill_ms(model, utt(instr, 2), opts)[1]
            model.prefix_cache(0)
            out[f"N{n}_{name}"] = {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in acc.items()}
            out[f"N{n}_reused_positions"] = reused
            lines.append(f"N={n:<5d}{name:<25s}{reused:>4d}" + "".join(f"{cell(acc[k]):>28s}" for k in ("off", "miss", "hit")))
    bt.close(); model.close()
    table = "\n".join(lines)
    print(table); print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
