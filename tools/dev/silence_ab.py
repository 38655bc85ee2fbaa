"""The output stage's silence step at 1.7B, synthetic weights, continuous stream mode, chunk 10, 200 frames,
16 kHz s16, B = 1 / 8 / 64:
  leg a  next_chunks_out at 16 kHz s16 on a build of the commit before (this tool run from that tree with `--legs a`: it calls
         nothing new)
  leg b  next_chunks_out at 16 kHz s16, nothing set: the path of leg a, one more test per segment and no new launch, copy or wait
  leg c  the step on every row (-50 dBFS, edges 50 ms, pauses 400 ms): k_trim, the copy of the kept counts and the extra wait in
         front of the plan. Synthetic weights give noise at a steady level, so the step has little to cut: what is timed is the
         pre-pass, not a shorter stream
Every chunk round is `generate(chunk)` then `next_chunks_out`, timed apart: ms per round split into generation and the chunk call
(vocoder, silence step, resampler, copy). After a warm-up the legs alternate in one process, five repetitions; median, minimum and
maximum of the repetitions' means. `stage_*`: the stage alone (no model), pushes of one chunk's 19200 samples to B rows from the
host, set as in legs b / c, on a signal of bursts and pauses.
`--merge A.json` adds the legs of another run's JSON (leg a, from the tree of the commit before) and judges leg b against it: the
difference of the medians against the spread (max - min) of leg b's own repetitions, per round and in the chunk call.
Prints one JSON object; `--json PATH` also writes it to PATH, `--table PATH` a text table."""
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
SILENCE = (-50.0, 50, 400)


def run(model, B, leg, frames=FRAMES):
    utts = [q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    opts = q.SynthesisOptions(max_length=frames, eos_token_id=None, seed=42, chunk_frames=CHUNK)
    s = model.session(utts, opts)
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, 1))
    s.set_output(RATE, pcm16=True)                       # (the call of the commit before)
    if leg == "c":
        s.set_silence(*SILENCE)
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
    want = frames * model.config.samples_per_frame * RATE // 24000      # (the rows have not ended: the stage still holds their tails)
    if leg != "c":
        assert 0.9 * want * B <= total <= want * B + B, (total, want * B)
    kept = total / float(want * B)
    s.close()
    return gen, voc, kept


def stage_alone(B, leg, pushes=20):
    """ms per push of CHUNK frames' samples to every one of B rows (host in, host out), the first push (allocations) left out.
    The signal: 300 ms bursts at -20 dBFS and 700 ms pauses at -80 dBFS."""
    n = CHUNK * 1920
    rng = np.random.default_rng(1)
    t = np.arange(n * (pushes + 1))
    amp = np.where((t % 24000) < 7200, 0.1, 0.0001)
    x = (amp[None, :] * rng.standard_normal((B, n * (pushes + 1)))).astype(np.float32)
    ps = api.PcmStage(0, B, n)
    for r in range(B):
        ps.set(r, RATE, pcm16=True)
        if leg == "c":
            ps.set_silence(r, *SILENCE)
    ms = []
    for k in range(pushes + 1):
        t0 = time.perf_counter()
        ps.push({r: x[r, k * n:(k + 1) * n] for r in range(B)})
        ms.append((time.perf_counter() - t0) * 1e3)
    ps.close()
    return ms[1:]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def table(out, batches):
    rows = ["leg        B   ms per round  med (min .. max)     generation med     chunk call med (min .. max)"]
    for B in batches:
        for leg in "abc":
            e = out.get(f"b{B}_{leg}")
            if not e:
                continue
            r, g, c = e["ms_per_round"], e["ms_generation"], e["ms_chunk_call"]
            rows.append(f"{leg}  {B:8d}   {r['median']:9.3f} ({r['min']:.3f} .. {r['max']:.3f})   {g['median']:9.3f}          "
                        f"{c['median']:9.3f} ({c['min']:.3f} .. {c['max']:.3f})")
    for B in batches:
        j = out.get(f"b{B}_b_vs_a")
        if j:
            rows.append(f"B = {B}: chunk call b - a = {j['chunk_call_median_diff_ms']:+.3f} ms, round b - a = {j['round_median_diff_ms']:+.3f} ms; "
                        f"spread of b's repetitions {j['b_chunk_call_spread_ms']:.3f} ms (chunk call) / {j['b_round_spread_ms']:.3f} ms (round): "
                        f"{'within' if j['within_spread'] else 'OVER'}")
    for B in batches:
        j = out.get(f"b{B}_c_vs_b")
        if j:
            rows.append(f"B = {B}: chunk call c - b = {j['chunk_call_median_diff_ms']:+.3f} ms, round c - b = {j['round_median_diff_ms']:+.3f} ms "
                        f"(reported, not judged; leg c kept {j['kept_share']:.3f} of the samples)")
    rows.append("stage alone, ms per push of 19200 samples to B rows  med (min .. max)")
    for B in batches:
        for leg in "bc":
            e = out.get(f"stage_b{B}_{leg}")
            if e:
                m = e["ms_per_push"]
                rows.append(f"{leg}  {B:8d}   {m['median']:9.3f} ({m['min']:.3f} .. {m['max']:.3f})")
    for B in batches:
        e = out.get(f"stage_b{B}_k_trim")
        if e:
            rows.append(f"B = {B}: the pre-pass (k_trim, the count copy, the wait) adds {e['ms_per_push']:.3f} ms per push (c - b)")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--table", default=None, help="write a text table to this file")
    ap.add_argument("--merge", default=None, help="JSON of a run of leg a (from the tree of the commit before)")
    ap.add_argument("--legs", default="bc", help="any of a, b, c")
    ap.add_argument("--batches", default="1,8,64")
    args = ap.parse_args()
    batches = [int(x) for x in args.batches.split(",")]
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    out = {"chunk_frames": CHUNK, "frames": FRAMES, "reps": REPS, "legs": args.legs, "rate": RATE, "silence": list(SILENCE)}
    for B in batches:
        for leg in args.legs:
            run(model, B, leg, frames=3 * CHUNK)                     # warm-up: allocations, the captured frame
        acc = {leg: {"gen": [], "voc": [], "round": [], "kept": []} for leg in args.legs}
        for rep in range(REPS):
            for leg in args.legs:
                gen, voc, kept = run(model, B, leg)
                print(f"B = {B} repetition {rep} leg {leg}: {np.mean(gen) + np.mean(voc):.3f} ms per round", file=sys.stderr, flush=True)
                a = acc[leg]
                a["gen"].append(float(np.mean(gen))); a["voc"].append(float(np.mean(voc)))
                a["round"].append(float(np.mean(gen) + np.mean(voc))); a["kept"].append(kept)
        for leg in args.legs:
            a = acc[leg]
            out[f"b{B}_{leg}"] = {"ms_per_round": stats(a["round"]), "ms_generation": stats(a["gen"]), "ms_chunk_call": stats(a["voc"]),
                                  "kept_share": float(np.mean(a["kept"]))}
        if "b" in args.legs and "c" in args.legs:
            b, c = out[f"b{B}_b"], out[f"b{B}_c"]
            out[f"b{B}_c_vs_b"] = {"chunk_call_median_diff_ms": c["ms_chunk_call"]["median"] - b["ms_chunk_call"]["median"],
                                   "round_median_diff_ms": c["ms_per_round"]["median"] - b["ms_per_round"]["median"], "kept_share": c["kept_share"]}
    model.close()
    if "b" in args.legs:
        for B in batches:
            for leg in "bc":
                if leg in args.legs:
                    out[f"stage_b{B}_{leg}"] = {"ms_per_push": stats(stage_alone(B, leg))}
            if all(f"stage_b{B}_{leg}" in out for leg in "bc"):
                out[f"stage_b{B}_k_trim"] = {"ms_per_push": out[f"stage_b{B}_c"]["ms_per_push"]["median"] - out[f"stage_b{B}_b"]["ms_per_push"]["median"]}
    if args.merge:
        other = json.load(open(args.merge))
        for B in batches:
            if f"b{B}_a" in other and f"b{B}_b" in out:
                a, b = other[f"b{B}_a"], out[f"b{B}_b"]
                out[f"b{B}_a"] = a
                dc = b["ms_chunk_call"]["median"] - a["ms_chunk_call"]["median"]
                dr = b["ms_per_round"]["median"] - a["ms_per_round"]["median"]
                sc = b["ms_chunk_call"]["max"] - b["ms_chunk_call"]["min"]
                sr = b["ms_per_round"]["max"] - b["ms_per_round"]["min"]
                out[f"b{B}_b_vs_a"] = {"chunk_call_median_diff_ms": dc, "round_median_diff_ms": dr, "b_chunk_call_spread_ms": sc,
                                       "b_round_spread_ms": sr, "within_spread": bool(abs(dc) <= sc and abs(dr) <= sr)}
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    if args.table:
        with open(args.table, "w") as f:
            f.write(table(out, batches))


if __name__ == "__main__":
    main()
