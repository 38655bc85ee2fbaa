"""The output stage's pitch step at 1.7B, synthetic weights, continuous stream mode, chunk 10, 200 frames,
16 kHz s16, B = 1 / 8 / 64:
  leg a  next_chunks_out at 16 kHz s16 on a build of the commit before (this tool run from that tree with `--legs a`: it calls
         nothing new)
  leg b  next_chunks_out at 16 kHz s16, no pitch set: the path of leg a, one more branch per row in the plan and no new launch
  leg c  every row at +200 cents (the stretcher at 891, k_pitch at 891 / 1000)
  leg d  every row at -1200 cents (the stretcher at 2000, k_pitch at 2: the most outputs per input)
Every chunk round is `generate(chunk)` then `next_chunks_out`, timed apart: ms per round split into generation and the chunk call
(vocoder, stretcher, pitch step, resampler, copy). After a warm-up the legs alternate in one process, five repetitions; median,
minimum and maximum of the repetitions' means. `stage_*`: the stage alone (no model), pushes of one chunk's 19200 samples to B rows
from the host, set as in legs b / c / d, and `t` with the stretcher alone at 891 / 2000 — what k_pitch's launch adds to a push is
the difference to the row that runs the same stretcher without it.
`--merge A.json` adds the legs of another run's JSON (leg a, from the tree of the commit before) and judges leg b against it: the
difference of the medians of the chunk call against the spread (max - min) of leg b's own repetitions.
`--stage-only` runs those rows alone, for a kernel trace.
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
CENTS = {"c": 200, "d": -1200}


def setup(obj, leg, rows):
    """legs c / d on a Session (rows None: every row at once) or a PcmStage; tc / td: the stretcher of c / d without the pitch step"""
    if leg in CENTS:
        if rows is None:
            obj.set_pitch(CENTS[leg])
        else:
            for r in rows:
                obj.set_pitch(r, CENTS[leg])
    elif leg in ("tc", "td"):
        for r in rows:
            obj.set_tempo(r, api.pcm_stage_pitch_plan(1000, CENTS[leg[1]])[0])


def run(model, B, leg, frames=FRAMES):
    utts = [q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    opts = q.SynthesisOptions(max_length=frames, eos_token_id=None, seed=42, chunk_frames=CHUNK)
    s = model.session(utts, opts)
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, 1))
    s.set_output(RATE, pcm16=True)                       # (the call of the commit before)
    setup(s, leg, None)
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
    assert 0.9 * want * B <= total <= want * B + 2 * B, (total, want * B)
    s.close()
    return gen, voc


def stage_alone(B, leg, pushes=20):
    """ms per push of CHUNK frames' samples to every one of B rows (host in, host out), the first push (allocations) left out."""
    n = CHUNK * 1920
    rng = np.random.default_rng(1)
    x = (0.1 * rng.standard_normal((B, n * (pushes + 1)))).astype(np.float32)
    ps = api.PcmStage(0, B, n)
    for r in range(B):
        ps.set(r, RATE, pcm16=True)
    setup(ps, leg, range(B))
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
        for leg in "abcd":
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
    rows.append("stage alone, ms per push of 19200 samples to B rows  med (min .. max)")
    for B in batches:
        for leg in ("b", "c", "tc", "d", "td"):
            e = out.get(f"stage_b{B}_{leg}")
            if e:
                m = e["ms_per_push"]
                rows.append(f"{leg:2s} {B:8d}   {m['median']:9.3f} ({m['min']:.3f} .. {m['max']:.3f})")
    for B in batches:
        e = out.get(f"stage_b{B}_k_pitch")
        if e:
            rows.append(f"B = {B}: +200 cents adds {e['c_ms_per_push']:.3f} ms per push over b, of it k_pitch {e['c_k_pitch_ms_per_push']:.3f} (c - the "
                        f"stretcher alone at 891); -1200 cents adds {e['d_ms_per_push']:.3f}, of it k_pitch {e['d_k_pitch_ms_per_push']:.3f} (d - the "
                        f"stretcher alone at 2000)")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--table", default=None, help="write a text table to this file")
    ap.add_argument("--merge", default=None, help="JSON of a run of leg a (from the tree of the commit before)")
    ap.add_argument("--legs", default="bcd", help="any of a, b, c, d")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--stage-only", action="store_true",
                    help="the stage-alone rows only, no model (under `rocprofv3 --kernel-trace --stats -f csv -d DIR --`: k_pitch's own time)")
    args = ap.parse_args()
    batches = [int(x) for x in args.batches.split(",")]
    if args.stage_only:
        out = {f"stage_b{B}_{leg}": {"ms_per_push": stats(stage_alone(B, leg))} for B in batches for leg in ("b", "c", "tc", "d", "td")}
        print(json.dumps(out, indent=1))
        return
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    out = {"chunk_frames": CHUNK, "frames": FRAMES, "reps": REPS, "legs": args.legs, "rate": RATE, "cents": CENTS}
    for B in batches:
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
    if "b" in args.legs:
        for B in batches:
            for leg in "bcd":
                if leg in args.legs:
                    out[f"stage_b{B}_{leg}"] = {"ms_per_push": stats(stage_alone(B, leg))}
                    if leg in CENTS:
                        out[f"stage_b{B}_t{leg}"] = {"ms_per_push": stats(stage_alone(B, "t" + leg))}
            if all(f"stage_b{B}_{leg}" in out for leg in "bcd"):
                m = {leg: out[f"stage_b{B}_{leg}"]["ms_per_push"]["median"] for leg in ("b", "c", "d", "tc", "td")}
                out[f"stage_b{B}_k_pitch"] = {"c_ms_per_push": m["c"] - m["b"], "c_k_pitch_ms_per_push": m["c"] - m["tc"],
                                              "d_ms_per_push": m["d"] - m["b"], "d_k_pitch_ms_per_push": m["d"] - m["td"]}
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
                                       "b_round_spread_ms": sr, "within_spread": bool(dc <= sc and dr <= sr)}
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    if args.table:
        with open(args.table, "w") as f:
            f.write(table(out, batches))


if __name__ == "__main__":
    main()
