"""The output stage's keyed watermark: the decision threshold on the CPU, and the step's cost on the GPU.

`--threshold` (CPU, the f64 host detector): per clip length 3 / 6 / 10 s, PAIRS (key, signal) pairs of the seeded speech-like
synthetic of tests/mark_cases.py. Null scores: the unmarked signal, and the signal marked with ANOTHER key, both scored with the
pair's key. Marked scores: the signal marked with the pair's key at -26 dB (the default), at -20 dB and at the quieter -30 / -34 dB.
Also the round trip of the default mark through the stage's own formats on the host (q3_resample + the G.711 helpers): 16 kHz s16
and 8 kHz mu-law, marked and null. Prints the distributions (min, 1 %, median, 99 %, max); `--table PATH` appends them to a file.

GPU legs (1.7B, synthetic weights, continuous stream mode, chunk 10, 200 frames, 16 kHz s16, B = 8):
  leg a  next_chunks_out on a build of the commit before (this tool run from that tree with `--legs a`: it calls nothing new)
  leg b  next_chunks_out, nothing set: the path of leg a
  leg c  the mark on every row (a key per row, the default strength): k_mark in the chain
ms per chunk round split into generation and the chunk call; after a warm-up the legs alternate in one process, REPS repetitions;
median, minimum and maximum of the repetitions' means. `--merge A.json` adds leg a from another run's JSON and judges leg b against
it: |median b - median a| against the spread (max - min) of leg a's own repetitions; both spreads are reported. `stage_*`: the stage
alone (no model), pushes of one chunk's 19200 samples to B rows from the host.
Prints one JSON object; `--json PATH` also writes it to PATH, `--table PATH` a text table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qwen3_tts_rs_amd as q                       # noqa: E402
from qwen3_tts_rs_amd import api, synth, _lib      # noqa: E402
from qwen3_tts_rs_amd.synth import synthetic_prompt      # noqa: E402

REPS, CHUNK, FRAMES, PROMPT, RATE = 5, 10, 200, 32, 16000
PAIRS, LENGTHS, DEFAULT_MB, OTHERS = 200, (3.0, 6.0, 10.0), -2600, (-2000, -3000, -3400)


def key_of(i, salt=0):
    return ((i + 1) * 0x9E3779B97F4A7C15 + salt * 0xD1B54A32D192ED03) & ((1 << 64) - 1) or 1


def dist(v):
    v = np.asarray(v, np.float64)
    return {"n": int(v.size), "min": float(v.min()), "p01": float(np.percentile(v, 1)), "median": float(np.median(v)),
            "p99": float(np.percentile(v, 99)), "max": float(v.max())}


def threshold(pairs=PAIRS):
    import mark_cases as M
    out = {}
    for sec in LENGTHS:
        null_plain, null_cross, marked = [], [], []
        quiet = {mb: [] for mb in OTHERS}
        rt = {k: [] for k in ("16k_s16_marked", "16k_s16_null", "8k_ulaw_marked", "8k_ulaw_null")}
        for i in range(pairs):
            x = M.speechlike(1000 * int(sec) + i, sec)
            key, other = key_of(i), key_of(i, 1)
            y = M.lib_embed(x, key, DEFAULT_MB)
            null_plain.append(M.lib_detect(x, key)[0])
            null_cross.append(M.lib_detect(M.lib_embed(x, other, DEFAULT_MB), key)[0])
            marked.append(M.lib_detect(y, key)[0])
            for mb in OTHERS:
                quiet[mb].append(M.lib_detect(M.lib_embed(x, key, mb), key)[0])
            if i < pairs // 4:                                     # (the host resampler is the slow part)
                for name, rate, fmt in (("16k_s16", 16000, "s16"), ("8k_ulaw", 8000, "ulaw")):
                    rt[name + "_marked"].append(M.lib_detect(M.host_round_trip(y, rate, fmt), key)[0])
                    rt[name + "_null"].append(M.lib_detect(M.host_round_trip(x, rate, fmt), key)[0])
        e = {"null_unmarked": dist(null_plain), "null_other_key": dist(null_cross), f"marked_{DEFAULT_MB}": dist(marked)}
        for mb in OTHERS:
            e[f"marked_{mb}"] = dist(quiet[mb])
        for k, v in rt.items():
            e["roundtrip_" + k] = dist(v)
        out[f"{sec:g}s"] = e
        print(f"{sec:g} s done", file=sys.stderr, flush=True)
    return out


def threshold_table(out):
    rows = [f"scores of q3_mark_detect (f64, CPU), {PAIRS} (key, signal) pairs per length (round trips: {PAIRS // 4}), speech-like synthetic",
            "length  population              n      min     1 %   median    99 %      max"]
    for sec, e in out.items():
        for name, d in e.items():
            rows.append(f"{sec:>6}  {name:<22} {d['n']:4d} {d['min']:8.3f} {d['p01']:7.3f} {d['median']:8.3f} {d['p99']:7.3f} {d['max']:8.3f}")
    return "\n".join(rows) + "\n"


def run(model, B, leg, frames=FRAMES):
    utts = [q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    opts = q.SynthesisOptions(max_length=frames, eos_token_id=None, seed=42, chunk_frames=CHUNK)
    s = model.session(utts, opts)
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, 1))
    s.set_output(RATE, pcm16=True)                       # (the call of the commit before)
    if leg == "c":
        for b in range(B):
            s.set_mark(key_of(b), b=b)
    s.prefill()
    gen, voc = [], []
    for k in range(frames // CHUNK):
        t0 = time.perf_counter()
        s.generate(CHUNK)
        t1 = time.perf_counter()
        s.next_chunks_out()
        t2 = time.perf_counter()
        gen.append((t1 - t0) * 1e3); voc.append((t2 - t1) * 1e3)
    s.close()
    return gen, voc


def stage_alone(B, leg, pushes=20):
    """ms per push of CHUNK frames' samples to every one of B rows (host in, host out), the first push (allocations) left out"""
    n = CHUNK * 1920
    rng = np.random.default_rng(1)
    x = (0.1 * rng.standard_normal((B, n * (pushes + 1)))).astype(np.float32)
    ps = api.PcmStage(0, B, n)
    for r in range(B):
        ps.set(r, RATE, pcm16=True)
        if leg == "c":
            ps.set_mark(r, key_of(r))
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
            if e:
                r, g, c = e["ms_per_round"], e["ms_generation"], e["ms_chunk_call"]
                rows.append(f"{leg}  {B:8d}   {r['median']:9.3f} ({r['min']:.3f} .. {r['max']:.3f})   {g['median']:9.3f}          "
                            f"{c['median']:9.3f} ({c['min']:.3f} .. {c['max']:.3f})")
        j = out.get(f"b{B}_b_vs_a")
        if j:
            rows.append(f"B = {B}: chunk call b - a = {j['chunk_call_median_diff_ms']:+.3f} ms; spread of a's repetitions {j['a_chunk_call_spread_ms']:.3f} ms, "
                        f"of b's {j['b_chunk_call_spread_ms']:.3f} ms: {'within' if j['within_spread'] else 'OVER'}")
        j = out.get(f"b{B}_c_vs_b")
        if j:
            rows.append(f"B = {B}: chunk call c - b = {j['chunk_call_median_diff_ms']:+.3f} ms per chunk (reported, not judged)")
        for leg in "bc":
            e = out.get(f"stage_b{B}_{leg}")
            if e:
                m = e["ms_per_push"]
                rows.append(f"stage alone {leg}  {B:4d}   {m['median']:9.3f} ({m['min']:.3f} .. {m['max']:.3f}) ms per push of 19200 samples to B rows")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--threshold", action="store_true", help="the CPU measurement of the score distributions; no GPU")
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--table", default=None, help="write a text table to this file")
    ap.add_argument("--merge", default=None, help="JSON of a run of leg a (from the tree of the commit before)")
    ap.add_argument("--legs", default="bc", help="any of a, b, c")
    ap.add_argument("--batches", default="8")
    args = ap.parse_args()
    if args.threshold:
        out = threshold(args.pairs)
        print(json.dumps(out, indent=1))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)
        if args.table:
            with open(args.table, "w") as f:
                f.write(threshold_table(out))
        return
    batches = [int(x) for x in args.batches.split(",")]
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    out = {"chunk_frames": CHUNK, "frames": FRAMES, "reps": REPS, "legs": args.legs, "rate": RATE}
    for B in batches:
        for leg in args.legs:
            run(model, B, leg, frames=3 * CHUNK)                     # warm-up: allocations, the captured frame
        acc = {leg: {"gen": [], "voc": [], "round": []} for leg in args.legs}
        for rep in range(REPS):
            for leg in args.legs:
                gen, voc = run(model, B, leg)
                print(f"B = {B} repetition {rep} leg {leg}: {np.mean(gen) + np.mean(voc):.3f} ms per round", file=sys.stderr, flush=True)
                a = acc[leg]
                a["gen"].append(float(np.mean(gen))); a["voc"].append(float(np.mean(voc))); a["round"].append(float(np.mean(gen) + np.mean(voc)))
        for leg in args.legs:
            a = acc[leg]
            out[f"b{B}_{leg}"] = {"ms_per_round": stats(a["round"]), "ms_generation": stats(a["gen"]), "ms_chunk_call": stats(a["voc"])}
        if "b" in args.legs and "c" in args.legs:
            b, c = out[f"b{B}_b"], out[f"b{B}_c"]
            out[f"b{B}_c_vs_b"] = {"chunk_call_median_diff_ms": c["ms_chunk_call"]["median"] - b["ms_chunk_call"]["median"]}
    model.close()
    if "a" not in args.legs:
        for B in batches:
            for leg in args.legs:
                out[f"stage_b{B}_{leg}"] = {"ms_per_push": stats(stage_alone(B, leg))}
    if args.merge:
        other = json.load(open(args.merge))
        for B in batches:
            if f"b{B}_a" in other and f"b{B}_b" in out:
                a, b = other[f"b{B}_a"], out[f"b{B}_b"]
                out[f"b{B}_a"] = a
                dc = b["ms_chunk_call"]["median"] - a["ms_chunk_call"]["median"]
                sa = a["ms_chunk_call"]["max"] - a["ms_chunk_call"]["min"]
                sb = b["ms_chunk_call"]["max"] - b["ms_chunk_call"]["min"]
                out[f"b{B}_b_vs_a"] = {"chunk_call_median_diff_ms": dc, "a_chunk_call_spread_ms": sa, "b_chunk_call_spread_ms": sb,
                                       "within_spread": bool(abs(dc) <= sa)}
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    if args.table:
        with open(args.table, "w") as f:
            f.write(table(out, batches))


if __name__ == "__main__":
    main()
