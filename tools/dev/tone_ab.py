"""The output stage's tone step at 1.7B, synthetic weights, continuous stream mode, chunk 10, 200 frames,
16 kHz s16, B = 8 (the settings of formant_ab.py, whose leg n is this tool's leg n):
  leg n  next_chunks_out with nothing set: no tone step
  leg t  every row with 8 bands (all five kinds): leg n plus k_tone, one workgroup per row
Every chunk round is `generate(chunk)` then `next_chunks_out`, timed apart. After a warm-up the legs alternate in one process, five
repetitions; median, minimum and maximum of the repetitions' means. `stage_*`: the stage alone (no model), pushes of one chunk's
19200 samples to 8 rows from the host, set as in the legs. `--legs n` runs leg n alone: the same file in a tree of the parent
commit measures "nothing set" on the parent build in the same visit. `--stage-only` runs the stage rows alone, for a kernel
trace. Prints one JSON object; `--table PATH` also writes a text table."""
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

REPS, CHUNK, FRAMES, PROMPT, RATE, B = 5, 10, 200, 32, 16000, 8
BANDS = "hp:120,ls:200:4:0.8,peak:450:-6:2,peak:1000:3:1,peak:3000:6:4,peak:5200:-9:6,hs:8000:-2,lp:10500:0:0.9"


def run(model, leg, frames=FRAMES):
    utts = [q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    s = model.session(utts, q.SynthesisOptions(max_length=frames, eos_token_id=None, seed=42, chunk_frames=CHUNK))
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, 1))
    s.set_output(RATE, pcm16=True)
    if leg == "t":
        s.set_tone(BANDS)
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
    return float(np.mean(gen)), float(np.mean(voc))


def stage_alone(leg, pushes=20):
    """ms per push of CHUNK frames' samples to every one of B rows (host in, host out), the first push (allocations) left out."""
    n = CHUNK * 1920
    x = (0.1 * np.random.default_rng(1).standard_normal((B, n * (pushes + 1)))).astype(np.float32)
    ps = api.PcmStage(0, B, n)
    for r in range(B):
        ps.set(r, RATE, pcm16=True)
        if leg == "t":
            ps.set_tone(r, BANDS)
    ms = []
    for k in range(pushes + 1):
        t0 = time.perf_counter()
        ps.push({r: x[r, k * n:(k + 1) * n] for r in range(B)})
        ms.append((time.perf_counter() - t0) * 1e3)
    ps.close()
    return ms[1:]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def table(out, legs):
    rows = [f"leg   ms per round  med (min .. max)     generation med     chunk call med (min .. max)     B = {B}"]
    for leg in legs:
        e = out.get(f"leg_{leg}")
        if e:
            r, g, c = e["ms_per_round"], e["ms_generation"], e["ms_chunk_call"]
            rows.append(f"{leg}     {r['median']:9.3f} ({r['min']:.3f} .. {r['max']:.3f})   {g['median']:9.3f}          "
                        f"{c['median']:9.3f} ({c['min']:.3f} .. {c['max']:.3f})")
    rows.append(f"stage alone, ms per push of 19200 samples to {B} rows  med (min .. max)")
    for leg in legs:
        m = out[f"stage_{leg}"]["ms_per_push"]
        rows.append(f"{leg}     {m['median']:9.3f} ({m['min']:.3f} .. {m['max']:.3f})")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--table", default=None, help="write a text table to this file")
    ap.add_argument("--legs", default="nt", help="the legs to run (n alone: what a tree of the parent commit can run)")
    ap.add_argument("--stage-only", action="store_true",
                    help="the stage-alone rows only, no model (under `rocprofv3 --kernel-trace --stats -f csv -d DIR --`: the kernels' own time)")
    args = ap.parse_args()
    out = {"chunk_frames": CHUNK, "frames": FRAMES, "reps": REPS, "rate": RATE, "rows": B, "bands": BANDS, "lib": _lib.LIB_PATH}
    if not args.stage_only:
        model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
        for leg in args.legs:
            run(model, leg, frames=3 * CHUNK)                        # warm-up: allocations, the captured frame
        acc = {leg: [] for leg in args.legs}
        for rep in range(REPS):
            for leg in args.legs:
                acc[leg].append(run(model, leg))
                print(f"repetition {rep} leg {leg}: {sum(acc[leg][-1]):.3f} ms per round", file=sys.stderr, flush=True)
        model.close()
        for leg in args.legs:
            g, v = [a for a, _ in acc[leg]], [b for _, b in acc[leg]]
            out[f"leg_{leg}"] = {"ms_per_round": stats([a + b for a, b in acc[leg]]), "ms_generation": stats(g), "ms_chunk_call": stats(v)}
    for leg in args.legs:
        out[f"stage_{leg}"] = {"ms_per_push": stats(stage_alone(leg))}
    print(json.dumps(out, indent=1))
    if args.table:
        with open(args.table, "w") as f:
            f.write(table(out, args.legs))


if __name__ == "__main__":
    main()
