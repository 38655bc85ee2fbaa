"""The output stage's formant step at 1.7B, synthetic weights, continuous stream mode, chunk 10, 200 frames,
16 kHz s16, B = 8 (the settings of pitch_ab.py, whose leg b at B = 8 is this tool's leg n on the commit before):
  leg n  next_chunks_out with nothing set: no stretcher, no pitch step, no formant step
  leg p  every row at +300 cents (the stretcher at 841, k_pitch at 841 / 1000)
  leg k  every row at +300 cents with keep = 1: leg p plus k_fm_frame and k_fm_ola
Every chunk round is `generate(chunk)` then `next_chunks_out`, timed apart. After a warm-up the legs alternate in one process, five
repetitions; median, minimum and maximum of the repetitions' means. `stage_*`: the stage alone (no model), pushes of one chunk's
19200 samples to 8 rows from the host, set as in the legs, and `f`: the formant step alone (a shift of +200 cents, no pitch).
`--stage-only` runs those rows alone, for a kernel trace. Prints one JSON object; `--table PATH` also writes a text table."""
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

REPS, CHUNK, FRAMES, PROMPT, RATE, B, CENTS = 5, 10, 200, 32, 16000, 8, 300
LEGS = "npk"


def setup(obj, leg, rows):
    """legs p / k / f on a Session (rows None: every row at once) or a PcmStage"""
    for r in ([-1] if rows is None else rows):
        args = (r,) if rows is not None else ()
        kw = {} if rows is not None else {"b": r}
        if leg in "pk":
            obj.set_pitch(*args, CENTS, **kw)
        if leg == "k":
            obj.set_formant(*args, True, 0, **kw)
        if leg == "f":
            obj.set_formant(*args, False, 200, **kw)


def run(model, leg, frames=FRAMES):
    utts = [q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    s = model.session(utts, q.SynthesisOptions(max_length=frames, eos_token_id=None, seed=42, chunk_frames=CHUNK))
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, 1))
    s.set_output(RATE, pcm16=True)
    setup(s, leg, None)
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


def table(out):
    rows = [f"leg   ms per round  med (min .. max)     generation med     chunk call med (min .. max)     B = {B}"]
    for leg in LEGS:
        e = out.get(f"leg_{leg}")
        if e:
            r, g, c = e["ms_per_round"], e["ms_generation"], e["ms_chunk_call"]
            rows.append(f"{leg}     {r['median']:9.3f} ({r['min']:.3f} .. {r['max']:.3f})   {g['median']:9.3f}          "
                        f"{c['median']:9.3f} ({c['min']:.3f} .. {c['max']:.3f})")
    rows.append(f"stage alone, ms per push of 19200 samples to {B} rows  med (min .. max)")
    for leg in LEGS + "f":
        m = out[f"stage_{leg}"]["ms_per_push"]
        rows.append(f"{leg}     {m['median']:9.3f} ({m['min']:.3f} .. {m['max']:.3f})")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--table", default=None, help="write a text table to this file")
    ap.add_argument("--stage-only", action="store_true",
                    help="the stage-alone rows only, no model (under `rocprofv3 --kernel-trace --stats -f csv -d DIR --`: the kernels' own time)")
    args = ap.parse_args()
    out = {"chunk_frames": CHUNK, "frames": FRAMES, "reps": REPS, "rate": RATE, "rows": B, "cents": CENTS}
    if not args.stage_only:
        model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
        for leg in LEGS:
            run(model, leg, frames=3 * CHUNK)                        # warm-up: allocations, the captured frame
        acc = {leg: [] for leg in LEGS}
        for rep in range(REPS):
            for leg in LEGS:
                acc[leg].append(run(model, leg))
                print(f"repetition {rep} leg {leg}: {sum(acc[leg][-1]):.3f} ms per round", file=sys.stderr, flush=True)
        model.close()
        for leg in LEGS:
            g, v = [a for a, _ in acc[leg]], [b for _, b in acc[leg]]
            out[f"leg_{leg}"] = {"ms_per_round": stats([a + b for a, b in acc[leg]]), "ms_generation": stats(g), "ms_chunk_call": stats(v)}
    for leg in LEGS + "f":
        out[f"stage_{leg}"] = {"ms_per_push": stats(stage_alone(leg))}
    print(json.dumps(out, indent=1))
    if args.table:
        with open(args.table, "w") as f:
            f.write(table(out))


if __name__ == "__main__":
    main()
