"""Block-allocated against whole-row codec stream state at the production decoder shape: the same pushes — R rows x 8
frames per push, 80 pushes per row (640 frames), random codes — on a stream of q3_codec_stream_create (leg u) and on one of
q3_codec_stream_create_blocked with 128-frame blocks (leg b). A push is synchronous, so its wall time is the pass: front over the
new columns (attention k_attn_cs / k_attn_cb over the row's cache), column copies, stack, samples to the host. Reports ms per push
around frame 100 and around frame 600 (pushes 10-19 and 70-79), legs alternating, five repetitions; R = 8 and 64.
Prints one JSON object; --json PATH also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import qwen3_tts_rs_amd as q                       # noqa: E402

REPS, STEP, PUSHES, BLOCK = 5, 8, 80, 128


def run(model, rows, leg, codes):
    cs = model.codec_stream(rows, STEP * PUSHES, block_frames=BLOCK if leg == "b" else 0)
    ms = []
    for k in range(PUSHES):
        part = {r: codes[r][k * STEP:(k + 1) * STEP] for r in range(rows)}
        t0 = time.perf_counter()
        cs.push(part)
        ms.append((time.perf_counter() - t0) * 1e3)
    cs.close()
    return ms


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rows", default="8,64")
    args = ap.parse_args()
    t = q.tiny()           # the talker does not run here: a tiny LM under the production decoder
    cfg = q.Q3Config(text_dim=t.text_dim, hidden=t.hidden, inter=t.inter, n_layers=t.n_layers, n_heads=t.n_heads, n_kv_heads=t.n_kv_heads,
                     cp_hidden=t.cp_hidden, cp_inter=t.cp_inter, cp_layers=t.cp_layers, cp_heads=t.cp_heads, cp_kv_heads=t.cp_kv_heads,
                     name="tiny-lm-full-decoder")
    model = q.Qwen3TTS.from_synthetic(cfg)
    out = {"frames_per_push": STEP, "pushes": PUSHES, "block_frames": BLOCK, "reps": REPS}
    for rows in [int(x) for x in args.rows.split(",")]:
        rng = np.random.default_rng(rows)
        codes = [rng.integers(0, 2048, size=(STEP * PUSHES, 16)).astype(np.uint32) for _ in range(rows)]
        for leg in "ub":
            run(model, rows, leg, codes)             # warm-up: workspaces, blocks in the device cache
        acc = {leg: {"f100": [], "f600": [], "all": []} for leg in "ub"}
        for _ in range(REPS):
            for leg in "ub":
                ms = run(model, rows, leg, codes)
                acc[leg]["f100"].append(float(np.median(ms[10:20]))); acc[leg]["f600"].append(float(np.median(ms[70:80])))
                acc[leg]["all"].append(float(np.sum(ms)))
        for leg in "ub":
            out[f"rows{rows}_{'whole_row' if leg == 'u' else 'blocked'}"] = {
                "ms_per_push_near_frame_100": stats(acc[leg]["f100"]), "ms_per_push_near_frame_600": stats(acc[leg]["f600"]),
                "ms_all_80_pushes": stats(acc[leg]["all"])}
    model.close()
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
