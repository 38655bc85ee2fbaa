#!/usr/bin/env python3
"""A/B of the weight format of the decode GEMVs on one MI355X (Model.set_weight_format): ms/frame of the bench session (1.7B
synthetic, B rows, 512-token prompts) with bf16, with FP8 on the 16-row tiles ("fp8") and with FP8 on the 4-row tiles as well
("fp8-all"), same process, formats alternating round by round, best and median of the timed runs per format; the bytes a frame
streams under each.   usage: w8_ab.py [--batches 1,2,8] [--frames 256] [--rounds 3] [--formats bf16,fp8,fp8-all]"""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import synth
from common import synthetic_prompt

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="1.7b"); ap.add_argument("--batches", default="1,2,8"); ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--formats", default="bf16,fp8,fp8-all")
a = ap.parse_args()
FORMATS = a.formats.split(",")                       # the first one is the baseline of the percentages
cfg = {"1.7b": q.qwen3_tts_1_7b, "0.6b": q.qwen3_tts_0_6b, "tiny": q.tiny}[a.model]()
model = q.Qwen3TTS.from_synthetic(cfg, device=0, seed=synth.DEFAULT_SEED)
opts = q.SynthesisOptions(max_length=a.frames, eos_token_id=None, seed=42)
for B in [int(b) for b in a.batches.split(",")]:
    utts = [q.Utterance(synthetic_prompt(512, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    ms = {f: [] for f in FORMATS}; mb = {}
    for rnd in range(a.rounds + 1):                  # round 0 warms every format up and is not counted
        for fmt in FORMATS:
            model.set_weight_format(fmt)
            s = model.session(utts, opts); s.prefill()
            t0 = time.perf_counter(); s.generate(a.frames, use_graph=True); dt = time.perf_counter() - t0
            mb[fmt] = s.frame_bytes(512 + a.frames // 2)[0] / 1e6
            s.close()
            if rnd:
                ms[fmt].append(dt * 1e3 / a.frames)
    model.set_weight_format("bf16")
    base = min(ms[FORMATS[0]])
    print(f"B={B:2d}: " + ", ".join(f"{f} {min(ms[f]):.4f} ms/frame (median {statistics.median(ms[f]):.4f}, {mb[f]:.0f} MB of weights per frame"
                                     + (")" if f == FORMATS[0] else f": {100.0 * (min(ms[f]) - base) / base:+.1f} %)") for f in FORMATS)
          + f" ({a.rounds} rounds of {a.frames} frames)", flush=True)
for fmt in FORMATS[1:]:
    model.set_weight_format(fmt)
    print("weights:", model.weight_info())
