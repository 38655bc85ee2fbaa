#!/usr/bin/env python3
"""A/B of the weight format of the decode GEMVs on one MI355X (Model.set_weight_format): ms/frame of the bench session (1.7B
synthetic, B rows, 512-token prompts) with bf16 and with FP8 weights, same process, formats alternating round by round, best and
median of the timed runs per format; the bytes a frame streams under each.   usage: w8_ab.py [--batches 1,8,16] [--frames 256] [--rounds 3]"""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import synth
from common import synthetic_prompt

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="1.7b"); ap.add_argument("--batches", default="1,8,16"); ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
cfg = {"1.7b": q.qwen3_tts_1_7b, "0.6b": q.qwen3_tts_0_6b, "tiny": q.tiny}[a.model]()
model = q.Qwen3TTS.from_synthetic(cfg, device=0, seed=synth.DEFAULT_SEED)
opts = q.SynthesisOptions(max_length=a.frames, eos_token_id=None, seed=42)
for B in [int(b) for b in a.batches.split(",")]:
    utts = [q.Utterance(synthetic_prompt(512, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    ms = {"bf16": [], "fp8": []}; mb = {}
    for rnd in range(a.rounds + 1):                  # round 0 warms both formats up and is not counted
        for fmt in ("bf16", "fp8"):
            model.set_weight_format(fmt)
            s = model.session(utts, opts); s.prefill()
            t0 = time.perf_counter(); s.generate(a.frames, use_graph=True); dt = time.perf_counter() - t0
            mb[fmt] = s.frame_bytes(512 + a.frames // 2)[0] / 1e6
            s.close()
            if rnd:
                ms[fmt].append(dt * 1e3 / a.frames)
    model.set_weight_format("bf16")
    b, f = min(ms["bf16"]), min(ms["fp8"])
    print(f"B={B:2d}: bf16 {b:.4f} ms/frame (median {statistics.median(ms['bf16']):.4f}, {mb['bf16']:.0f} MB of weights per frame), "
          f"fp8 {f:.4f} (median {statistics.median(ms['fp8']):.4f}, {mb['fp8']:.0f} MB): {100.0 * (f - b) / b:+.1f} % ({a.rounds} rounds of {a.frames} frames)", flush=True)
model.set_weight_format("fp8")
print("weights:", model.weight_info())
