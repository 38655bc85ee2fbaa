#!/usr/bin/env python3
"""A/B of the talker K/V dtype on one MI355X, same process, dtypes alternating: f32 / bf16 / fp8 (KV8) sessions on the
synthetic model — ms per frame at B = 64 with the bench prompts and at B = 1 and B = 8 behind a 4096-position prompt — and, for
one greedy row, the share of the first 64 frames whose code 0 equals the f32 session's.
usage: kv8_ab.py [--model 1.7b] [--frames 128] [--rounds 3]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import synth
from common import synthetic_prompt

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="1.7b"); ap.add_argument("--frames", type=int, default=128); ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
cfg = {"1.7b": q.qwen3_tts_1_7b, "0.6b": q.qwen3_tts_0_6b, "tiny": q.tiny}[a.model]()
model = q.Qwen3TTS.from_synthetic(cfg, device=0, seed=synth.DEFAULT_SEED)
DTYPES = ("f32", "bf16", "fp8")
bench = lambda B: [q.Utterance(synthetic_prompt(512, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
deep = lambda B: [q.Utterance(synthetic_prompt(64, i), language=q.Language.English, instruct_ids=synthetic_prompt(4096, 5000 + i), seed=42 + i) for i in range(B)]
CASES = [("B=64 bench prompts", bench(64)), ("B=1 behind 4096 positions", deep(1)), ("B=8 behind 4096 positions", deep(8))]


def run(utts, dtype, frames, opts):
    s = model.session(utts, opts, kv_dtype=dtype); s.prefill()
    t0 = time.perf_counter(); s.generate(frames, use_graph=True); dt = time.perf_counter() - t0      # (generate ends in a device synchronise)
    c0 = s.codes(0)[:, 0].copy(); kvb = s.frame_bytes(4096)[1]; s.close()
    return dt * 1e3 / frames, c0, kvb


for name, utts in CASES:
    opts = q.SynthesisOptions(max_length=a.frames, eos_token_id=None, seed=42)
    best = {d: 1e9 for d in DTYPES}; kvb = {}
    for d in DTYPES:
        run(utts, d, 8, opts)                               # warm: capture, session-shape cache, the pools' first slabs
    for rnd in range(a.rounds):
        for d in DTYPES:
            ms, _, kvb[d] = run(utts, d, a.frames, opts)
            best[d] = min(best[d], ms)
    print(f"{name}: " + ", ".join(f"{d} {best[d]:.4f} ms/frame" for d in DTYPES) +
          f"  (best of {a.rounds}, {a.frames} frames; K/V bytes per frame at 4096 positions: " + ", ".join(f"{d} {kvb[d] / 1e6:.1f} MB" for d in DTYPES) + ")", flush=True)
greedy = q.SynthesisOptions(max_length=64, eos_token_id=None, seed=42, temperature=0.0)
codes = {d: run(bench(1), d, 64, greedy)[1] for d in DTYPES}
for d in DTYPES[1:]:
    print(f"greedy row, first 64 frames: code 0 of the {d} session equals the f32 session's in {100.0 * (codes[d] == codes['f32']).mean():.1f} % of the frames")
print("pool:", model.kv_pool_info())
