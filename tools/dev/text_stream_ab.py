"""Streaming text input at 1.7B, synthetic weights: (1) time from the first text token to the first audio chunk of an
open-text session, against today's time to first audio (the whole 512-token text first); (2) ms per frame of sessions whose rows
are open (text not closed: the frame's glue kernels take their hold-aware paths) against closed ones, B = 1 and B = 8.
Prints one JSON object; `--json PATH` also writes it to PATH."""
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

REPS, PROMPT, CHUNK = 5, 512, 10


def ms_per_frame(model, B, open_rows, frames=128, warm=16):
    utts = [q.Utterance(synthetic_prompt(PROMPT, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(B)]
    opts = q.SynthesisOptions(max_length=frames + warm, eos_token_id=None, seed=42)
    if open_rows:        # first token at creation, the rest appended before the prefill, the text left open
        first = [q.Utterance(list(u.text_ids)[:1], u.speaker, u.language, seed=u.seed) for u in utts]
        s = model.session(first, opts)
        for b, u in enumerate(utts):
            s.open_text(b); s.append_text(b, list(u.text_ids)[1:])
    else:
        s = model.session(utts, opts)
    s.prefill(); s.generate(warm)
    t = time.perf_counter(); s.generate(frames); el = time.perf_counter() - t
    codes = [s.codes(b) for b in range(B)]
    s.close()
    return el * 1000.0 / frames, codes


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args()
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    ids = list(synthetic_prompt(PROMPT, 0))
    opts = q.SynthesisOptions(max_length=30, eos_token_id=None, seed=42, chunk_frames=CHUNK)
    closed, opened = [], []
    for _ in range(REPS + 1):
        t = time.perf_counter()
        ss = model.synthesize_streaming(ids, q.Speaker.Ryan, q.Language.English, opts)
        ss.next_chunk(); closed.append((time.perf_counter() - t) * 1000.0); ss._s.close()
        t = time.perf_counter()
        ts = model.synthesize_streaming_text(ids[:1], q.Speaker.Ryan, q.Language.English, opts)
        ts.push(ids[1:CHUNK + 1])                # the tokens the first chunk needs, as soon as they exist
        c = ts.next_chunk(); opened.append((time.perf_counter() - t) * 1000.0); ts.close()
        assert c is not None
    out = {"ttfa_ms_p50_whole_text": float(np.median(closed[1:])), "first_token_to_audio_ms_p50": float(np.median(opened[1:])),
           "prompt_tokens": PROMPT, "chunk_frames": CHUNK}
    for B in (1, 8):
        mc, cc = ms_per_frame(model, B, False)
        mo, co = ms_per_frame(model, B, True)
        out[f"b{B}_ms_per_frame_closed"] = mc
        out[f"b{B}_ms_per_frame_open"] = mo
        out[f"b{B}_frames"] = 128
    model.close()
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
