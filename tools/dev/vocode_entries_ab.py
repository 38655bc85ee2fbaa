"""One sha256 per (entry, row) of every entry that turns a row's frames into samples, at 1.7B synthetic width with the full-size
codec: the listing of a build. Two builds vocode alike when their listings are equal line for line (profiles/vocode_range_ab.txt).
  run          8 rows x 160 frames, EOS off: q3_session_run serial (Q3_DECODE_OVERLAP=0) and overlapped (=1, 64-frame segments)
  rows         3 CustomVoice rows that end at frames 40 / 27 / 33, chunk 10, EOS on: run serial / overlapped / one row, decode, decode pieces,
               decode_codes, the chunks of both stream modes (next_chunk_row, and next_chunk with read-ahead), a batcher ticket
  icl          one ICL row: decode, run, a batcher ticket, the cancel of a parked ticket
Uses only entries both builds have, so the same file runs from either tree."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import qwen3_tts_rs_amd as q                       # noqa: E402
from qwen3_tts_rs_amd import synth, _lib           # noqa: E402
from qwen3_tts_rs_amd.synth import synthetic_prompt      # noqa: E402

KNOBS = ("Q3_DECODE_OVERLAP", "Q3_DECODE_SEG", "Q3_DECODE_TAIL", "Q3_DECODE_RESIDENT")


def line(entry, row, a):
    a = np.ascontiguousarray(a)
    print(f"{entry:<34} row {row}  {a.size:>8}  {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def run(model, utts, opts, **env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    s = model.session(utts, opts)
    audio, _ = s.run()
    s.close()
    return [a.samples for a in audio]


def chunks(s, b, one_row=False):
    parts = []
    for _ in range(64):
        a, done = s.next_chunk() if one_row else s.next_chunk_row(b)
        if a is not None:
            parts.append(a.samples)
        if done:
            return np.concatenate(parts)
    raise RuntimeError("the row did not finish")


def main():
    model = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    wide = [q.Utterance(synthetic_prompt(32, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(8)]
    o160 = q.SynthesisOptions(max_length=160, eos_token_id=None, seed=42)
    for name, env in (("run serial 8x160", dict(Q3_DECODE_OVERLAP=0)), ("run overlapped 8x160", dict(Q3_DECODE_OVERLAP=1, Q3_DECODE_SEG=64, Q3_DECODE_TAIL=32))):
        for b, a in enumerate(run(model, wide, o160, **env)):
            line(name, b, a)

    utts = [q.Utterance(synthetic_prompt(4 + i, i), q.Speaker.Ryan, q.Language.English, seed=42 + i, max_length=(40, 27, 33)[i]) for i in range(3)]
    opts = q.SynthesisOptions(max_length=40, temperature=1.3, top_k=0, top_p=1.0, seed=11, min_new_tokens=2, chunk_frames=10)
    for name, env in (("run serial", dict(Q3_DECODE_OVERLAP=0)), ("run overlapped seg16", dict(Q3_DECODE_OVERLAP=1, Q3_DECODE_SEG=16, Q3_DECODE_TAIL=16)), ("run default", {})):
        for b, a in enumerate(run(model, utts, opts, **env)):
            line(name, b, a)
    for b, u in enumerate(utts):
        line("run one row", b, run(model, [u], opts)[0])
    for mode in (1, 0):
        s = model.session(utts, opts)
        _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, mode))
        s.prefill(); s.generate(40)
        for b in range(3):
            c = s.codes(b); n = len(c)
            if mode == 1:
                line("codes", b, c)
                line("decode", b, s.decode(b))
                for f0, f1 in ((0, min(7, n)), (min(3, n - 1), n), (max(n - 13, 0), n)):
                    line(f"decode [{f0}, {f1})", b, s.decode(b, f0, f1))
                line("decode_codes", b, model.decode_codes(c).samples)
            line(f"next_chunk_row mode {mode}", b, chunks(s, b))
        s.close()
        for b, u in enumerate(utts):
            s = model.session([u], opts)
            _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, mode))
            line(f"next_chunk mode {mode}", b, chunks(s, 0, one_row=True))
            s.close()
    bat = q.Batcher(model, slots=3, frame_budget=40, prompt_budget=32, options=opts)
    for b, (_c, p) in enumerate(bat.run_all(utts, want_pcm=True, poll_frames=8)):
        line("batcher ticket", b, p)
    bat.close()

    rng = np.random.default_rng(5)
    icl = q.Utterance(synthetic_prompt(11, 4), language=q.Language.French, xvector=rng.standard_normal(model.config.hidden).astype(np.float32),
                      ref_codes=rng.integers(0, 2048, size=(5, 16)).astype(np.uint32), ref_text_ids=synthetic_prompt(3, 94), seed=46, max_length=16)
    host = q.SynthesisOptions(max_length=20, eos_token_id=None, seed=1)
    s = model.session([icl], host)
    s.prefill(); s.generate(20)
    line("icl codes", 0, s.codes(0)); line("icl decode", 0, s.decode(0))
    s.close()
    line("icl run", 0, run(model, [icl], host)[0])
    bat = q.Batcher(model, slots=1, frame_budget=40, prompt_budget=48, options=host, max_parked=1)
    line("icl batcher ticket", 0, bat.run_all([icl], want_pcm=True, poll_frames=8)[0][1])
    t = bat.submit(icl, want_pcm=True)
    bat.step(4); bat.park(t); bat.cancel(t)
    c, p = bat.fetch(t)
    line(f"icl cancel of parked ({len(c)} frames)", 0, p)
    bat.close()
    model.close()


if __name__ == "__main__":
    main()
