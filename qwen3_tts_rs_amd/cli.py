"""`python -m qwen3_tts_rs_amd.cli` — the flag surface of the reference's `generate_audio` binary
(src/bin/generate_audio.rs:30-120, README.md:362-380) on the MI355X engine: synthesize one utterance, write the WAV
(PCM16, audio/io.rs:143-165) and the dump files the reference writes (codes_seed{S}_frames{N}.bin i64 LE,
audio_seed{S}_frames{N}.bin f32 LE, metadata_seed{S}_frames{N}.json; generate_audio.rs:724-813).

`--compare --reference-dir DIR` is the reference's own pin hook (generate_audio.rs:69-75, 549-553, 816-931): EOS is
switched off so that both engines run exactly --frames frames, and this run's codes / PCM are compared with the
codes_seed{S}_frames{N}.bin / audio_seed{S}_frames{N}.bin dumps found in DIR — produced by the reference binary (or its
Python upstream) for the same text, seed and sampling flags. tests/PIN_WITH_REFERENCE.md has the exact commands.

Differences, all explicit: `--synthetic {tiny,0.6b,1.7b}` runs without a checkpoint (seeded random weights — there is
no network here); `--token-ids` / `--instruct-ids` bypass the tokenizer; `--ref-audio` runs the speaker encoder (and, with
`--ref-text`, the speech encoder for ICL) of a Base checkpoint on the GPU — `--xvector-npy` / `--ref-codes-bin` inject
precomputed ones instead."""
import argparse
import json
import os
import sys
import time

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="qwen3_tts_rs_amd.cli", description=__doc__.split("\n\n")[0])
    ap.add_argument("-t", "--text", default="Hello")
    ap.add_argument("-s", "--seed", type=int, default=42)
    ap.add_argument("-f", "--frames", type=int, default=2048, help="max frames (~164 s); generation stops at EOS")
    ap.add_argument("-d", "--duration", type=float, default=None, help="max duration in seconds (overrides --frames): frames = duration * 12.5")
    ap.add_argument("--temperature", type=float, default=0.7)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--repetition-penalty", type=float, default=1.05)
    ap.add_argument("-m", "--model-dir", default="test_data/model")
    ap.add_argument("-o", "--output-dir", default="test_data/rust_audio")
    ap.add_argument("-c", "--compare", action="store_true", help="compare with reference dumps (if they exist); runs exactly --frames frames (no EOS)")
    ap.add_argument("--reference-dir", default="test_data/reference_audio", help="directory holding the reference's codes_/audio_ dumps")
    ap.add_argument("--compare-strict", action="store_true", help="with --compare: exit 1 unless all codes are identical and the PCM is within 1e-3 RMS")
    ap.add_argument("--tokenizer-dir", default=None)
    ap.add_argument("--speaker", default="ryan")
    ap.add_argument("--language", default="english")
    ap.add_argument("--custom-voice", action="store_true", help="accepted for compatibility: the model size always comes from config.json here")
    ap.add_argument("--instruct", default=None, help="voice description (VoiceDesign models)")
    ap.add_argument("--ref-audio", default=None)
    ap.add_argument("--ref-intake", choices=["host", "device"], default="host",
                    help="where --ref-audio is decoded, downmixed and resampled to 24 kHz: on the host (q3_wav_read + q3_resample), or on the "
                         "GPU in one launch (RefAudio.from_wav: PCM 8/16/24/32, float32, G.711; up to 8 channels)")
    ap.add_argument("--ref-text", default=None)
    ap.add_argument("--x-vector-only", action="store_true")
    ap.add_argument("--output", default=None, help="output WAV path (overrides default naming)")
    ap.add_argument("--device", default="auto", help="auto | hip | hip:N | cuda:N (accepted as an alias)")
    # engine-specific
    ap.add_argument("--synthetic", choices=["tiny", "0.6b", "1.7b"], default=None, help="seeded random weights instead of --model-dir")
    ap.add_argument("--token-ids", default=None, help="comma-separated text token ids (bypasses the tokenizer)")
    ap.add_argument("--instruct-ids", default=None, help="comma-separated instruct token ids")
    ap.add_argument("--xvector-npy", default=None, help="speaker embedding [hidden] f32 (.npy) for voice cloning")
    ap.add_argument("--ref-codes-bin", default=None, help="reference codec frames (codes_*.bin) for ICL voice cloning")
    ap.add_argument("--streaming", action="store_true", help="stream chunks (reports time to first audio)")
    ap.add_argument("--output-rate", type=int, default=24000, metavar="HZ",
                    help="with --streaming: the chunks leave through the output stage at this sample rate (8000, 16000, 44100, 48000, ...); "
                         "the WAV header carries it")
    ap.add_argument("--tempo", type=float, default=1.0, metavar="X",
                    help="with --streaming: the speaking rate, 0.5 .. 2.0 (1.25 = 1.25 x as fast), applied by the output stage's time "
                         "stretcher as the chunks leave")
    ap.add_argument("--pitch", type=float, default=0.0, metavar="SEMITONES",
                    help="with --streaming: the pitch, -12 .. +12 semitones, applied by the output stage (varispeed behind the time "
                         "stretcher: the duration stays, formants move with the pitch; +-3 is the useful range for speech)")
    ap.add_argument("--output-format", choices=["f32", "s16", "ulaw", "alaw"], default="f32",
                    help="with --streaming: the format the chunks leave the output stage in; ulaw / alaw (ITU-T G.711, one byte per "
                         "sample) write a G.711 WAV (format tag 7 / 6)")
    ap.add_argument("--gain-db", type=float, default=0.0, metavar="X",
                    help="with --streaming: a gain, -60 .. +24 dB, applied by the output stage in front of its look-ahead peak limiter")
    ap.add_argument("--ceiling-db", type=float, default=0.0, metavar="Y", action=_Given, help="with --streaming: the limiter's ceiling, -24 .. 0 dBFS")
    ap.add_argument("--target-lufs", type=float, default=None, metavar="L",
                    help="with --streaming: steer the audio to this integrated loudness (ITU-R BS.1770-4), -40 .. -5 LUFS, by the output "
                         "stage's causal normaliser; sets a -1 dB ceiling unless --ceiling-db is given, and prints the measured loudness "
                         "and the final gain (the next request's --prior-gain-db)")
    ap.add_argument("--prior-gain-db", type=float, default=0.0, metavar="X",
                    help="with --target-lufs: the gain the first 400 ms leave at, -60 .. +24 dB (the final gain of an earlier request "
                         "with the same voice)")
    ap.add_argument("--trim-silence-db", type=float, default=None, metavar="T",
                    help="with --streaming: cut near-silence by the output stage before anything else touches the audio: 10 ms hops "
                         "whose level is under T dBFS (-90 .. -20, e.g. -50) are dropped at the two ends beyond --edge-ms and inside "
                         "the utterance beyond --max-pause-ms; prints the samples cut at the front, in pauses and at the end")
    ap.add_argument("--edge-ms", type=int, default=50, metavar="MS", action=_Given,
                    help="with --trim-silence-db: the silence kept at the start and at the end, 0 .. 1000 ms in steps of 10")
    ap.add_argument("--max-pause-ms", type=int, default=400, metavar="MS", action=_Given,
                    help="with --trim-silence-db: the longest pause left inside the utterance, 20 .. 2000 ms in steps of 10")
    ap.add_argument("--watermark-key", default=None, metavar="HEX",
                    help="with --streaming: add an inaudible keyed watermark by the output stage (behind the loudness step, in front of "
                         "the limiter); HEX: the 64-bit key, e.g. c0ffee")
    ap.add_argument("--watermark-db", type=float, default=-26.0, metavar="X", action=_Given,
                    help="with --watermark-key: the mark's level re the local signal level, -40 .. -10 dB (default -26)")
    ap.add_argument("--detect-watermark", nargs=2, default=None, metavar=("HEX", "FILE.wav"),
                    help="instead of synthesizing: score FILE.wav for the watermark of key HEX and print the score, the offset and the "
                         "decision; with --ref-intake device the clip is converted and scored on the GPU")
    ap.add_argument("--feed-tokens", type=int, default=0, metavar="N",
                    help="feed the text N tokens at a time through the open-text path, as an LLM would (reports the time from the "
                         "first token to the first audio; writes the same WAV as without the flag)")
    ap.add_argument("--prefix-cache", type=int, default=0, metavar="PAGES",
                    help="keep up to PAGES KV pages (128 positions each) of prefilled --instruct prompts for later requests of this model (0 = off)")
    ap.add_argument("--no-eos", action="store_true", help="disable EOS (fixed-length runs on synthetic weights)")
    ap.add_argument("--tokenize", nargs="+", default=None, metavar="WAV",
                    help="instead of synthesizing: encode these clips with the 12.5 Hz speech tokenizer of --model-dir (or a seeded one with "
                         "--synthetic) — one intake launch (RefAudio.many), one packed encoder pass (SpeechEncoder.encode_refs) — and write "
                         "<output-dir>/<stem>.codes.bin per clip (the codes_*.bin format of --ref-codes-bin)")
    return ap


def tokenize_clips(a, dev: int) -> int:
    """--tokenize: WAV files -> <stem>.codes.bin through RefAudio.many and SpeechEncoder.encode_refs."""
    import qwen3_tts_rs_amd as q
    from qwen3_tts_rs_amd import api
    stems = [os.path.splitext(os.path.basename(p))[0] for p in a.tokenize]
    if len(set(stems)) != len(stems):
        print("error: --tokenize: two clips share a file name; their outputs would overwrite each other", file=sys.stderr)
        return 2
    refs = []
    try:
        if a.synthetic:
            enc = q.SpeechEncoder.from_synthetic(q.tiny_speech_config() if a.synthetic == "tiny" else None, device=dev)
        else:
            tok = os.path.join(a.model_dir, "speech_tokenizer", "model.safetensors")
            if not os.path.exists(tok):
                tok = os.path.join(os.path.dirname(os.path.abspath(a.model_dir)), "speech_tokenizer", "model.safetensors")
            enc = q.SpeechEncoder.from_safetensors(tok, None, dev)
        clips = []
        for p in a.tokenize:
            desc = api.wav_info(p)
            with open(p, "rb") as f:
                raw = f.read()
            clips.append((raw[desc.data_offset:desc.data_offset + desc.data_bytes], desc.sample_rate, desc.fmt, desc.channels))
        refs = api.RefAudio.many(clips, device=dev)
        codes = enc.encode_refs(refs)
    except (api._lib.Q3Error, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    os.makedirs(a.output_dir, exist_ok=True)
    for p, stem, ref, c in zip(a.tokenize, stems, refs, codes):
        out = os.path.join(a.output_dir, stem + ".codes.bin")
        api.save_codes_binary(out, c)
        print(f"Tokenized: {p} ({ref.duration():.2f}s, {ref.source_rate} Hz) -> {out} ({c.shape[0]} frames)")
    for r in refs:
        r.close()
    enc.close()
    return 0


def parse_device(s: str) -> int:
    """parse_device (lib.rs:1875-1926): auto / hip / hip:N; cuda[:N] accepted as an alias; cpu / metal are errors here."""
    s = s.lower()
    if s in ("auto", "hip", "cuda", "gpu"):
        return 0
    for p in ("hip:", "cuda:"):
        if s.startswith(p):
            return int(s[len(p):])
    raise ValueError(f"Unsupported device '{s}': this build runs on MI355X only (auto | hip | hip:N)")


def compare_with_reference(reference_dir: str, seed: int, num_frames: int, codes: np.ndarray, audio: np.ndarray, out=print) -> dict:
    """compare_with_reference (generate_audio.rs:816-931): this run's codes / PCM against the dumps
    codes_seed{seed}_frames{num_frames}.bin (i64 LE, frame-major) and audio_seed{seed}_frames{num_frames}.bin (f32 LE) in
    `reference_dir`. Prints the reference's report lines (first five differing indices, max / mean / RMSE, MATCH / CLOSE /
    DIFFERENT at 1e-5 / 1e-3 of max difference) plus what a parity pin needs: the first differing (frame, group) and the
    north-star verdict (all codec ids identical, PCM within 1e-3 RMS). Returns the numbers."""
    from qwen3_tts_rs_amd import api
    rep = {"codes_found": False, "audio_found": False, "codes_match": None, "first_diff": None, "n_diff": None,
           "max_diff": None, "mean_diff": None, "rmse": None, "status": None, "pinned": None}
    mine = np.ascontiguousarray(codes, dtype=np.uint32).reshape(-1, 16)
    cp = os.path.join(reference_dir, f"codes_seed{seed}_frames{num_frames}.bin")
    if os.path.exists(cp):
        ref = api.load_codes_binary(cp)
        rep["codes_found"] = True
        a, b = ref.reshape(-1).astype(np.int64), mine.reshape(-1).astype(np.int64)
        match = a.size == b.size and bool((a == b).all())
        rep["codes_match"] = match
        if match:
            out(f"Codes: MATCH (all {a.size} values identical)")
            rep["n_diff"] = 0
        else:
            out("Codes: MISMATCH"); out(f"  Reference: {a.size} values"); out(f"  This run:  {b.size} values")
            n = min(a.size, b.size)
            bad = np.nonzero(a[:n] != b[:n])[0]
            for i in bad[:5]:
                out(f"  Index {int(i)} (frame {int(i) // 16}, group {int(i) % 16}): Reference={int(a[i])}, This run={int(b[i])}")
            if bad.size > 5:
                out(f"  ... and {bad.size - 5} more differences")
            out(f"  Total differences: {bad.size}")
            rep["n_diff"] = int(bad.size)
            if bad.size:
                rep["first_diff"] = (int(bad[0]) // 16, int(bad[0]) % 16)
                out(f"  First divergence: frame {rep['first_diff'][0]}, group {rep['first_diff'][1]} "
                    f"(group 0 = talker sample, 1..15 = code-predictor argmax; every later frame depends on it)")
    else:
        out(f"Codes: reference not found at {cp!r}")
    ap = os.path.join(reference_dir, f"audio_seed{seed}_frames{num_frames}.bin")
    if os.path.exists(ap):
        ref = api.load_audio_binary(ap)
        rep["audio_found"] = True
        mine_a = np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
        n = min(ref.size, mine_a.size)
        if n > 0:
            d = np.abs(ref[:n].astype(np.float64) - mine_a[:n].astype(np.float64))
            rep["max_diff"], rep["mean_diff"], rep["rmse"] = float(d.max()), float(d.mean()), float(np.sqrt(np.mean(d * d)))
            rep["status"] = "MATCH" if rep["max_diff"] < 1e-5 else "CLOSE" if rep["max_diff"] < 1e-3 else "DIFFERENT"
            out(f"\nAudio comparison ({n} samples):"); out(f"  Reference samples: {ref.size}"); out(f"  This run samples:  {mine_a.size}")
            out(f"  Max difference: {rep['max_diff']:.6f}"); out(f"  Mean difference: {rep['mean_diff']:.6f}"); out(f"  RMSE: {rep['rmse']:.6f}")
            out(f"  Status: {rep['status']} (max diff " + ("< 1e-5)" if rep["status"] == "MATCH" else "< 1e-3)" if rep["status"] == "CLOSE" else ">= 1e-3)"))
    else:
        out(f"Audio: reference not found at {ap!r}")
    mp = os.path.join(reference_dir, f"metadata_seed{seed}_frames{num_frames}.json")
    if os.path.exists(mp):
        with open(mp) as f:
            out(f"\nReference metadata: {json.load(f)}")
    if rep["codes_found"] and rep["audio_found"] and rep["rmse"] is not None:
        same_len = rep["codes_match"] is True
        rep["pinned"] = bool(same_len and rep["rmse"] <= 1e-3)
        out(f"\nParity (north star: codec ids bit-exact, PCM within 1e-3 RMS): {'PINNED' if rep['pinned'] else 'NOT pinned'}")
    return rep


class _Given(argparse.Action):
    """stores the value and, as <dest>_given, that the flag was on the command line"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values); setattr(namespace, self.dest + "_given", True)


def loudness_from_args(a):
    """(target_mB, prior_mB, ceiling_mB) of --target-lufs / --prior-gain-db / --ceiling-db, or None without --target-lufs;
    ValueError for a combination the CLI refuses (before anything is loaded)."""
    if a.target_lufs is None:
        if a.prior_gain_db != 0.0:
            raise ValueError("--prior-gain-db applies to --target-lufs")
        return None
    if not a.streaming:
        raise ValueError("--target-lufs applies to --streaming (normalise a whole utterance with api.resample_gpu(..., target_mb=))")
    target, prior = int(round(a.target_lufs * 100.0)), int(round(a.prior_gain_db * 100.0))
    if not -4000 <= target <= -500:
        raise ValueError(f"--target-lufs {a.target_lufs} out of range (-40 .. -5)")
    if not -6000 <= prior <= 2400:
        raise ValueError(f"--prior-gain-db {a.prior_gain_db} out of range (-60 .. +24)")
    ceiling = int(round(a.ceiling_db * 100.0)) if getattr(a, "ceiling_db_given", False) else -100
    return target, prior, ceiling


def silence_from_args(a):
    """(threshold_db, edge_ms, pause_ms) of --trim-silence-db / --edge-ms / --max-pause-ms, or None without --trim-silence-db;
    ValueError for a combination the CLI refuses (before anything is loaded)."""
    if a.trim_silence_db is None:
        if getattr(a, "edge_ms_given", False) or getattr(a, "max_pause_ms_given", False):
            raise ValueError("--edge-ms / --max-pause-ms apply to --trim-silence-db")
        return None
    if not a.streaming:
        raise ValueError("--trim-silence-db applies to --streaming (trim a whole utterance with api.trim_silence)")
    if not -90.0 <= a.trim_silence_db <= -20.0:
        raise ValueError(f"--trim-silence-db {a.trim_silence_db} out of range (-90 .. -20)")
    if not 0 <= a.edge_ms <= 1000 or a.edge_ms % 10:
        raise ValueError(f"--edge-ms {a.edge_ms} out of range (0 .. 1000 in steps of 10)")
    if not 20 <= a.max_pause_ms <= 2000 or a.max_pause_ms % 10:
        raise ValueError(f"--max-pause-ms {a.max_pause_ms} out of range (20 .. 2000 in steps of 10)")
    return a.trim_silence_db, a.edge_ms, a.max_pause_ms


def mark_from_args(a):
    """(key, db) of --watermark-key / --watermark-db, or None without --watermark-key; ValueError for a combination the CLI
    refuses (before anything is loaded)."""
    from qwen3_tts_rs_amd import api
    if a.watermark_key is None:
        if getattr(a, "watermark_db_given", False):
            raise ValueError("--watermark-db applies to --watermark-key")
        return None
    if not a.streaming:
        raise ValueError("--watermark-key applies to --streaming (mark a whole utterance with api.mark_embed)")
    try:
        key = api.mark_key(a.watermark_key)
    except ValueError:
        raise ValueError(f"--watermark-key {a.watermark_key!r} is not a 64-bit hexadecimal number")
    if key == 0:
        raise ValueError("--watermark-key 0 is off")
    if not -40.0 <= a.watermark_db <= -10.0:
        raise ValueError(f"--watermark-db {a.watermark_db} out of range (-40 .. -10)")
    return key, a.watermark_db


def detect_watermark(a, dev: int) -> int:
    """--detect-watermark HEX FILE.wav: the score, the offset and the decision."""
    from qwen3_tts_rs_amd import api
    hexkey, path = a.detect_watermark
    try:
        key = api.mark_key(hexkey)
        if a.ref_intake == "device":
            ref = api.RefAudio.from_wav(path, device=dev)
            r = ref.mark_score(key); dur = ref.duration(); ref.close()
        else:
            clip = api.AudioBuffer.load(path)
            if clip.sample_rate != 24000:
                clip = api.resample(clip, 24000)
            r = api.mark_detect(clip, key); dur = clip.duration()
    except (api._lib.Q3Error, OSError, ValueError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    print(f"Watermark: score {r.score:.2f} (threshold {api.MARK_SCORE_DETECT:.2f}), offset {r.offset}, {dur:.2f}s scored on the "
          f"{'device' if a.ref_intake == 'device' else 'host'}: {'DETECTED' if r.detected else 'not detected'}")
    return 0


def max_frames_from_args(a) -> int:
    return int(a.duration * 12.5) if a.duration is not None else a.frames


def feed_tokens(model, utt, opts, ids, n_feed):
    """The text through the open-text path n_feed tokens at a time, frames generated between the pieces as far as
    the text allows: (samples, codes, ms from the first token to the first chunk's audio). The codes are those of the whole-text
    run, and the samples its whole-utterance decode."""
    import dataclasses
    t0 = time.time(); ttfa = None
    chunk = opts.chunk_frames if opts.chunk_frames > 0 else 10
    s = model.session([dataclasses.replace(utt, text_ids=list(ids[:n_feed]))], opts)
    try:
        s.open_text(0); s.prefill()
        pos, closed = n_feed, False
        while True:
            if pos < len(ids):
                s.append_text(0, ids[pos:pos + n_feed]); pos += n_feed
            elif not closed:
                s.append_text(0, [], last=True); closed = True
            s.generate(opts.max_length)                 # as many frames as the text received so far allows
            n, done = s.frames(0)
            if ttfa is None and n > 0 and (n >= chunk or done):
                s.decode(0, 0, min(n, chunk))
                ttfa = (time.time() - t0) * 1000.0
            if done:
                break
        return s.decode(0), s.codes(0), (ttfa if ttfa is not None else (time.time() - t0) * 1000.0)
    finally:
        s.close()


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    import qwen3_tts_rs_amd as q
    from qwen3_tts_rs_amd import api
    from qwen3_tts_rs_amd.text import TextTokenizer
    # flag validation of generate_audio.rs:163-210
    if a.instruct and a.ref_audio:
        print("error: --instruct and --ref-audio are mutually exclusive.\n  --instruct is for VoiceDesign models (text-described voices).\n"
              "  --ref-audio is for Base models (voice cloning from reference audio).", file=sys.stderr)
        return 2
    if a.ref_text and not (a.ref_audio or a.xvector_npy):
        print("error: --ref-text requires --ref-audio (reference text is the transcript of the reference audio for ICL voice cloning)", file=sys.stderr)
        return 2
    if a.x_vector_only and not (a.ref_audio or a.xvector_npy):
        print("error: --x-vector-only requires --ref-audio (x_vector_only is a voice cloning mode)", file=sys.stderr)
        return 2
    if a.x_vector_only and a.ref_text:
        print("error: --x-vector-only and --ref-text are contradictory.\n  x_vector_only uses only the speaker embedding (no ICL).", file=sys.stderr)
        return 2
    try:
        loud = loudness_from_args(a)
        sil = silence_from_args(a)
        mark = mark_from_args(a)
    except ValueError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    dev = parse_device(a.device)
    if a.detect_watermark:
        return detect_watermark(a, dev)
    if a.tokenize:
        return tokenize_clips(a, dev)
    speaker, language = q.Speaker.from_str(a.speaker), q.Language.from_str(a.language)
    frames = max_frames_from_args(a)
    t0 = time.time()
    if a.synthetic:
        cfg = {"tiny": q.tiny, "0.6b": q.qwen3_tts_0_6b, "1.7b": q.qwen3_tts_1_7b}[a.synthetic]()
        model = q.Qwen3TTS.from_synthetic(cfg, device=dev)
        if a.ref_audio:      # a Base-style synthetic model: seeded ECAPA-TDNN of the matching embedding width
            scfg = q.tiny_speaker_config(cfg.hidden) if a.synthetic == "tiny" else q.SpeakerEncoderConfig(enc_dim=cfg.hidden)
            model.attach_speaker_encoder(q.SpeakerEncoder.from_synthetic(scfg, device=dev))
            if a.ref_text and not a.ref_codes_bin:      # ICL from raw audio: seeded speech encoder (Mimi shapes)
                model.attach_speech_encoder(q.SpeechEncoder.from_synthetic(None, device=dev))     # 16 codebooks, whatever the talker's size
        tok = TextTokenizer.from_pretrained(None, a.tokenizer_dir, allow_stand_in=True)     # --synthetic: the labelled stand-in
    else:
        # a real checkpoint needs its real tokenizer (the reference fails to load without one, text.rs:62-110) unless every
        # piece of text arrives as ids
        need_text = not a.token_ids or (a.instruct and not a.instruct_ids) or bool(a.ref_text)
        try:
            tok = TextTokenizer.from_pretrained(a.model_dir, a.tokenizer_dir)
        except FileNotFoundError as e:
            if need_text:
                print(f"error: {e}", file=sys.stderr)
                return 2
            tok = None
        model = q.Qwen3TTS.from_pretrained(a.model_dir, device=dev)
    print(f"Loaded model in {time.time() - t0:.2f}s ({model.config.name}, type {model.model_type.name if model.model_type else 'unknown'}, "
          f"tokenizer: {tok.kind if tok else 'none (--token-ids)'})")
    if a.prefix_cache > 0:
        model.prefix_cache(a.prefix_cache)
    ids = [int(x) for x in a.token_ids.split(",")] if a.token_ids else tok.encode(a.text)
    opts = q.SynthesisOptions(max_length=frames, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p,
                              repetition_penalty=a.repetition_penalty, seed=a.seed)
    if a.no_eos or a.compare:          # --compare: don't stop early when comparing with the reference (generate_audio.rs:549-553)
        opts.eos_token_id = None
    utt = q.Utterance(ids, speaker, language, seed=a.seed)
    if a.instruct or a.instruct_ids:
        utt.instruct_ids = [int(x) for x in a.instruct_ids.split(",")] if a.instruct_ids else tok.encode(a.instruct)
    if a.ref_audio:          # run_voice_clone (generate_audio.rs:213-300): speaker embedding from the reference WAV
        if a.ref_intake == "device":      # decode, downmix and resampling on the GPU, the samples stay there
            try:
                ref = api.RefAudio.from_wav(a.ref_audio, device=dev)
            except api._lib.Q3Error as e:
                print(f"error: {e}", file=sys.stderr)
                return 2
            print(f"Reference audio: {a.ref_audio} ({ref.duration():.2f}s, {ref.source_rate} Hz, {ref.source_format}, "
                  f"{ref.source_channels} ch)")
        else:
            ref = api.AudioBuffer.load(a.ref_audio)
            print(f"Reference audio: {a.ref_audio} ({ref.duration():.2f}s, {ref.sample_rate} Hz)")
        print("Mode: ICL (reference codes + text)" if a.ref_text else "Mode: x_vector_only (no reference text)")
        try:
            if a.ref_text and not a.ref_codes_bin and not a.x_vector_only:
                # ICL from raw audio: speaker embedding + codec frames of the reference clip (lib.rs:1132-1190)
                prompt = model.create_voice_clone_prompt(ref, ref_text_ids=tok.encode(a.ref_text))
                utt.xvector, utt.ref_codes, utt.ref_text_ids = prompt.speaker_embedding, prompt.ref_codes, prompt.ref_text_ids
            else:
                utt.xvector = model.create_voice_clone_prompt(ref).speaker_embedding
        except api._lib.Q3Error as e:
            print(f"error: {e}", file=sys.stderr)
            return 2
    elif a.xvector_npy:
        utt.xvector = np.load(a.xvector_npy).astype(np.float32).reshape(-1)
    if utt.xvector is not None:
        if a.ref_codes_bin and not a.x_vector_only:
            utt.ref_codes = api.load_codes_binary(a.ref_codes_bin)
            utt.ref_text_ids = tok.encode(a.ref_text or "")
    print(f"Generating up to {frames} frames...")
    t1 = time.time(); ttfa = None
    out_rate = 24000; g711 = None
    if a.output_rate != 24000 and not a.streaming:
        print("error: --output-rate applies to --streaming (resample a whole utterance with api.resample_gpu)", file=sys.stderr)
        return 2
    tempo = int(round(a.tempo * 1000.0))
    if tempo != 1000 and not a.streaming:
        print("error: --tempo applies to --streaming (stretch a whole utterance with api.resample_gpu(..., tempo_permille=))", file=sys.stderr)
        return 2
    cents = int(round(a.pitch * 100.0))
    if cents != 0 and not a.streaming:
        print("error: --pitch applies to --streaming (shift a whole utterance with api.resample_gpu(..., pitch_cents=))", file=sys.stderr)
        return 2
    gain_mb, ceiling_mb = int(round(a.gain_db * 100.0)), int(round(a.ceiling_db * 100.0))
    if loud is not None:
        ceiling_mb = loud[2]
    reading = None; cuts = None
    if (a.output_format != "f32" or gain_mb or ceiling_mb) and not a.streaming:
        print("error: --output-format / --gain-db / --ceiling-db apply to --streaming (convert a whole utterance with "
              "api.resample_gpu(..., fmt=, gain_mb=, ceiling_mb=))", file=sys.stderr)
        return 2
    if a.streaming and (a.output_rate != 24000 or tempo != 1000 or cents != 0 or a.output_format != "f32" or gain_mb or ceiling_mb or loud is not None or sil is not None or mark is not None):
        # the chunks of the streaming session, each through the session's output stage as it leaves
        s = model.session([utt], opts)
        try:
            s.set_output(a.output_rate, fmt=a.output_format)
            if tempo != 1000:
                s.set_tempo(tempo)
            if cents != 0:
                s.set_pitch(cents)
            if gain_mb or ceiling_mb:
                s.set_level(gain_mb, ceiling_mb)
            if loud is not None:
                s.set_loudness(api.LOUD_NORMALIZE, loud[0], loud[1])
            if sil is not None:
                s.set_silence(*sil)
            if mark is not None:
                s.set_mark(*mark)
        except api._lib.Q3Error as e:
            print(f"error: {e}", file=sys.stderr)
            return 2
        chunks, done = [], False
        while not done:
            c, done = s.next_chunks_out()[0]
            if c is not None:
                if ttfa is None:
                    ttfa = (time.time() - t1) * 1000.0
                chunks.append(c.samples)
        samples = np.concatenate(chunks) if chunks else np.zeros(0, api.PCM_DTYPE[api.PCM_NAMES.index(a.output_format)])
        if loud is not None:
            reading = s.loudness(0)
        if sil is not None:
            cuts = s.silence(0)
        codes = s.codes(0); s.close()
        timing = None; out_rate = a.output_rate
        if a.output_format in ("ulaw", "alaw"):
            g711 = samples; samples = np.zeros(0, np.float32)
        elif a.output_format == "s16":
            samples = samples.astype(np.float32) / np.float32(32767.0)
    elif a.streaming:
        ss = api.StreamingSession(model, utt, opts)
        chunks = []
        for c in ss:
            if ttfa is None:
                ttfa = (time.time() - t1) * 1000.0
            chunks.append(c.samples)
        samples = np.concatenate(chunks) if chunks else np.zeros(0, np.float32)
        codes = ss._s.codes(0); ss._s.close()
        timing = None
    elif a.feed_tokens > 0:
        samples, codes, ttfa = feed_tokens(model, utt, opts, ids, a.feed_tokens)
        timing = None
        print(f"Fed {len(ids)} tokens {a.feed_tokens} at a time: first token to first audio {ttfa:.1f} ms")
    else:
        s = model.session([utt], opts)
        audio, timing = s.run()
        samples, codes = audio[0].samples, s.codes(0); s.close()
    wall = time.time() - t1
    n = int(codes.shape[0])
    audio = api.AudioBuffer(samples if g711 is None else np.zeros(g711.size, np.float32), out_rate)      # (G.711: the length alone)
    print(f"Generated: {audio.duration():.2f}s, {len(audio)} samples, {n} frames in {wall * 1e3:.0f} ms (RTF {wall / max(audio.duration(), 1e-9):.3f})"
          + (f", TTFA {ttfa:.1f} ms" if ttfa is not None else ""))
    if reading is not None:
        print(f"Loudness: {reading.lufs:.2f} LUFS measured over {reading.gated} of {reading.blocks} blocks (target {a.target_lufs:.2f}), "
              f"final gain {reading.gain_db:+.2f} dB (--prior-gain-db {reading.gain_db:.2f} for the next request of this voice)")
    if cuts is not None:
        print(f"Silence: {cuts.lead_cut} samples cut at the front, {cuts.pause_cut} in pauses, {cuts.trail_cut} at the end "
              f"({cuts.n_out} of {cuts.n_in} samples at 24 kHz kept; under {a.trim_silence_db:.1f} dBFS, edges {a.edge_ms} ms, pauses {a.max_pause_ms} ms)")
    if mark is not None:
        print(f"Watermark: key {mark[0]:x} at {mark[1]:.1f} dB re the local level")
    os.makedirs(a.output_dir, exist_ok=True)
    wav = a.output or os.path.join(a.output_dir, f"audio_seed{a.seed}_frames{n}.wav")
    if g711 is not None:
        api.save_wav_g711(wav, g711, out_rate, a.output_format)
    else:
        audio.save(wav)
    api.save_codes_binary(os.path.join(a.output_dir, f"codes_seed{a.seed}_frames{n}.bin"), codes)
    if g711 is None:                                  # (the dump is f32: a G.711 run leaves its WAV)
        api.save_audio_binary(os.path.join(a.output_dir, f"audio_seed{a.seed}_frames{n}.bin"), samples)
    meta = {"text": a.text, "seed": a.seed, "num_frames": n, "temperature": a.temperature, "top_k": a.top_k, "top_p": a.top_p,
            "input_ids": ids, "codes_shape": [n, 16], "audio_samples": int(len(audio)), "sample_rate": out_rate}
    with open(os.path.join(a.output_dir, f"metadata_seed{a.seed}_frames{n}.json"), "w") as f:
        json.dump(meta, f, indent=2)
    print(f"Saved WAV to: {wav}")
    if timing is not None:
        print(f"Stages: prefill {timing.prefill_ms:.1f} ms, generation {timing.generation_ms:.1f} ms ({timing.generation_frames} frames), decode {timing.decode_ms:.1f} ms")
    model.close()
    if a.compare:
        print("\n=== Comparing with reference ===")
        rep = compare_with_reference(a.reference_dir, a.seed, n, codes, samples)
        if a.compare_strict and not rep["pinned"]:
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
