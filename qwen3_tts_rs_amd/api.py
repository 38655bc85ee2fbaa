"""Python mirror of the reference's public API over the C ABI (include/q3tts.h).

Names, argument meaning and error behaviour follow the reference crate's re-exports
(src/lib.rs:107-117): `Qwen3TTS`, `SynthesisOptions`, `SynthesisTiming`, `StreamingSession`,
`AudioBuffer`, `Speaker`, `Language`, `CODEC_EOS_TOKEN_ID`, `SAMPLES_PER_FRAME`. Differences:
text arrives as token ids (the tokenizer, src/tokenizer/text.rs, is outside the hot path) and the
synthesis calls accept a LIST of utterances, which run as one batch on the GPU (the reference is
batch 1; each sequence behaves exactly like its own batch-1 run).
"""
import ctypes
import enum
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import lib, check, COptions, CRequest, CTiming
from .config import Q3Config
from . import synth

# the keyed watermark of the output stage
MARK_DB_DEFAULT = -26.0                                  # Q3_MARK_STRENGTH_DEFAULT
MARK_SCORE_DETECT = float(lib.q3_mark_score_detect())    # Q3_MARK_SCORE_DETECT: a clip carries the key's mark from this score on

MAX_BATCH = 64                 # Q3_MAX_BATCH (include/q3tts.h): sequences per session
CODEC_EOS_TOKEN_ID = 2150      # lib.rs:1466
SAMPLES_PER_FRAME = 1920       # lib.rs:1469


class Language(enum.Enum):     # talker.rs:59-108
    Chinese = 2055
    English = 2050
    Japanese = 2058
    Korean = 2064
    German = 2053
    French = 2061
    Russian = 2069
    Portuguese = 2071
    Spanish = 2054
    Italian = 2070

    def token_id(self) -> int:
        return self.value

    @staticmethod
    def from_str(s: str) -> "Language":
        table = {"english": "English", "en": "English", "chinese": "Chinese", "zh": "Chinese", "japanese": "Japanese",
                 "ja": "Japanese", "korean": "Korean", "ko": "Korean", "german": "German", "de": "German",
                 "french": "French", "fr": "French", "russian": "Russian", "ru": "Russian", "portuguese": "Portuguese",
                 "pt": "Portuguese", "spanish": "Spanish", "es": "Spanish", "italian": "Italian", "it": "Italian"}
        k = s.lower()
        if k not in table:
            raise ValueError(f"Unknown language: {s}")
        return Language[table[k]]


class Speaker(enum.Enum):      # talker.rs:111-157
    Serena = 3066
    Vivian = 3065
    UncleFu = 3010
    Ryan = 3061
    Aiden = 2861
    OnoAnna = 2873
    Sohee = 2864
    Eric = 2875
    Dylan = 2878

    def token_id(self) -> int:
        return self.value

    def native_language(self) -> Language:
        if self in (Speaker.Ryan, Speaker.Aiden):
            return Language.English
        if self is Speaker.OnoAnna:
            return Language.Japanese
        if self is Speaker.Sohee:
            return Language.Korean
        return Language.Chinese

    @staticmethod
    def from_str(s: str) -> "Speaker":
        table = {"ryan": "Ryan", "serena": "Serena", "vivian": "Vivian", "aiden": "Aiden", "uncle_fu": "UncleFu",
                 "unclefu": "UncleFu", "ono_anna": "OnoAnna", "onoanna": "OnoAnna", "sohee": "Sohee", "eric": "Eric",
                 "dylan": "Dylan"}
        k = s.lower()
        if k not in table:
            raise ValueError(f"Unknown speaker: {s}")
        return Speaker[table[k]]


@dataclass
class SynthesisOptions:        # lib.rs:1786-1836
    max_length: int = 2048
    temperature: float = 0.9
    top_k: int = 50
    top_p: float = 0.9
    repetition_penalty: float = 1.05
    eos_token_id: Optional[int] = CODEC_EOS_TOKEN_ID
    chunk_frames: int = 10
    min_new_tokens: int = 2
    seed: Optional[int] = None

    def to_c(self) -> COptions:
        o = COptions()
        o.temperature = float(self.temperature); o.top_p = float(self.top_p)
        o.repetition_penalty = float(self.repetition_penalty)
        o.seed = 0 if self.seed is None else int(self.seed)
        o.max_length = int(self.max_length); o.top_k = int(self.top_k)
        o.eos_token_id = -1 if self.eos_token_id is None else int(self.eos_token_id)
        o.chunk_frames = int(self.chunk_frames); o.min_new_tokens = int(self.min_new_tokens)
        o.has_seed = 0 if self.seed is None else 1
        return o


@dataclass
class SynthesisTiming:         # lib.rs:138-147
    prefill_ms: float
    generation_ms: float
    generation_frames: int
    decode_ms: float


@dataclass
class AudioBuffer:             # audio/io.rs:28-34
    samples: np.ndarray
    sample_rate: int = 24000

    def __len__(self) -> int:
        return int(self.samples.shape[0])

    def duration(self) -> float:
        return len(self) / float(self.sample_rate)

    def save(self, path: str):                       # AudioBuffer::save → save_wav (audio/io.rs:143-165)
        save_wav(path, self.samples, self.sample_rate)

    @classmethod
    def load(cls, path: str) -> "AudioBuffer":       # AudioBuffer::load → load_wav (audio/io.rs:106-141)
        return load_wav(path)


@dataclass
class Utterance:
    """One request: token ids + conditioning (the argument lists of lib.rs:718-724 / 802-808)."""
    text_ids: Sequence[int]
    speaker: Speaker = Speaker.Ryan
    language: Language = Language.English
    instruct_ids: Optional[Sequence[int]] = None     # voice design
    xvector: Optional[np.ndarray] = None             # voice clone: speaker embedding (x-vector)
    ref_codes: Optional[np.ndarray] = None           # ICL voice clone: reference codec frames [n_ref][16]
    ref_text_ids: Optional[Sequence[int]] = None     # ICL voice clone: reference transcript token ids
    seed: Optional[int] = None                       # overrides options.seed for this sequence
    max_length: Optional[int] = None                 # overrides options.max_length for this sequence (rows of a session end at their own limit)
    options: Optional["SynthesisOptions"] = None     # this sequence's own sampling options (SynthesisOptions is per call in the reference); default: the session's

    def mode(self) -> int:
        if self.instruct_ids is not None:
            return 2
        if self.xvector is not None:
            return 1
        return 0


def fill_request(r, u: "Utterance", options: "SynthesisOptions", keep: list):
    """q3_request of one utterance; the arrays it points to are appended to `keep` (the caller keeps them alive)"""
    r.mode = u.mode()
    t = np.ascontiguousarray(u.text_ids, dtype=np.uint32); keep.append(t)
    r.text_ids = t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)); r.n_text = len(t)
    if u.instruct_ids is not None:
        ins = np.ascontiguousarray(u.instruct_ids, dtype=np.uint32); keep.append(ins)
        r.instruct_ids = ins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)); r.n_instruct = len(ins)
    r.speaker_id = u.speaker.token_id(); r.language_id = u.language.token_id()
    if u.xvector is not None:
        xv = np.ascontiguousarray(u.xvector, dtype=np.float32); keep.append(xv)
        r.xvector = xv.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    if u.ref_codes is not None:          # prepended at decode even without a transcript (lib.rs:1022); ICL needs both
        rc = np.ascontiguousarray(u.ref_codes, dtype=np.uint32).reshape(-1, 16); keep.append(rc)
        r.ref_codes = rc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)); r.n_ref = rc.shape[0]
        if u.ref_text_ids is not None:
            rt = np.ascontiguousarray(u.ref_text_ids, dtype=np.uint32); keep.append(rt)
            r.ref_text_ids = rt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)); r.n_ref_text = len(rt)
    o = (u.options or options).to_c()
    o.chunk_frames = options.chunk_frames           # the streaming chunk is a property of the session
    if u.seed is not None:
        o.seed = int(u.seed); o.has_seed = 1
    if u.max_length is not None:
        o.max_length = int(u.max_length)
    r.opts = o


class Session:
    """A batch of utterances on one GPU (q3_session). Owns KV pages, RNG streams, penalty masks."""

    def __init__(self, model: "Qwen3TTS", utts: Sequence[Utterance], options: SynthesisOptions, debug: bool = False,
                 frame_budget: int = 0, prompt_budget: int = 0, kv_bf16: bool = False):
        """frame_budget / prompt_budget > 0: capacity (frames per row / prompt positions per row) for requests swapped in
        later with a larger max_length or a longer prompt (q3_session_create_reserved); the rows of `utts` still end at
        their own limits."""
        self.model = model
        self.B = len(utts)
        self.options = options
        self._keep = []
        self._ref_frames = [0 if u.ref_codes is None else int(np.asarray(u.ref_codes).reshape(-1, 16).shape[0]) for u in utts]
        self._frame_budget = int(frame_budget)
        self._row_limit = [self._limit_of(u) for u in utts]       # frames a row can reach: sizes the PCM buffers of run()
        # per row what sizes the buffers of next_chunks_out: [tempo, level on, pitch, silence (edge_ms, pause_ms) or None]
        self._out_rows = [[1000, False, 0, None] for _ in utts]
        reqs = (CRequest * self.B)()
        for i, u in enumerate(utts):
            self._fill(reqs[i], u)
        h = ctypes.c_void_p()
        if frame_budget > 0 or prompt_budget > 0:
            check(lib.q3_session_create_reserved(model._h, reqs, self.B, int(frame_budget), int(prompt_budget), ctypes.byref(h)))
        else:
            check(lib.q3_session_create(model._h, reqs, self.B, ctypes.byref(h)))
        self._h = h
        if kv_bf16:      # the reference GPU path's cache dtype (q3_session_set_kv_dtype): half the K/V bytes, not bit-comparable with the F32 oracle
            check(lib.q3_session_set_kv_dtype(self._h, 1))
        if debug:
            check(lib.q3_session_set_debug(self._h, 1))

    def _fill(self, r, u: Utterance):
        fill_request(r, u, self.options, self._keep)

    def _note_out(self, b: int, field: int, value):
        for r in (range(self.B) if int(b) < 0 else [int(b)]):
            self._out_rows[r][field] = value

    def _limit_of(self, u: Utterance) -> int:
        lim = u.max_length if u.max_length is not None else (u.options or self.options).max_length
        return max(int(lim), int(self.options.max_length), self._frame_budget)

    def close(self):
        if getattr(self, "_h", None):
            lib.q3_session_free(self._h); self._h = None

    __del__ = close

    def replace(self, b: int, utt: Utterance):
        """Continuous batching (q3_session_replace): row b — normally a finished one whose codes / PCM have been fetched — starts
        over with `utt` at its frame 0 while the other rows keep going; they are bit-for-bit unaffected."""
        r = CRequest()
        keep = []                                   # the C side copies the request: nothing to keep beyond the call
        fill_request(r, utt, self.options, keep)
        check(lib.q3_session_replace(self._h, int(b), ctypes.byref(r)))
        del keep
        if b < len(self._row_limit):
            self._row_limit[b] = self._limit_of(utt)
        self._ref_frames[b] = 0 if utt.ref_codes is None else int(np.asarray(utt.ref_codes).reshape(-1, 16).shape[0])

    def park_row(self, b: int) -> "Parked":
        """Take running row b out of the session between two frames (q3_session_park_row): its K/V pages, device state and codes
        move into the returned record; the row is left idle. The other rows keep their bits."""
        h = ctypes.c_void_p()
        check(lib.q3_session_park_row(self._h, int(b), ctypes.byref(h)))
        p = Parked(h, self, self._row_limit[b] if b < len(self._row_limit) else 0, self._ref_frames[b])
        self._ref_frames[b] = 0
        return p

    def resume_row(self, b: int, parked: "Parked"):
        """Put a record of this session into row b — idle or ended — (q3_session_resume_row): the row goes on exactly where it
        stopped. The record is consumed on success."""
        if parked._h is None:
            raise ValueError("the record has been resumed or freed")
        check(lib.q3_session_resume_row(self._h, int(b), parked._h))
        parked._h = None
        if b < len(self._row_limit):
            self._row_limit[b] = max(self._row_limit[b], parked._row_limit)
        self._ref_frames[b] = parked._ref_frames

    def next_chunk(self) -> Tuple[Optional[AudioBuffer], bool]:
        """The next chunk of a one-row session, with read-ahead (q3_session_next_chunk): (chunk or None, done). A row has one
        streaming position, so this may be mixed with `next_chunk_row` / `next_chunks` on the same row."""
        chunk = self.options.chunk_frames if self.options.chunk_frames > 0 else 10      # the engine's default
        buf = np.zeros(chunk * self.model.config.samples_per_frame, dtype=np.float32)
        n = ctypes.c_size_t(); d = ctypes.c_int()
        check(lib.q3_session_next_chunk(self._h, buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(n), ctypes.byref(d)))
        return (AudioBuffer(buf[:n.value].copy()) if n.value else None), bool(d.value)

    def next_chunk_row(self, b: int) -> Tuple[Optional[AudioBuffer], bool]:
        """StreamingSession::next_chunk for row b of a multi-sequence session: (chunk or None, done)."""
        spf = self.model.config.samples_per_frame
        buf = np.zeros(max(self.options.chunk_frames, 1) * spf, dtype=np.float32)
        n = ctypes.c_size_t(); d = ctypes.c_int()
        check(lib.q3_session_next_chunk_row(self._h, int(b), buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(n), ctypes.byref(d)))
        return (AudioBuffer(buf[:n.value].copy()) if n.value else None), bool(d.value)

    def next_chunks(self) -> List[Tuple[Optional[AudioBuffer], bool]]:
        """next_chunk_row for every row in one call (q3_session_next_chunks): one (chunk or None, done) per row. In continuous
        stream mode the rows' chunks are vocoded together, from per-row decoder state."""
        B = self.B; spf = self.model.config.samples_per_frame
        bufs = [np.zeros(max(self.options.chunk_frames, 1) * spf, dtype=np.float32) for _ in range(B)]
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data_as(ctypes.c_void_p) for b in bufs])
        caps = (ctypes.c_size_t * B)(*[b.size for b in bufs])
        n = (ctypes.c_size_t * B)(); d = (ctypes.c_int * B)()
        check(lib.q3_session_next_chunks(self._h, ptrs, caps, n, d))
        return [((AudioBuffer(bufs[b][:n[b]].copy()) if n[b] else None), bool(d[b])) for b in range(B)]

    def set_output(self, rate: int, pcm16: bool = False, fmt: Optional[str] = None):
        """The output of `next_chunks_out`, for all rows (q3_session_set_output): a sample rate the output stage supports, float32
        or int16 — or fmt = "f32" / "s16" / "ulaw" / "alaw" (G.711, one uint8 per sample). Legal before the first streamed chunk;
        `next_chunks` and the whole-utterance calls ignore it."""
        code = pcm_format(pcm16, fmt)
        check(lib.q3_session_set_output(self._h, int(rate), code))
        self._out = (int(rate), code)

    def set_level(self, gain_mb: int, ceiling_mb: int, b: int = -1):
        """The level of row b (-1: every row) in `next_chunks_out` (q3_session_set_level): a gain and the ceiling of its look-ahead
        peak limiter, in millibel (1/100 dB); (0, 0) = off. The window and the persistence of `set_tempo`."""
        check(lib.q3_session_set_level(self._h, int(b), int(gain_mb), int(ceiling_mb)))
        self._note_out(b, 1, bool(int(gain_mb) or int(ceiling_mb)))

    def set_loudness(self, mode: int, target_mb: int = -1900, prior_mb: int = 0, b: int = -1):
        """The loudness step of row b (-1: every row) in `next_chunks_out` (q3_session_set_loudness): LOUD_OFF, LOUD_METER or
        LOUD_NORMALIZE to target_mb (millibel of LUFS, -1900 = -19 LUFS) from the gain prior_mb. The window and the persistence of
        `set_tempo`."""
        check(lib.q3_session_set_loudness(self._h, int(b), int(mode), int(target_mb), int(prior_mb)))

    def loudness(self, b: int = 0) -> "Loudness":
        """Row b's reading after its last streamed chunk (q3_session_loudness)."""
        m = ctypes.c_float(); g = ctypes.c_float(); nb = ctypes.c_int(); cg = ctypes.c_int()
        check(lib.q3_session_loudness(self._h, int(b), ctypes.byref(m), ctypes.byref(g), ctypes.byref(nb), ctypes.byref(cg)))
        return Loudness.of(m.value, g.value, nb.value, cg.value)

    def set_silence(self, threshold_db, edge_ms: int = 50, pause_ms: int = 400, b: int = -1):
        """The silence step of row b (-1: every row) in `next_chunks_out` (q3_session_set_silence): hops under threshold_db (dB re
        full scale, -90..-20; None or 0 = off) are cut at the row's two ends down to edge_ms and inside it down to pause_ms. The
        window and the persistence of `set_tempo`."""
        thr = silence_mb(threshold_db)
        check(lib.q3_session_set_silence(self._h, int(b), thr, int(edge_ms), int(pause_ms)))
        self._note_out(b, 3, (int(edge_ms), int(pause_ms)) if thr else None)

    def set_mark(self, key, db: float = MARK_DB_DEFAULT, b: int = -1):
        """The keyed watermark of row b (-1: every row) in `next_chunks_out` (q3_session_set_mark): key 0 or None = off; db: its
        strength in dB re the local signal level, -40..-10. The window and the persistence of `set_tempo`."""
        check(lib.q3_session_set_mark(self._h, int(b), mark_key(key), mark_mb(db)))

    def silence(self, b: int = 0) -> "Silence":
        """Row b's counts after its last streamed chunk (q3_session_silence)."""
        v = [ctypes.c_int64() for _ in range(5)]
        check(lib.q3_session_silence(self._h, int(b), *[ctypes.byref(x) for x in v]))
        return Silence(*[int(x.value) for x in v])

    def set_tempo(self, tempo_permille: int, b: int = -1):
        """The speaking rate of row b (-1: every row) in `next_chunks_out` (q3_session_set_tempo): 500..2000 permille, 1250 = 1.25 x
        as fast, 1000 = off. Legal while the row has streamed nothing since its start or its `replace`; the setting stays with the
        row across a `replace` until it is set again."""
        check(lib.q3_session_set_tempo(self._h, int(b), int(tempo_permille)))
        self._note_out(b, 0, int(tempo_permille))

    def set_pitch(self, cents: int, b: int = -1):
        """The pitch of row b (-1: every row) in `next_chunks_out` (q3_session_set_pitch): -1200..1200 cents, 0 = off; the row's
        duration stays that of its tempo. Varispeed behind the time stretcher: formants move with the pitch, +-300 cents is the
        useful range for speech. The window and the persistence of `set_tempo`; a pitch that the row's tempo does not admit (the
        stretcher would leave 500..2000) is refused."""
        check(lib.q3_session_set_pitch(self._h, int(b), int(cents)))
        self._note_out(b, 2, int(cents))

    def next_chunks_out(self) -> List[Tuple[Optional[AudioBuffer], bool]]:
        """`next_chunks` through the session's output stage (q3_session_next_chunks_out): one (chunk or None, done) per row, the
        chunks at the rate of `set_output`, int16 arrays when it asked for them. A row's last samples (the resampler holds 64
        input samples back) come in the call that reports it done."""
        B = self.B; spf = self.model.config.samples_per_frame
        rate, s16 = getattr(self, "_out", (24000, False))
        n_in = max(self.options.chunk_frames, 1) * spf
        rows = [tuple(r) for r in self._out_rows]
        cap = {k: pcm_stage_bound(rate, n_in, *k) for k in set(rows)}
        bufs = [np.zeros(cap[rows[b]], dtype=PCM_DTYPE[int(s16)]) for b in range(B)]
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data_as(ctypes.c_void_p) for b in bufs])
        caps = (ctypes.c_size_t * B)(*[b.size for b in bufs])
        n = (ctypes.c_size_t * B)(); d = (ctypes.c_int * B)()
        check(lib.q3_session_next_chunks_out(self._h, ptrs, caps, n, d))
        return [((AudioBuffer(bufs[b][:n[b]].copy(), rate) if n[b] else None), bool(d[b])) for b in range(B)]

    def prefill(self):
        check(lib.q3_session_prefill(self._h))

    def prefill_info(self) -> dict:
        """q3_session_prefill_info: what the prefill of a ragged first batch ran — layer passes, how many of them packed passes, rows
        packed, activation rows of the largest pack, rows that went through equal-length groups. All zeros for a one-length session."""
        info = (ctypes.c_int32 * 8)()
        check(lib.q3_session_prefill_info(self._h, info))
        return dict(passes=int(info[0]), packs=int(info[1]), rows_packed=int(info[2]), max_pack_rows=int(info[3]), rows_grouped=int(info[4]))

    # ---- streaming text input ----
    def open_text(self, b: int):
        """Row b takes the rest of its text in pieces (append_text); before prefill. Its utterance carries the first ids."""
        check(lib.q3_session_open_text(self._h, int(b)))

    def append_text(self, b: int, ids: Sequence[int], last: bool = False):
        """Append token ids to open row b; last=True closes its text (tts_eos follows)."""
        t = np.ascontiguousarray(list(ids), dtype=np.uint32)
        check(lib.q3_session_append_text(self._h, int(b), t.ctypes.data_as(ctypes.c_void_p) if t.size else None, int(t.size),
                                         1 if last else 0))

    def text_state(self, b: int = 0) -> dict:
        """n_text (tokens received), frames_committed, frames_runnable (what the text allows now), closed, frames_replayed
        (frames the session replayed, all rows)."""
        v = [ctypes.c_int() for _ in range(5)]
        check(lib.q3_session_text_state(self._h, int(b), *[ctypes.byref(x) for x in v]))
        return {"n_text": v[0].value, "frames_committed": v[1].value, "frames_runnable": v[2].value,
                "closed": bool(v[3].value), "frames_replayed": v[4].value}

    def generate(self, n_frames: int, use_graph: bool = True):
        check(lib.q3_session_generate(self._h, int(n_frames), 1 if use_graph else 0))

    def frames(self, b: int = 0) -> Tuple[int, bool]:
        n = ctypes.c_int(); d = ctypes.c_int()
        check(lib.q3_session_frames(self._h, b, ctypes.byref(n), ctypes.byref(d)))
        return n.value, bool(d.value)

    def codes(self, b: int = 0) -> np.ndarray:
        n, _ = self.frames(b)
        out = np.zeros((max(n, 1), 16), dtype=np.uint32)
        got = ctypes.c_int()
        check(lib.q3_session_codes(self._h, b, out.ctypes.data_as(ctypes.c_void_p), out.shape[0], ctypes.byref(got)))
        return out[:got.value]

    def decode(self, b: int = 0, f0: int = 0, f1: Optional[int] = None) -> np.ndarray:
        n, _ = self.frames(b)
        f1 = n if f1 is None else f1
        spf = self.model.config.samples_per_frame
        extra = 0 if self._ref_frames is None else self._ref_frames[b]
        out = np.zeros(max((f1 - f0 + extra) * spf, 1), dtype=np.float32)
        got = ctypes.c_size_t()
        check(lib.q3_session_decode(self._h, b, f0, f1, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(got)))
        return out[:got.value]

    def run(self, use_graph: bool = True) -> Tuple[List[AudioBuffer], SynthesisTiming]:
        """synthesize_with_timing (lib.rs:425-501) for the batch."""
        spf = self.model.config.samples_per_frame
        capl = [(self._row_limit[i] + self._ref_frames[i]) * spf for i in range(self.B)]      # a row's own limit may exceed the session's
        bufs = [np.zeros(c, dtype=np.float32) for c in capl]
        ptrs = (ctypes.c_void_p * self.B)(*[b.ctypes.data_as(ctypes.c_void_p) for b in bufs])
        caps = (ctypes.c_size_t * self.B)(*capl)
        ns = (ctypes.c_size_t * self.B)()
        t = CTiming()
        check(lib.q3_session_run(self._h, 1 if use_graph else 0, ptrs, caps, ns, ctypes.byref(t)))
        audio = [AudioBuffer(bufs[i][:ns[i]].copy()) for i in range(self.B)]
        return audio, SynthesisTiming(t.prefill_ms, t.generation_ms, t.generation_frames, t.decode_ms)

    def run_timing_only(self, use_graph: bool = True, pcm_out=None) -> SynthesisTiming:
        """`run` without building AudioBuffers. pcm_out = None: the samples stay in HBM; pcm_out = [(address, capacity in
        samples)] per row (e.g. rows of one pinned host tensor, reused step after step): every row's samples are copied to
        the host inside the call, as `synthesize` hands them back (lib.rs:718-784)."""
        ns = (ctypes.c_size_t * self.B)()
        t = CTiming()
        ptrs = caps = None
        if pcm_out is not None:
            assert len(pcm_out) == self.B
            ptrs = (ctypes.c_void_p * self.B)(*[int(a) for a, _ in pcm_out])
            caps = (ctypes.c_size_t * self.B)(*[int(c) for _, c in pcm_out])
        check(lib.q3_session_run(self._h, 1 if use_graph else 0, ptrs, caps, ns, ctypes.byref(t)))
        self.last_samples = [int(x) for x in ns]
        return SynthesisTiming(t.prefill_ms, t.generation_ms, t.generation_frames, t.decode_ms)

    # ---- stage taps (parity tests) ----
    def prefill_len(self, b: int = 0) -> Tuple[int, int]:
        p = ctypes.c_int(); t = ctypes.c_int()
        check(lib.q3_session_prefill_len(self._h, b, ctypes.byref(p), ctypes.byref(t)))
        return p.value, t.value

    def prefix_info(self, b: int = 0) -> int:
        """Positions of row b's prompt whose K/V came from the model's prefix cache (q3_session_prefix_info; after prefill)."""
        n = ctypes.c_int()
        check(lib.q3_session_prefix_info(self._h, int(b), ctypes.byref(n)))
        return n.value

    def get(self, what: int, shape, b: int = 0, dtype=np.float32) -> np.ndarray:
        out = np.zeros(shape, dtype=dtype)
        check(lib.q3_session_get(self._h, what, b, out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        return out

    def talker_step(self, embeds: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        cfg = self.model.config
        e = np.ascontiguousarray(embeds, dtype=np.float32).reshape(self.B, cfg.hidden)
        hid = np.zeros((self.B, cfg.hidden), dtype=np.float32); lg = np.zeros((self.B, cfg.codec_vocab), dtype=np.float32)
        check(lib.q3_talker_step(self._h, e.ctypes.data_as(ctypes.c_void_p), hid.ctypes.data_as(ctypes.c_void_p),
                                 lg.ctypes.data_as(ctypes.c_void_p)))
        return hid, lg

    def cp_generate(self, last_hidden: np.ndarray, sem_embed: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        cfg = self.model.config
        lh = np.ascontiguousarray(last_hidden, dtype=np.float32).reshape(self.B, cfg.hidden)
        se = np.ascontiguousarray(sem_embed, dtype=np.float32).reshape(self.B, cfg.hidden)
        codes = np.zeros((self.B, 15), dtype=np.uint32); lg = np.zeros((self.B, 15, cfg.cp_vocab), dtype=np.float32)
        check(lib.q3_cp_generate(self._h, lh.ctypes.data_as(ctypes.c_void_p), se.ctypes.data_as(ctypes.c_void_p),
                                 codes.ctypes.data_as(ctypes.c_void_p), lg.ctypes.data_as(ctypes.c_void_p)))
        return codes, lg

    def set_profile(self, on: bool):
        check(lib.q3_session_set_profile(self._h, 1 if on else 0))

    def profile_read(self, reset: bool = True) -> Tuple[float, float, int]:
        ms = ctypes.c_double(); by = ctypes.c_double(); n = ctypes.c_long()
        check(lib.q3_session_profile_read(self._h, ctypes.byref(ms), ctypes.byref(by), ctypes.byref(n), 1 if reset else 0))
        return ms.value, by.value, n.value

    def profile_shapes(self, reset: bool = True) -> List[Tuple[int, ...]]:
        """distinct GEMV launches since set_profile(True): (M, N, K, epi, rms 0/1, reserved 0, tiled, count)"""
        n = ctypes.c_int()
        check(lib.q3_session_profile_shapes(self._h, None, 0, ctypes.byref(n), 0))
        buf = (ctypes.c_int * (8 * max(n.value, 1)))()
        check(lib.q3_session_profile_shapes(self._h, buf, n.value, ctypes.byref(n), 1 if reset else 0))
        return [tuple(buf[i * 8:(i + 1) * 8]) for i in range(n.value)]

    def submit_info(self) -> Tuple[int, int]:
        """(path, packets per frame): 0 nothing captured / eager, 1 hipGraphLaunch, 2 own AQL queue with HIP's fences, 4 own AQL
        queue with fence-free boundaries between the write-through kernels (the default), 3 own queue without any fence (probe)
        (include/q3tts.h: q3_session_submit_info; environment Q3_AQL)."""
        p = ctypes.c_int(); n = ctypes.c_int()
        check(lib.q3_session_submit_info(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def submit_fences(self) -> Tuple[int, int]:
        """(packets per frame without their acquire fence, without their release fence): q3_session_submit_fences"""
        a = ctypes.c_int(); r = ctypes.c_int()
        check(lib.q3_session_submit_fences(self._h, ctypes.byref(a), ctypes.byref(r)))
        return a.value, r.value

    def frame_bytes(self, kv_len: int) -> Tuple[float, float]:
        w = ctypes.c_double(); k = ctypes.c_double()
        check(lib.q3_session_frame_bytes(self._h, kv_len, ctypes.byref(w), ctypes.byref(k)))
        return w.value, k.value


class Parked:
    """A parked row (q3_parked): what Session.park_row returns and Session.resume_row consumes. It holds the row's K/V pages
    until it is resumed or freed, and may outlive its session."""

    def __init__(self, handle, session: "Session", row_limit: int, ref_frames: int):
        self._h = handle
        self._model = session.model          # the record holds its own reference on the native model; this keeps the wrapper too
        self._row_limit = row_limit
        self._ref_frames = ref_frames

    def info(self) -> dict:
        if self._h is None:
            raise ValueError("the record has been resumed or freed")
        v = [ctypes.c_int() for _ in range(4)]; nb = ctypes.c_size_t()
        check(lib.q3_parked_info(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(nb)))
        return {"frames_committed": v[0].value, "limit": v[1].value, "done": bool(v[2].value), "kv_pages": v[3].value,
                "state_bytes": nb.value}

    def free(self):
        """Give the record's pages back without resuming it."""
        if getattr(self, "_h", None):
            lib.q3_parked_free(self._h); self._h = None

    __del__ = free


class Batcher:
    """Continuous batcher (q3_batcher): requests of any prompt kind, length and options queue up and run through the rows of
    one session; `step` fills free rows, runs a few frames of the shared frame graph and collects finished rows. The
    scheduling loop is native — this class only marshals requests and results."""
    QUEUED, RUNNING, DONE, FAILED = 0, 1, 2, 3
    CANCELLED = 4
    PARKED = 5
    _WANT = {"codes": 0, "pcm": 1, "stream": 2}

    def __init__(self, model: "Qwen3TTS", slots: int = 8, frame_budget: int = 2048, prompt_budget: int = 0,
                 options: Optional[SynthesisOptions] = None, max_parked: int = 0, quantum_frames: int = 0, fresh_first: bool = False):
        """slots: rows of the session; frame_budget: largest max_length a request may ask for; prompt_budget: prefill
        positions a row can hold (at least 16 = CustomVoice / x-vector prompts; VoiceDesign: instruct length + 16; ICL:
        reference frames + 16); options: defaults for utterances without their own. max_parked > 0 switches parking on
        (q3_batcher_set_parking): up to that many tickets may wait parked beside the rows; quantum_frames > 0 adds the time
        slice; fresh_first puts tickets that have never run ahead of parked ones."""
        self.model = model
        self.options = options or SynthesisOptions()
        h = ctypes.c_void_p()
        check(lib.q3_batcher_create(model._h, int(slots), int(frame_budget), int(prompt_budget), ctypes.byref(h)))
        self._h = h
        if max_parked or quantum_frames or fresh_first:
            check(lib.q3_batcher_set_parking(self._h, int(max_parked), int(quantum_frames), 1 if fresh_first else 0))
        self._streamed = set()                      # tickets of submit_streamed (their samples leave through read, not fetch)
        self._output = {}                           # ticket -> (rate, pcm16) of the streamed tickets with an output of their own

    def close(self):
        if getattr(self, "_h", None):
            lib.q3_batcher_free(self._h); self._h = None

    __del__ = close

    def submit(self, utt: Utterance, want_pcm: bool = True) -> int:
        """Queue one request; returns its ticket. The request is copied by the library."""
        keep = []                                   # alive until the call returns: the library copies the request
        r = CRequest(); fill_request(r, utt, self.options, keep)
        t = ctypes.c_int64()
        check(lib.q3_batcher_submit(self._h, ctypes.byref(r), 1 if want_pcm else 0, ctypes.byref(t)))
        return int(t.value)

    def submit_streamed(self, utt: Utterance, sample_rate: int = 24000, pcm16: bool = False, tempo_permille: int = 1000,
                        fmt: Optional[str] = None, gain_mb: int = 0, ceiling_mb: int = 0, target_lufs: Optional[float] = None,
                        prior_gain_db: float = 0.0, pitch_cents: int = 0, silence=None, mark=None) -> int:
        """Queue one request whose audio is delivered while it runs (`read`); returns its ticket. sample_rate / pcm16 / fmt: the
        ticket's own output (q3_batcher_ticket_output) — `read` then returns samples at that rate, int16 when asked, uint8 for
        fmt "ulaw" / "alaw". tempo_permille: its speaking rate (q3_batcher_ticket_tempo; 1250 = 1.25 x as fast, 1000 = off).
        gain_mb / ceiling_mb: its level (q3_batcher_ticket_level; millibel, (0, 0) = off). target_lufs: the loudness it is steered
        to, from the gain prior_gain_db (q3_batcher_ticket_loudness; `loudness(ticket)` reads the result). pitch_cents: its pitch
        (q3_batcher_ticket_pitch; -1200..1200, 0 = off). silence = (threshold_db, edge_ms, pause_ms): its silence step
        (q3_batcher_ticket_silence; `silence(ticket)` reads the counts). mark = (key, db) or key: its keyed watermark
        (q3_batcher_ticket_mark)."""
        code = pcm_format(pcm16, fmt)
        keep = []
        r = CRequest(); fill_request(r, utt, self.options, keep)
        t = ctypes.c_int64()
        check(lib.q3_batcher_submit_streamed(self._h, ctypes.byref(r), ctypes.byref(t)))
        self._streamed.add(int(t.value))
        self._set_output(int(t.value), sample_rate, code, tempo_permille, gain_mb, ceiling_mb, pitch_cents)
        if target_lufs is not None:
            try:
                self.ticket_loudness(int(t.value), LOUD_NORMALIZE, int(round(float(target_lufs) * 100.0)), int(round(float(prior_gain_db) * 100.0)))
            except _lib.Q3Error:
                self.cancel(int(t.value)); self.fetch(int(t.value))      # the ticket was never run: it leaves with the refusal
                raise
        if silence is not None:
            try:
                self.ticket_silence(int(t.value), *silence)
            except _lib.Q3Error:
                self.cancel(int(t.value)); self.fetch(int(t.value))
                raise
        if mark is not None:
            try:
                self.ticket_mark(int(t.value), *(mark if isinstance(mark, (tuple, list)) else (mark,)))
            except _lib.Q3Error:
                self.cancel(int(t.value)); self.fetch(int(t.value))
                raise
        return int(t.value)

    def _set_output(self, ticket: int, sample_rate: int, code: int, tempo_permille: int = 1000, gain_mb: int = 0, ceiling_mb: int = 0,
                    pitch_cents: int = 0):
        code = int(code); level = bool(int(gain_mb) or int(ceiling_mb))
        if int(sample_rate) == 24000 and not code and int(tempo_permille) == 1000 and not level and not int(pitch_cents):
            return
        try:
            if int(sample_rate) != 24000 or code:
                self.ticket_output(ticket, sample_rate, fmt=PCM_NAMES[code])
            if int(tempo_permille) != 1000:
                self.ticket_tempo(ticket, tempo_permille)
            if int(pitch_cents):
                self.ticket_pitch(ticket, pitch_cents)
            if level:
                self.ticket_level(ticket, gain_mb, ceiling_mb)
        except _lib.Q3Error:
            self.cancel(ticket); self.fetch(ticket)      # the ticket was never run: it leaves with the refusal
            raise

    def ticket_output(self, ticket: int, sample_rate: int, pcm16: bool = False, fmt: Optional[str] = None):
        """A streamed ticket's own output (q3_batcher_ticket_output): between its submission and the next `step`."""
        code = pcm_format(pcm16, fmt)
        check(lib.q3_batcher_ticket_output(self._h, int(ticket), int(sample_rate), code))
        if int(sample_rate) == 24000 and not code:
            self._output.pop(int(ticket), None)
        else:
            self._output[int(ticket)] = (int(sample_rate), code)

    def ticket_level(self, ticket: int, gain_mb: int, ceiling_mb: int):
        """A streamed ticket's level (q3_batcher_ticket_level): between its submission and the next `step`."""
        check(lib.q3_batcher_ticket_level(self._h, int(ticket), int(gain_mb), int(ceiling_mb)))
        if int(gain_mb) or int(ceiling_mb):
            self._output.setdefault(int(ticket), (24000, PCM_F32))      # read through q3_batcher_read_out

    def ticket_loudness(self, ticket: int, mode: int, target_mb: int = -1900, prior_mb: int = 0):
        """A streamed ticket's loudness step (q3_batcher_ticket_loudness): between its submission and the next `step`."""
        check(lib.q3_batcher_ticket_loudness(self._h, int(ticket), int(mode), int(target_mb), int(prior_mb)))
        if int(mode) != LOUD_OFF:
            self._output.setdefault(int(ticket), (24000, PCM_F32))      # read through q3_batcher_read_out

    def loudness(self, ticket: int) -> "Loudness":
        """The ticket's reading after the parts that have landed (q3_batcher_ticket_loudness_read): final once `read` has reported
        it done, valid until `fetch`."""
        m = ctypes.c_float(); g = ctypes.c_float(); nb = ctypes.c_int(); cg = ctypes.c_int()
        check(lib.q3_batcher_ticket_loudness_read(self._h, int(ticket), ctypes.byref(m), ctypes.byref(g), ctypes.byref(nb), ctypes.byref(cg)))
        return Loudness.of(m.value, g.value, nb.value, cg.value)

    def ticket_mark(self, ticket: int, key, db: float = MARK_DB_DEFAULT):
        """A streamed ticket's keyed watermark (q3_batcher_ticket_mark): between its submission and the next `step`."""
        check(lib.q3_batcher_ticket_mark(self._h, int(ticket), mark_key(key), mark_mb(db)))
        if mark_key(key):
            self._output.setdefault(int(ticket), (24000, PCM_F32))      # read through q3_batcher_read_out

    def ticket_silence(self, ticket: int, threshold_db, edge_ms: int = 50, pause_ms: int = 400):
        """A streamed ticket's silence step (q3_batcher_ticket_silence): between its submission and the next `step`."""
        thr = silence_mb(threshold_db)
        check(lib.q3_batcher_ticket_silence(self._h, int(ticket), thr, int(edge_ms), int(pause_ms)))
        if thr:
            self._output.setdefault(int(ticket), (24000, PCM_F32))      # read through q3_batcher_read_out

    def silence(self, ticket: int) -> "Silence":
        """The ticket's counts after the parts that have landed (q3_batcher_ticket_silence_read): final once `read` has reported it
        done, valid until `fetch`."""
        v = [ctypes.c_int64() for _ in range(5)]
        check(lib.q3_batcher_ticket_silence_read(self._h, int(ticket), *[ctypes.byref(x) for x in v]))
        return Silence(*[int(x.value) for x in v])

    def ticket_tempo(self, ticket: int, tempo_permille: int):
        """A streamed ticket's speaking rate (q3_batcher_ticket_tempo): between its submission and the next `step`."""
        check(lib.q3_batcher_ticket_tempo(self._h, int(ticket), int(tempo_permille)))
        if int(tempo_permille) != 1000:
            self._output.setdefault(int(ticket), (24000, PCM_F32))      # read through q3_batcher_read_out

    def ticket_pitch(self, ticket: int, cents: int):
        """A streamed ticket's pitch in cents (q3_batcher_ticket_pitch): between its submission and the next `step`."""
        check(lib.q3_batcher_ticket_pitch(self._h, int(ticket), int(cents)))
        if int(cents):
            self._output.setdefault(int(ticket), (24000, PCM_F32))      # read through q3_batcher_read_out

    def submit_open(self, utt: Utterance, want: str = "stream", sample_rate: int = 24000, pcm16: bool = False,
                    fmt: Optional[str] = None) -> int:
        """Queue one request whose text arrives in pieces (`append_text`); the utterance carries the first ids. want: "stream"
        (samples through `read`), "pcm" or "codes" (through `fetch`). sample_rate / pcm16 / fmt (want "stream" only): the ticket's
        own output, as in `submit_streamed`. Returns its ticket."""
        if want not in self._WANT:
            raise ValueError(f"want must be one of {sorted(self._WANT)}, not {want!r}")
        code = pcm_format(pcm16, fmt)
        if want != "stream" and (int(sample_rate) != 24000 or code):
            raise ValueError("sample_rate / pcm16 apply to streamed tickets (want=\"stream\")")
        keep = []
        r = CRequest(); fill_request(r, utt, self.options, keep)
        t = ctypes.c_int64()
        check(lib.q3_batcher_submit_open(self._h, ctypes.byref(r), self._WANT[want], ctypes.byref(t)))
        if want == "stream":
            self._streamed.add(int(t.value))
            self._set_output(int(t.value), sample_rate, code)
        return int(t.value)

    def append_text(self, ticket: int, ids: Sequence[int], last: bool = False):
        """Append token ids to an open ticket, in any state (queued, being prefilled, running); last=True closes its text. Host
        only: the frames see the tokens from the next `step` on."""
        t = np.ascontiguousarray(list(ids), dtype=np.uint32)
        check(lib.q3_batcher_append_text(self._h, int(ticket), t.ctypes.data_as(ctypes.c_void_p) if t.size else None, int(t.size),
                                         1 if last else 0))

    def text_state(self, ticket: int) -> dict:
        """n_text (tokens received), frames_committed, frames_runnable (what the text allows now), closed."""
        v = [ctypes.c_int() for _ in range(4)]
        check(lib.q3_batcher_text_state(self._h, int(ticket), *[ctypes.byref(x) for x in v]))
        return {"n_text": v[0].value, "frames_committed": v[1].value, "frames_runnable": v[2].value, "closed": bool(v[3].value)}

    def cancel(self, ticket: int):
        """Give a ticket's place back (between steps): a queued one leaves the queue, a running one keeps the frames it has
        committed (`fetch` / `read` deliver them) and frees its row. The ticket reads CANCELLED."""
        check(lib.q3_batcher_cancel(self._h, int(ticket)))

    def park(self, ticket: int):
        """Take a running ticket out of its row (between steps); it reads PARKED and keeps its frames until `unpark`."""
        check(lib.q3_batcher_park(self._h, int(ticket)))

    def unpark(self, ticket: int):
        """A parked ticket waits for a row again: it re-enters — any free row — at a later fill and goes on where it stopped."""
        check(lib.q3_batcher_unpark(self._h, int(ticket)))

    def park_info(self) -> dict:
        """n_parked, max_parked, parks, resumes, moved (resumes into another row than the one left), pages_parked."""
        n = ctypes.c_int(); mx = ctypes.c_int(); pg = ctypes.c_int()
        v = [ctypes.c_longlong() for _ in range(3)]
        check(lib.q3_batcher_park_info(self._h, ctypes.byref(n), ctypes.byref(mx), *[ctypes.byref(x) for x in v], ctypes.byref(pg)))
        return {"n_parked": n.value, "max_parked": mx.value, "parks": v[0].value, "resumes": v[1].value, "moved": v[2].value,
                "pages_parked": pg.value}

    def read(self, ticket: int, max_samples: Optional[int] = None) -> Tuple[np.ndarray, bool]:
        """(samples of a streamed ticket that have landed and were not read yet — at most max_samples —, done). Never blocks;
        done is True once the ticket has finished and its last sample has been read. A failed ticket raises its error. A ticket
        with an output of its own (`submit_streamed(..., sample_rate=, pcm16=)`) is read in that format (q3_batcher_read_out)."""
        if max_samples is None:
            max_samples = max(self.poll(ticket)[2], 1)      # every landed sample (more may land before the read: they come next time)
        if int(ticket) in self._output:
            buf = np.zeros(int(max_samples), PCM_DTYPE[int(self._output[int(ticket)][1])])
            n = ctypes.c_size_t(); d = ctypes.c_int()
            check(lib.q3_batcher_read_out(self._h, int(ticket), buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(n), ctypes.byref(d)))
            return buf[:n.value].copy(), bool(d.value)
        buf = np.zeros(int(max_samples), np.float32)
        n = ctypes.c_size_t(); d = ctypes.c_int()
        check(lib.q3_batcher_read(self._h, int(ticket), buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(n), ctypes.byref(d)))
        return buf[:n.value].copy(), bool(d.value)

    def stream_info(self) -> dict:
        """Block figures of the streamed tickets' codec stream (as CodecStream.info), as of the last decode job."""
        bf = ctypes.c_int(); bb = ctypes.c_size_t(); tot = ctypes.c_int(); use = ctypes.c_int(); peak = ctypes.c_int()
        check(lib.q3_batcher_stream_info(self._h, ctypes.byref(bf), ctypes.byref(bb), ctypes.byref(tot), ctypes.byref(use), ctypes.byref(peak)))
        return {"block_frames": bf.value, "block_bytes": bb.value, "blocks_total": tot.value, "blocks_in_use": use.value,
                "blocks_peak": peak.value}

    def step(self, n_frames: int = 32, use_graph: bool = True) -> Tuple[int, int, int]:
        """One scheduling round: (rows running, requests queued, tickets finished in this call)."""
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib.q3_batcher_step(self._h, int(n_frames), 1 if use_graph else 0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def poll(self, ticket: int) -> Tuple[int, int, int]:
        st, n, ns = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        check(lib.q3_batcher_poll(self._h, int(ticket), ctypes.byref(st), ctypes.byref(n), ctypes.byref(ns)))
        return st.value, n.value, ns.value

    def fetch(self, ticket: int) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """(codes [n][16] u32, PCM or None) of a finished ticket, which is released; a failed ticket raises its error."""
        st, n, ns = self.poll(ticket)
        if int(ticket) in self._streamed:
            ns = 0                                    # a streamed ticket's samples go through read
        codes = np.zeros((n, 16), np.uint32); pcm = np.zeros(ns, np.float32)
        check(lib.q3_batcher_fetch(self._h, int(ticket), codes.ctypes.data_as(ctypes.c_void_p), n,
                                   pcm.ctypes.data_as(ctypes.c_void_p) if ns else None, ns))
        self._streamed.discard(int(ticket))          # released by the library (a call that raised above keeps it)
        self._output.pop(int(ticket), None)
        return codes, (pcm if ns else None)

    def run_all(self, utts: Sequence[Utterance], want_pcm: bool = True, poll_frames: int = 32, use_graph: bool = True):
        """Submit everything, step until the queue is drained; results in request order (a failed request raises)."""
        tickets = [self.submit(u, want_pcm) for u in utts]
        while True:
            running, queued, _ = self.step(poll_frames, use_graph)
            if running == 0 and queued == 0:
                break
        return [self.fetch(t) for t in tickets]


class StreamingSession:
    """StreamingSession (lib.rs:1484-1782): iterate to receive AudioBuffer chunks of up to
    chunk_frames*1920 samples; each chunk is decoded as an independent utterance (lib.rs:1755-1758)."""

    def __init__(self, model: "Qwen3TTS", utt: Utterance, options: SynthesisOptions, continuous: bool = False):
        """continuous=True: chunks are decoded with left context and concatenate to exactly the non-streaming audio
        (q3_session_set_stream_mode 1); the default reproduces the reference's context-free chunk decode."""
        self._s = Session(model, [utt], options)
        if continuous:
            check(lib.q3_session_set_stream_mode(self._s._h, 1))
        self._done = False

    def next_chunk(self) -> Optional[AudioBuffer]:
        if self._done:
            return None
        chunk, self._done = self._s.next_chunk()
        return chunk

    def frames_generated(self) -> int:
        return self._s.frames(0)[0]

    def is_done(self) -> bool:
        return self._done

    def close(self):
        self._s.close()

    def __iter__(self):
        return self

    def __next__(self) -> AudioBuffer:
        c = self.next_chunk()
        if c is None:
            raise StopIteration
        return c


class TextStreamingSession:
    """StreamingSession whose text arrives in pieces (q3_session_open_text / q3_session_append_text): `push` token
    ids as they come, `finish` once the text is complete; `next_chunk` returns the next AudioBuffer, or None while the text does
    not reach a whole chunk yet. The concatenated chunks equal those of StreamingSession over the whole text."""

    def __init__(self, model: "Qwen3TTS", utt: Utterance, options: SynthesisOptions, continuous: bool = False):
        self._s = Session(model, [utt], options)
        if continuous:
            check(lib.q3_session_set_stream_mode(self._s._h, 1))
        self._s.open_text(0)
        self._done = False
        self._finished = False

    def push(self, ids: Sequence[int]):
        self._s.append_text(0, ids, last=False)

    def finish(self, ids: Sequence[int] = ()):
        if not self._finished:
            self._s.append_text(0, ids, last=True)
            self._finished = True

    def next_chunk(self) -> Optional[AudioBuffer]:
        if self._done:
            return None
        chunk, self._done = self._s.next_chunk()
        return chunk

    def text_state(self) -> dict:
        return self._s.text_state(0)

    def frames_generated(self) -> int:
        return self._s.frames(0)[0]

    def is_done(self) -> bool:
        return self._done

    def close(self):
        self._s.close()


class ModelType(enum.Enum):    # config.rs:176-194
    Base = 0
    CustomVoice = 1
    VoiceDesign = 2


class Qwen3TTS:
    """Qwen3TTS facade (lib.rs:154-173). Construct with `from_pretrained` (model directory: config.json +
    safetensors, lib.rs:180-262), `from_tensors` (name → array, the from_weights path, lib.rs:267) or
    `from_synthetic`."""

    def __init__(self, config: Q3Config, device: int = 0, _handle=None):
        self.config = config
        self.device_index = device
        self.model_type: Optional[ModelType] = None     # None = loaded without config.json (lib.rs:383-386)
        if _handle is not None:
            self._h = _handle
            return
        h = ctypes.c_void_p()
        c = config.to_c()
        check(lib.q3_model_create(ctypes.byref(c), device, ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_pretrained(cls, model_dir: str, device: int = 0) -> "Qwen3TTS":
        """Load `<dir>/config.json`, `<dir>/model.safetensors` and `<dir>/speech_tokenizer/model.safetensors`
        (lib.rs:180-262) through the C++ loader (q3_model_load). Tokenization stays with the caller."""
        h = ctypes.c_void_p(); mt = ctypes.c_int(-1)
        check(lib.q3_model_load(str(model_dir).encode(), device, ctypes.byref(h), ctypes.byref(mt)))
        from .config import CConfig
        c = CConfig()
        check(lib.q3_model_config(h, ctypes.byref(c)))
        m = cls(Q3Config.from_c(c), device, _handle=h)
        m.model_type = ModelType(mt.value) if mt.value >= 0 else None
        # Base checkpoints carry `speaker_encoder.*` (lib.rs:233-249): attach the encoder when the keys are there
        import os
        from .speaker import SpeakerEncoder, SpeakerEncoderConfig
        st = os.path.join(str(model_dir), "model.safetensors")
        probe = ctypes.c_int()
        if device >= 0 and lib.q3_safetensors_info(st.encode(), b"speaker_encoder.fc.weight", ctypes.byref(probe), None, 0, None) == 0:
            cfg_path = os.path.join(str(model_dir), "config.json")
            scfg = SpeakerEncoderConfig.from_json(cfg_path)[0] if os.path.exists(cfg_path) else SpeakerEncoderConfig(enc_dim=m.config.hidden)
            m.attach_speaker_encoder(SpeakerEncoder.from_safetensors(st, scfg, device))
        # the speech tokenizer file carries the Mimi encoder under `encoder.*` (lib.rs:251-258, encoder_12hz.rs:54-71)
        from .speech_encoder import SpeechEncoder
        tok = os.path.join(str(model_dir), "speech_tokenizer", "model.safetensors")
        if not os.path.exists(tok):
            tok = os.path.join(os.path.dirname(os.path.abspath(str(model_dir))), "speech_tokenizer", "model.safetensors")
        if device >= 0 and os.path.exists(tok) and \
                lib.q3_safetensors_info(tok.encode(), b"encoder.downsample.conv.weight", ctypes.byref(probe), None, 0, None) == 0:
            try:        # non-fatal, as try_load_speech_encoder (lib.rs:1362-1388): without it only ICL cloning is unavailable
                m.attach_speech_encoder(SpeechEncoder.from_safetensors(tok, None, device))
            except _lib.Q3Error:
                pass
        return m

    # ---- voice cloning front end (lib.rs:1049-1190) ----
    speaker_encoder = None       # SpeakerEncoder, attached by from_pretrained for Base checkpoints / attach_speaker_encoder

    def attach_speaker_encoder(self, enc):
        if enc.config.enc_dim != self.config.hidden:
            raise ValueError(f"speaker embedding dim {enc.config.enc_dim} != talker hidden size {self.config.hidden}")
        self.speaker_encoder = enc

    def supports_voice_cloning(self) -> bool:          # lib.rs:390-396
        return self.model_type in (None, ModelType.Base)

    def has_speaker_encoder(self) -> bool:
        return self.speaker_encoder is not None

    speech_encoder = None        # SpeechEncoder (Mimi), attached by from_pretrained when speech_tokenizer/model.safetensors has encoder.* keys

    def attach_speech_encoder(self, enc):
        self.speech_encoder = enc

    def has_speech_encoder(self) -> bool:              # lib.rs:1049-1051
        return self.speech_encoder is not None

    def create_voice_clone_prompt(self, ref_audio: "AudioBuffer", ref_text_ids=None, ref_codes=None):
        """create_voice_clone_prompt (lib.rs:1132-1190). x_vector_only when `ref_text_ids` is None; with a transcript the
        reference audio is also encoded to codec frames by the speech encoder (Encoder12Hz, encoder_12hz.rs:119-144) for
        ICL. `ref_codes` (optional) overrides that encoder with frames computed elsewhere."""
        from .speaker import VoiceClonePrompt
        if self.speaker_encoder is None:
            hint = {ModelType.CustomVoice: " CustomVoice models use preset speakers (synthesize_with_voice), not voice cloning. "
                                           "Use a Base model for voice cloning.",
                    ModelType.VoiceDesign: " VoiceDesign models use text-described voices, not voice cloning. "
                                           "Use a Base model for voice cloning."}.get(
                self.model_type, " Ensure model weights contain `speaker_encoder.*` keys (only Base models include a speaker encoder).")
            raise _lib.Q3Error(3, "Speaker encoder not available." + hint)
        if isinstance(ref_audio, RefAudio):       # converted on the device already: both encoders read it there
            emb = self.speaker_encoder.encode_ref(ref_audio)
            if ref_text_ids is None:
                return VoiceClonePrompt(emb)
            if ref_codes is None:
                if self.speech_encoder is None:
                    raise _lib.Q3Error(7, "ICL voice cloning requires a speech encoder, but it was not loaded. Ensure the speech tokenizer "
                                          "weights contain encoder keys, or use x_vector_only mode by passing ref_text=None.")
                ref_codes = self.speech_encoder.encode_ref(ref_audio)
            return VoiceClonePrompt(emb, np.ascontiguousarray(ref_codes, dtype=np.uint32), np.asarray(ref_text_ids, dtype=np.uint32))
        if ref_audio.sample_rate != 24000:       # both encoders assume 24 kHz input (lib.rs:1156-1166)
            ref_audio = resample_to_24k(ref_audio)
        emb = self.speaker_encoder.encode(ref_audio.samples, ref_audio.sample_rate)
        if ref_text_ids is None:
            return VoiceClonePrompt(emb)
        if ref_codes is None:
            if self.speech_encoder is None:         # lib.rs:1172-1178
                raise _lib.Q3Error(7, "ICL voice cloning requires a speech encoder, but it was not loaded. Ensure the speech tokenizer "
                                      "weights contain encoder keys, or use x_vector_only mode by passing ref_text=None.")
            ref_codes = self.speech_encoder.encode(ref_audio.samples, ref_audio.sample_rate)      # [T_frames, 16]
        return VoiceClonePrompt(emb, np.ascontiguousarray(ref_codes, dtype=np.uint32), np.asarray(ref_text_ids, dtype=np.uint32))

    def create_voice_clone_prompts(self, refs: List["RefAudio"], ref_text_ids=None):
        """create_voice_clone_prompt for many RefAudio objects with one call per encoder (encode_refs). `ref_text_ids`:
        None, or one entry per clip, None for an x-vector-only clip. Prompt i equals create_voice_clone_prompt(refs[i],
        ref_text_ids[i]) field for field."""
        from .speaker import VoiceClonePrompt
        refs = list(refs)
        texts = [None] * len(refs) if ref_text_ids is None else list(ref_text_ids)
        if len(texts) != len(refs):
            raise ValueError(f"{len(refs)} clips, {len(texts)} ref_text_ids entries")
        if any(not isinstance(r, RefAudio) for r in refs):
            raise TypeError("create_voice_clone_prompts takes RefAudio objects (RefAudio.many)")
        if not refs:
            return []
        if self.speaker_encoder is None:
            raise _lib.Q3Error(3, "Speaker encoder not available. Ensure model weights contain `speaker_encoder.*` keys "
                                  "(only Base models include a speaker encoder).")
        icl = [i for i, t in enumerate(texts) if t is not None]
        if icl and self.speech_encoder is None:
            raise _lib.Q3Error(7, "ICL voice cloning requires a speech encoder, but it was not loaded. Ensure the speech tokenizer "
                                  "weights contain encoder keys, or use x_vector_only mode by passing ref_text=None.")
        embs = self.speaker_encoder.encode_refs(refs)
        codes = dict(zip(icl, self.speech_encoder.encode_refs([refs[i] for i in icl]))) if icl else {}
        return [VoiceClonePrompt(embs[i].copy()) if texts[i] is None else
                VoiceClonePrompt(embs[i].copy(), np.ascontiguousarray(codes[i], dtype=np.uint32), np.asarray(texts[i], dtype=np.uint32))
                for i in range(len(refs))]

    def synthesize_voice_clone_prompt(self, text_ids, prompt, language: "Language", options=None):
        """synthesize_voice_clone (lib.rs:1202-1262) with a VoiceClonePrompt."""
        return self.synthesize_voice_clone(text_ids, prompt.speaker_embedding, language, options,
                                           ref_codes=prompt.ref_codes, ref_text_ids=prompt.ref_text_ids)

    def supports_preset_speakers(self) -> bool:        # lib.rs:398-404 (permissive when unknown)
        return self.model_type in (None, ModelType.CustomVoice)

    def supports_voice_design(self) -> bool:           # lib.rs:409-411
        return self.model_type == ModelType.VoiceDesign

    def close(self):
        if getattr(self, "_h", None):
            lib.q3_model_free(self._h); self._h = None

    __del__ = close

    def set_tensor(self, name: str, arr: np.ndarray, dtype: int):
        a = np.ascontiguousarray(arr)
        check(lib.q3_model_set_tensor(self._h, name.encode(), dtype, a.ctypes.data_as(ctypes.c_void_p), a.size))

    def finalize(self):
        check(lib.q3_model_finalize(self._h))

    @classmethod
    def from_synthetic(cls, config: Q3Config, device: int = 0, seed: int = synth.DEFAULT_SEED, sink=None) -> "Qwen3TTS":
        """`sink(name, array, dtype)` (optional) also receives every tensor — used by tests to feed the
        CPU oracle the identical checkpoint."""
        m = cls(config, device)
        for name, arr, dt in synth.synthetic_checkpoint(config, m._h, seed):
            m.set_tensor(name, arr, dt)
            if sink is not None:
                sink(name, arr, dt)
        m.finalize()
        return m

    @classmethod
    def from_tensors(cls, config: Q3Config, tensors, device: int = 0) -> "Qwen3TTS":
        m = cls(config, device)
        for name, (arr, dt) in tensors.items():
            m.set_tensor(name, arr, dt)
        m.finalize()
        return m

    def kv_pool_limit(self, max_pages: int):
        """Cap of the model's KV page pool (q3_model_kv_pool_limit; 0 = HBM is the limit). A session that needs a page beyond
        it fails with Q3_KV_OVERFLOW — the reference's cache-overflow bail (kv_cache.rs:293-300)."""
        check(lib.q3_model_kv_pool_limit(self._h, int(max_pages)))

    def set_codec_planes(self, planes: int):
        """bf16 planes per f32 operand in the vocoder's matrix-core convs (q3_model_set_codec_planes): 3 = exact f32 products
        (default), 2 = hi + mid planes only (PCM within 1e-4 RMS of the reference instead of 2.5e-5; 30 % less vocoder time)."""
        check(lib.q3_model_set_codec_planes(self._h, int(planes)))

    def kv_pool_trim(self) -> int:
        """Slabs of the KV page pool that hold no page in use go back to the device (q3_model_kv_pool_trim); bytes freed."""
        n = ctypes.c_size_t()
        check(lib.q3_model_kv_pool_trim(self._h, ctypes.byref(n)))
        return n.value

    def kv_pool_info(self) -> dict:
        """Page geometry and occupancy of the model's KV pool in f32-equivalent pages — a bf16 session's page counts half
        (q3_model_kv_pool_info)."""
        pp = ctypes.c_int(); pb = ctypes.c_size_t(); tot = ctypes.c_int(); use = ctypes.c_int(); peak = ctypes.c_int()
        check(lib.q3_model_kv_pool_info(self._h, ctypes.byref(pp), ctypes.byref(pb), ctypes.byref(tot), ctypes.byref(use), ctypes.byref(peak)))
        return {"page_positions": pp.value, "page_bytes": pb.value, "pages_total": tot.value, "pages_in_use": use.value, "pages_peak": peak.value}

    def prefix_cache(self, max_pages: int):
        """Capacity of the model's prefix cache in KV pages of 128 positions (q3_model_prefix_cache); 0 = off (the default), which
        also drops every cached page. With it on, the prefilled K/V pages of a VoiceDesign instruction are linked into later requests
        that carry the same instruction, and their prefill starts at the first position that is not cached — same bits, less time."""
        check(lib.q3_model_prefix_cache(self._h, int(max_pages)))

    def prefix_cache_info(self) -> dict:
        """Capacity, occupancy and counters of the prefix cache (q3_model_prefix_cache_info). pages_shared: cached pages a row
        holds too; hit_positions: prompt positions that were not computed again."""
        mx = ctypes.c_int(); n = ctypes.c_int(); sh = ctypes.c_int()
        lk = ctypes.c_longlong(); hp = ctypes.c_longlong(); ev = ctypes.c_longlong()
        check(lib.q3_model_prefix_cache_info(self._h, ctypes.byref(mx), ctypes.byref(n), ctypes.byref(sh), ctypes.byref(lk), ctypes.byref(hp), ctypes.byref(ev)))
        return {"max_pages": mx.value, "pages_cached": n.value, "pages_shared": sh.value, "lookups": lk.value,
                "hit_positions": hp.value, "evictions": ev.value}

    def arena(self) -> Tuple[int, int]:
        p = ctypes.c_void_p(); n = ctypes.c_size_t()
        check(lib.q3_model_arena(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def mark_loaded(self):
        check(lib.q3_model_mark_loaded(self._h))

    # ---- synthesis API (lib.rs:416-501, 718-870, 1070-1110) ----
    def session(self, utts: Sequence[Utterance], options: Optional[SynthesisOptions] = None, debug: bool = False, kv_bf16: bool = False) -> Session:
        return Session(self, utts, options or SynthesisOptions(), debug, kv_bf16=kv_bf16)

    def synthesize(self, text_ids: Sequence[int], options: Optional[SynthesisOptions] = None) -> AudioBuffer:
        return self.synthesize_with_voice(text_ids, Speaker.Ryan, Language.English, options)

    def synthesize_with_voice(self, text_ids, speaker: Speaker, language: Language, options=None) -> AudioBuffer:
        audio, _ = self.synthesize_with_timing(text_ids, speaker, language, options)
        return audio

    def synthesize_with_timing(self, text_ids, speaker: Speaker, language: Language, options=None):
        s = self.session([Utterance(text_ids, speaker, language)], options)
        try:
            audio, timing = s.run()
        finally:
            s.close()
        return audio[0], timing

    def synthesize_voice_design(self, text_ids, instruct_ids, language: Language, options=None) -> AudioBuffer:
        s = self.session([Utterance(text_ids, language=language, instruct_ids=instruct_ids)], options)
        try:
            audio, _ = s.run()
        finally:
            s.close()
        return audio[0]

    def synthesize_voice_clone(self, text_ids, xvector, language: Language, options=None, ref_codes=None, ref_text_ids=None):
        """synthesize_voice_clone_debug (lib.rs:897-1046): x-vector-only, or ICL when ref_codes + ref_text_ids are given.
        Returns (AudioBuffer, codes)."""
        s = self.session([Utterance(text_ids, language=language, xvector=xvector, ref_codes=ref_codes, ref_text_ids=ref_text_ids)], options)
        try:
            s.prefill(); s.generate(max(s._row_limit))
            return AudioBuffer(s.decode(0)), s.codes(0)
        finally:
            s.close()

    def synthesize_batch(self, utts: Sequence[Utterance], options=None):
        """Batch of arbitrary requests (any mix of prompt kinds and lengths): up to Q3_MAX_BATCH (64) of them per session — a
        session prefills rows of equal prefill length together and decodes all rows in one captured frame graph
        (q3_session_create on a ragged batch) —, results in request order. The timing is the sum over the sessions."""
        audio: List[Optional[AudioBuffer]] = [None] * len(utts)
        tot = SynthesisTiming(0.0, 0.0, 0, 0.0)
        for k in range(0, len(utts), MAX_BATCH):
            part = list(range(k, min(k + MAX_BATCH, len(utts))))
            s = self.session([utts[i] for i in part], options)
            try:
                a, t = s.run()
            finally:
                s.close()
            for j, i in enumerate(part):
                audio[i] = a[j]
            tot = SynthesisTiming(tot.prefill_ms + t.prefill_ms, tot.generation_ms + t.generation_ms,
                                  tot.generation_frames + t.generation_frames, tot.decode_ms + t.decode_ms)
        return audio, tot

    def synthesize_continuous(self, utts: Sequence[Utterance], options=None, slots: int = 8, poll_frames: int = 32,
                              decode: bool = True, use_graph: bool = True):
        """Continuous batching over ONE session of `slots` rows: the first `slots` requests start together; whenever a row ends
        (EOS, or its own max_length) its codes are collected and the next waiting request is swapped into the row
        (q3_session_replace) while the other rows keep running — no row idles until the slowest one is done. The requests
        may be of any prompt kind and length (a session prefills rows of equal prefill length together). Returns (codes per request, PCM per request or None, frames generated, wall seconds
        of the generation loop)."""
        import time as _time
        o = options or SynthesisOptions()
        utts = list(utts)
        n0 = min(slots, len(utts))
        budget = max((u.max_length if u.max_length is not None else (u.options or o).max_length) for u in utts)
        # capacity for the longest request and the longest prompt, whenever they arrive (prompt positions: instruct + role /
        # codec overlay rows + ICL reference frames; 16 covers the fixed part of every prompt kind, talker.rs:451-627)
        prompt = max((0 if u.instruct_ids is None else len(u.instruct_ids)) + (0 if u.ref_codes is None else int(np.asarray(u.ref_codes).reshape(-1, 16).shape[0])) + 16 for u in utts)
        s = Session(self, utts[:n0], o, frame_budget=budget, prompt_budget=prompt)
        owner = list(range(n0)); nxt = n0
        codes: List[Optional[np.ndarray]] = [None] * len(utts); pcm: List[Optional[np.ndarray]] = [None] * len(utts)
        frames = 0
        t0 = _time.perf_counter()
        try:
            s.prefill()
            while any(i is not None for i in owner):
                s.generate(poll_frames, use_graph=use_graph)
                for b in range(n0):
                    i = owner[b]
                    if i is None:
                        continue
                    n, done = s.frames(b)
                    if not done:
                        continue
                    codes[i] = s.codes(b); frames += int(codes[i].shape[0])
                    if decode:
                        pcm[i] = s.decode(b)
                    if nxt < len(utts):
                        s.replace(b, utts[nxt]); owner[b] = nxt; nxt += 1
                    else:
                        owner[b] = None
            wall = _time.perf_counter() - t0
        finally:
            s.close()
        return codes, pcm, frames, wall

    def synthesize_continuous_streaming(self, utts: Sequence[Utterance], options=None, slots: int = 8, poll_frames: int = 10,
                                        on_audio=None, use_graph: bool = True):
        """Continuous batching with streamed audio (Batcher.submit_streamed): every request's samples are handed to
        on_audio(index, samples, done) as they land — after each step of poll_frames frames —, `done` with a request's last
        piece (which may be empty). The pieces of a request concatenate to the PCM synthesize_continuous gives it. Returns
        the codes per request."""
        o = options or SynthesisOptions()
        utts = list(utts)
        budget = max((u.max_length if u.max_length is not None else (u.options or o).max_length) for u in utts)
        prompt = max((0 if u.instruct_ids is None else len(u.instruct_ids)) + (0 if u.ref_codes is None else int(np.asarray(u.ref_codes).reshape(-1, 16).shape[0])) + 16 for u in utts)
        bt = Batcher(self, slots=min(slots, max(len(utts), 1)), frame_budget=budget, prompt_budget=prompt, options=o)
        try:
            tickets = [bt.submit_streamed(u) for u in utts]
            open_ = set(range(len(utts)))

            def drain():
                for i in sorted(open_):
                    samples, done = bt.read(tickets[i])
                    if samples.size or done:
                        if on_audio is not None:
                            on_audio(i, samples, done)
                    if done:
                        open_.discard(i)
            while True:
                running, queued, _ = bt.step(poll_frames, use_graph)
                drain()
                if running == 0 and queued == 0:
                    break
            drain()                                  # (the step that found nothing running waited for the last samples)
            return [bt.fetch(t)[0] for t in tickets]
        finally:
            bt.close()

    def synthesize_streaming(self, text_ids, speaker: Speaker, language: Language, options=None,
                             continuous: bool = False) -> StreamingSession:
        return StreamingSession(self, Utterance(text_ids, speaker, language), options or SynthesisOptions(), continuous)

    def synthesize_voice_design_streaming(self, text_ids, instruct_ids, language: Language, options=None,
                                          continuous: bool = False) -> StreamingSession:
        """synthesize_voice_design_streaming (lib.rs:1095-1128)."""
        return StreamingSession(self, Utterance(text_ids, language=language, instruct_ids=instruct_ids), options or SynthesisOptions(), continuous)

    def synthesize_streaming_text(self, first_ids, speaker: Speaker, language: Language, options=None,
                                  continuous: bool = False) -> "TextStreamingSession":
        """Streaming TEXT input: speech starts from the first token ids while the rest of the text is still
        being written (an LLM -> TTS pipeline). `push` more ids as they arrive, `finish` when the text is complete; the audio
        equals synthesize_streaming over the whole text. Token ids, not text: re-tokenizing a growing string can change ids
        already sent, and that is the caller's business."""
        return TextStreamingSession(self, Utterance(list(first_ids), speaker, language), options or SynthesisOptions(), continuous)

    def synthesize_voice_clone_debug(self, text_ids, prompt, language: Language, options=None):
        """synthesize_voice_clone_debug (lib.rs:897-1046): (AudioBuffer, FrameCodes) for a VoiceClonePrompt."""
        return self.synthesize_voice_clone(text_ids, prompt.speaker_embedding, language, options,
                                           ref_codes=prompt.ref_codes, ref_text_ids=prompt.ref_text_ids)

    def device(self) -> str:                            # lib.rs:1325-1327
        return f"hip:{self.device_index}"

    @classmethod
    def from_pretrained_with_tokenizer(cls, model_dir: str, tokenizer_dir: Optional[str], device: int = 0):
        """from_pretrained_with_tokenizer (lib.rs:192-262): (model, TextTokenizer) — tokenization stays on the host side."""
        from .text import TextTokenizer
        return cls.from_pretrained(model_dir, device), TextTokenizer.from_pretrained(model_dir, tokenizer_dir)

    def decode_codes(self, codes: np.ndarray, taps=None) -> AudioBuffer:
        """decode_codes (lib.rs:881-890): codes [n][16] u32."""
        c = np.ascontiguousarray(codes, dtype=np.uint32).reshape(-1, 16)
        out = np.zeros(c.shape[0] * self.config.samples_per_frame, dtype=np.float32)
        tp = None
        if taps is not None:
            tp = (ctypes.c_void_p * 10)(*[t.ctypes.data_as(ctypes.c_void_p) if t is not None else None for t in taps])
        check(lib.q3_decode_codes(self._h, c.ctypes.data_as(ctypes.c_void_p), c.shape[0], out.ctypes.data_as(ctypes.c_void_p), tp))
        return AudioBuffer(out)

    def codec_stream(self, rows: int, max_frames: int, block_frames: int = 0, max_blocks: int = 0) -> "CodecStream":
        """The vocoder with per-row state (q3_codec_stream_*): frames are appended to rows and decoded as they come, many rows
        per pass; a row's samples are those of decode_codes over everything it has been given. block_frames > 0 (a multiple of
        32): the state is allocated in blocks of that many frames as a row grows, at most max_blocks of them (0 = no bound)."""
        return CodecStream(self, rows, max_frames, block_frames, max_blocks)

    def pcm_stage(self, rows: int, max_push_samples: int) -> "PcmStage":
        """The output stage (q3_pcm_stage_*): rows that each resample the engine's 24 kHz f32 to their own rate and format as it
        streams; max_push_samples: the most 24 kHz samples a row takes in one push."""
        return PcmStage(self, rows, max_push_samples)

    def frame_embed(self, sem_token: int, codes15, text_add: np.ndarray) -> np.ndarray:
        c = np.ascontiguousarray(codes15, dtype=np.uint32); t = np.ascontiguousarray(text_add, dtype=np.float32)
        out = np.zeros(self.config.hidden, dtype=np.float32)
        check(lib.q3_frame_embed(self._h, int(sem_token), c.ctypes.data_as(ctypes.c_void_p), t.ctypes.data_as(ctypes.c_void_p),
                                 out.ctypes.data_as(ctypes.c_void_p)))
        return out


class CodecStream:
    def __init__(self, model: "Qwen3TTS", rows: int, max_frames: int, block_frames: int = 0, max_blocks: int = 0):
        self.model = model; self.rows = int(rows); self.max_frames = int(max_frames)
        self._h = ctypes.c_void_p()
        if block_frames or max_blocks:
            check(lib.q3_codec_stream_create_blocked(model._h, self.rows, self.max_frames, int(block_frames), int(max_blocks),
                                                     ctypes.byref(self._h)))
        else:
            check(lib.q3_codec_stream_create(model._h, self.rows, self.max_frames, ctypes.byref(self._h)))

    def prime(self, row: int, codes: np.ndarray):
        """State-only frames for a row at frame 0 (a voice-clone prompt's reference codes): the caches are filled, no samples."""
        c = np.ascontiguousarray(codes, dtype=np.uint32).reshape(-1, 16)
        check(lib.q3_codec_stream_prime(self._h, int(row), c.ctypes.data_as(ctypes.c_void_p), c.shape[0]))

    def info(self) -> dict:
        """Block figures: block_frames (0 = whole-row state), block_bytes, blocks_total, blocks_in_use, blocks_peak."""
        bf = ctypes.c_int(); bb = ctypes.c_size_t(); tot = ctypes.c_int(); use = ctypes.c_int(); peak = ctypes.c_int()
        check(lib.q3_codec_stream_info(self._h, ctypes.byref(bf), ctypes.byref(bb), ctypes.byref(tot), ctypes.byref(use), ctypes.byref(peak)))
        return {"block_frames": bf.value, "block_bytes": bb.value, "blocks_total": tot.value, "blocks_in_use": use.value,
                "blocks_peak": peak.value}

    def push(self, frames: dict, stage: Optional["PcmStage"] = None, stage_rows: Optional[dict] = None, last=()) -> dict:
        """{row: codes [n][16]} -> {row: samples [n * samples_per_frame]}: every row of the call in one decode pass.
        stage: the rows' samples go through it (q3_codec_stream_push_out) — row r through stage row stage_rows[r] (default r) —
        and come back at that row's rate and format; rows in `last` flush their stage row (no frames: only the flush)."""
        if stage is None:
            return self._push_lists(list(frames.keys()), list(frames.values()))
        rows = list(frames.keys()); n = len(rows); spf = self.model.config.samples_per_frame
        cs = [np.ascontiguousarray(frames[r], dtype=np.uint32).reshape(-1, 16) for r in rows]
        srows = [int((stage_rows or {}).get(r, r)) for r in rows]
        outs = [np.zeros(stage.bound(sr, c.shape[0] * spf), dtype=stage.dtype(sr)) for sr, c in zip(srows, cs)]
        r_ = (ctypes.c_int * n)(*[int(x) for x in rows])
        fp = (ctypes.c_void_p * n)(*[c.ctypes.data_as(ctypes.c_void_p) for c in cs])
        nf = (ctypes.c_int * n)(*[c.shape[0] for c in cs])
        sr_ = (ctypes.c_int * n)(*srows)
        ls = (ctypes.c_int * n)(*[1 if r in last else 0 for r in rows])
        op = (ctypes.c_void_p * n)(*[o.ctypes.data_as(ctypes.c_void_p) for o in outs])
        cp = (ctypes.c_size_t * n)(*[o.size for o in outs])
        ns = (ctypes.c_size_t * n)()
        check(lib.q3_codec_stream_push_out(self._h, n, r_, fp, nf, stage._h, sr_, ls, op, cp, ns))
        return {int(rows[i]): outs[i][:ns[i]].copy() for i in range(n)}

    def _push_lists(self, rows: Sequence[int], codes: Sequence[np.ndarray], cap: Optional[Sequence[int]] = None) -> dict:
        """push with the rows as given (a row may be listed twice: the call is then refused); cap overrides the buffer sizes."""
        n = len(rows); spf = self.model.config.samples_per_frame
        cs = [np.ascontiguousarray(c, dtype=np.uint32).reshape(-1, 16) for c in codes]
        outs = [np.zeros(c.shape[0] * spf, dtype=np.float32) for c in cs]
        r = (ctypes.c_int * n)(*[int(x) for x in rows])
        fp = (ctypes.c_void_p * n)(*[c.ctypes.data_as(ctypes.c_void_p) for c in cs])
        nf = (ctypes.c_int * n)(*[c.shape[0] for c in cs])
        op = (ctypes.c_void_p * n)(*[o.ctypes.data_as(ctypes.c_void_p) for o in outs])
        cp = (ctypes.c_size_t * n)(*[int(x) for x in (cap if cap is not None else [o.size for o in outs])])
        check(lib.q3_codec_stream_push(self._h, n, r, fp, nf, op, cp))
        return {int(rows[i]): outs[i] for i in range(n)}

    def reset(self, row: int):
        check(lib.q3_codec_stream_reset(self._h, int(row)))

    def pos(self, row: int) -> int:
        n = ctypes.c_int()
        check(lib.q3_codec_stream_pos(self._h, int(row), ctypes.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "_h", None):
            lib.q3_codec_stream_free(self._h); self._h = None

    __del__ = close


PCM_F32, PCM_S16, PCM_ULAW, PCM_ALAW = 0, 1, 2, 3
PCM_NAMES = ("f32", "s16", "ulaw", "alaw")
PCM_DTYPE = (np.float32, np.int16, np.uint8, np.uint8)


def pcm_format(pcm16: bool = False, fmt: Optional[str] = None) -> int:
    """The Q3_PCM_* code of a `pcm16=` / `fmt=` pair of keywords (one of them at most)."""
    if fmt is None:
        return PCM_S16 if pcm16 else PCM_F32
    if pcm16:
        raise ValueError("give pcm16= or fmt=, not both")
    if fmt not in PCM_NAMES:
        raise ValueError(f"fmt must be one of {list(PCM_NAMES)}, not {fmt!r}")
    return PCM_NAMES.index(fmt)


def pcm_stage_taps(rate: int) -> Tuple[np.ndarray, int, int]:
    """(taps [L][128] f32, L, M) of the output stage's filter for `rate` (q3_pcm_stage_taps); an unsupported rate raises."""
    L = ctypes.c_int(); M = ctypes.c_int()
    check(lib.q3_pcm_stage_taps(int(rate), None, 0, ctypes.byref(L), ctypes.byref(M)))
    t = np.zeros((L.value, 128), np.float32)
    check(lib.q3_pcm_stage_taps(int(rate), t.ctypes.data_as(ctypes.c_void_p), t.size, ctypes.byref(L), ctypes.byref(M)))
    return t, L.value, M.value


def pcm_stage_bound(rate: int, n_in: int, tempo_permille: int = 1000, level: bool = False, pitch_cents: int = 0, silence=None) -> int:
    """The most samples one push of n_in 24 kHz samples returns at `rate` (q3_pcm_stage_bound), for a row at tempo_permille
    (q3_pcm_stage_bound_tempo), with `level` one that has a level (q3_pcm_stage_bound_level), with pitch_cents one that has a pitch
    (q3_pcm_stage_bound_pitch), with silence = (edge_ms, pause_ms) one that has a silence step (q3_pcm_stage_bound_silence)."""
    n = ctypes.c_size_t()
    if silence is not None:
        check(lib.q3_pcm_stage_bound_silence(int(rate), int(tempo_permille), int(pitch_cents), 1 if level else 0, int(silence[0]), int(silence[1]),
                                             int(n_in), ctypes.byref(n)))
    elif int(pitch_cents):
        check(lib.q3_pcm_stage_bound_pitch(int(rate), int(tempo_permille), int(pitch_cents), 1 if level else 0, int(n_in), ctypes.byref(n)))
    elif level:
        check(lib.q3_pcm_stage_bound_level(int(rate), int(tempo_permille), int(n_in), ctypes.byref(n)))
    elif int(tempo_permille) == 1000:
        check(lib.q3_pcm_stage_bound(int(rate), int(n_in), ctypes.byref(n)))
    else:
        check(lib.q3_pcm_stage_bound_tempo(int(rate), int(tempo_permille), int(n_in), ctypes.byref(n)))
    return int(n.value)


def pcm_stage_tempo_count(tempo_permille: int, n_in_total: int, ended: bool = False) -> Tuple[int, int]:
    """(frames computed, 24 kHz samples final) of the time stretcher after n_in_total input samples (q3_pcm_stage_tempo_count)."""
    f = ctypes.c_size_t(); y = ctypes.c_size_t()
    check(lib.q3_pcm_stage_tempo_count(int(tempo_permille), int(n_in_total), 1 if ended else 0, ctypes.byref(f), ctypes.byref(y)))
    return int(f.value), int(y.value)


def pcm_stage_pitch_plan(tempo_permille: int, cents: int) -> Tuple[int, float]:
    """(the tempo the stretcher runs at, the pitch in cents the row then has) for a row at tempo_permille asked for `cents`
    (q3_pcm_stage_pitch_plan); a combination the stretcher cannot serve raises."""
    te = ctypes.c_int(); c = ctypes.c_double()
    check(lib.q3_pcm_stage_pitch_plan(int(tempo_permille), int(cents), ctypes.byref(te), ctypes.byref(c)))
    return int(te.value), float(c.value)


def pcm_stage_pitch_tables() -> Tuple[np.ndarray, np.ndarray, int, int]:
    """(Sc, W2, S1, S2): the pitch step's sinc and squared-window tables as the stage uploads them (q3_pcm_stage_pitch_tables)."""
    s1 = ctypes.c_int(); s2 = ctypes.c_int()
    check(lib.q3_pcm_stage_pitch_tables(None, 0, None, 0, ctypes.byref(s1), ctypes.byref(s2)))
    sc = np.zeros(61 * s1.value + 2, np.float32); w2 = np.zeros(64 * s2.value + 2, np.float32)
    check(lib.q3_pcm_stage_pitch_tables(sc.ctypes.data_as(ctypes.c_void_p), sc.size, w2.ctypes.data_as(ctypes.c_void_p), w2.size,
                                        ctypes.byref(s1), ctypes.byref(s2)))
    return sc, w2, s1.value, s2.value


def pcm_stage_pitch_count(tempo_permille: int, cents: int, n_in_total: int, ended: bool = False) -> int:
    """24 kHz samples that have left the stretcher and the pitch step after n_in_total input samples (q3_pcm_stage_pitch_count)."""
    n = ctypes.c_size_t()
    check(lib.q3_pcm_stage_pitch_count(int(tempo_permille), int(cents), int(n_in_total), 1 if ended else 0, ctypes.byref(n)))
    return int(n.value)


def pcm_stage_level_coeffs(gain_mb: int, ceiling_mb: int) -> Tuple[np.float32, np.float32]:
    """(g, c) as the stage computes them from millibel (q3_pcm_stage_level_coeffs)."""
    g = ctypes.c_float(); c = ctypes.c_float()
    check(lib.q3_pcm_stage_level_coeffs(int(gain_mb), int(ceiling_mb), ctypes.byref(g), ctypes.byref(c)))
    return np.float32(g.value), np.float32(c.value)


def pcm_stage_level_count(n_in_total: int, ended: bool = False) -> int:
    """Outputs of the level step that are final after n_in_total inputs (q3_pcm_stage_level_count)."""
    n = ctypes.c_size_t()
    check(lib.q3_pcm_stage_level_count(int(n_in_total), 1 if ended else 0, ctypes.byref(n)))
    return int(n.value)


LOUD_OFF, LOUD_METER, LOUD_NORMALIZE = 0, 1, 2


class Loudness(NamedTuple):
    """A row's reading: integrated loudness in LUFS (-inf without an estimate), the gated mean square it comes from, the last gain
    (a factor, and in dB: what a host passes as the next request's prior), the blocks stored and those that passed both gates."""
    lufs: float
    mean_square: float
    gain: float
    gain_db: float
    blocks: int
    gated: int

    @classmethod
    def of(cls, m, g, blocks, gated):
        m = float(np.float32(m)); g = float(np.float32(g))
        return cls(-0.691 + 10.0 * float(np.log10(m)) if m > 0.0 else float("-inf"), m, g, 20.0 * float(np.log10(g)) if g > 0.0 else float("-inf"),
                   int(blocks), int(gated))


def loudness_kweight(rate: int) -> Tuple[np.ndarray, np.ndarray]:
    """BS.1770's K-weighting at `rate`: (shelf, high-pass), each b0 b1 b2 a0 a1 a2 in float64 (q3_loudness_kweight)."""
    sh = np.zeros(6, np.float64); hp = np.zeros(6, np.float64)
    check(lib.q3_loudness_kweight(int(rate), sh.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), hp.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return sh, hp


def pcm_stage_loudness_consts(target_mb: int = -1900, prior_mb: int = 0) -> Tuple[np.float32, ...]:
    """(T, P, gate_abs, a_lo, a_hi) as the stage computes them from millibel (q3_pcm_stage_loudness_consts)."""
    v = [ctypes.c_float() for _ in range(5)]
    check(lib.q3_pcm_stage_loudness_consts(int(target_mb), int(prior_mb), *[ctypes.byref(x) for x in v]))
    return tuple(np.float32(x.value) for x in v)


class Silence(NamedTuple):
    """A row's silence step in 24 kHz samples: what entered it, what left it, and what was cut at the front (the input index of the
    first sample kept), in pauses and at the end. After the flush n_in - lead_cut - pause_cut - trail_cut == n_out."""
    n_in: int
    n_out: int
    lead_cut: int
    pause_cut: int
    trail_cut: int


def silence_mb(threshold_db) -> int:
    """A threshold in dB re full scale as the stage's millibel (None or 0: off)."""
    return 0 if threshold_db is None else int(round(float(threshold_db) * 100.0))


def mark_key(key) -> int:
    """A watermark key as the library's uint64: an int, a hex string ("c0ffee" / "0xc0ffee"), None or 0 for off."""
    if key is None:
        return 0
    k = int(key, 16) if isinstance(key, str) else int(key)
    if not 0 <= k < (1 << 64):
        raise ValueError(f"a watermark key is 64 bits, not {key!r}")
    return k


def mark_mb(db) -> int:
    """A strength in dB re the local signal level as the stage's millibel."""
    return int(round(float(db) * 100.0))


def mark_carrier(key) -> np.ndarray:
    """The carrier of a key (q3_mark_carrier): one period of 4096 samples at 24 kHz, float32, unit RMS."""
    c = np.zeros(4096, np.float32)
    check(lib.q3_mark_carrier(mark_key(key), c.ctypes.data_as(ctypes.c_void_p)))
    return c


def mark_embed(samples, key, db: float = MARK_DB_DEFAULT):
    """The watermark step's definition on the CPU for one whole 24 kHz clip (q3_mark_embed), with the bits a stage row with
    `set_mark` returns — what a caller of the whole-utterance paths (`run`, `decode`, `Batcher.fetch`) applies to their result.
    AudioBuffer in, AudioBuffer out; an array gives an array."""
    x = np.ascontiguousarray(samples.samples if isinstance(samples, AudioBuffer) else samples, dtype=np.float32).reshape(-1)
    if isinstance(samples, AudioBuffer) and samples.sample_rate != 24000:
        raise ValueError(f"mark_embed takes 24 kHz audio, not {samples.sample_rate} Hz")
    y = np.zeros(x.size, np.float32)
    check(lib.q3_mark_embed(x.ctypes.data_as(ctypes.c_void_p), x.size, mark_key(key), mark_mb(db), y.ctypes.data_as(ctypes.c_void_p)))
    return AudioBuffer(y, 24000) if isinstance(samples, AudioBuffer) else y


@dataclass
class MarkScore:
    """The detector's reading of a clip for one key: score in standard deviations of the correlation over the 4096 shifts, offset:
    the carrier index of the clip's first sample, detected: score >= MARK_SCORE_DETECT."""
    score: float
    offset: int
    detected: bool


def mark_detect(samples, key) -> MarkScore:
    """The watermark detector on the CPU, in float64 (q3_mark_detect), for a 24 kHz mono clip of at least 8192 samples."""
    x = np.ascontiguousarray(samples.samples if isinstance(samples, AudioBuffer) else samples, dtype=np.float32).reshape(-1)
    if isinstance(samples, AudioBuffer) and samples.sample_rate != 24000:
        raise ValueError(f"mark_detect takes 24 kHz audio, not {samples.sample_rate} Hz (resample it first)")
    sc = ctypes.c_double(); off = ctypes.c_int()
    check(lib.q3_mark_detect(x.ctypes.data_as(ctypes.c_void_p), x.size, mark_key(key), ctypes.byref(sc), ctypes.byref(off)))
    return MarkScore(sc.value, off.value, sc.value >= MARK_SCORE_DETECT)


def pcm_stage_silence_hold(edge_ms: int, pause_ms: int) -> int:
    """The most samples a row's silence step retains (q3_pcm_stage_silence_hold)."""
    n = ctypes.c_size_t()
    check(lib.q3_pcm_stage_silence_hold(int(edge_ms), int(pause_ms), ctypes.byref(n)))
    return int(n.value)


def trim_silence(samples, threshold_db: float, edge_ms: int = 50, pause_ms: int = 400, counts: bool = False):
    """The silence step's definition on the CPU for one whole 24 kHz clip (q3_silence_trim): the edges cut down to edge_ms, pauses
    down to pause_ms, with the bits a stage row with `set_silence` returns. AudioBuffer in, AudioBuffer out; an array gives an
    array. counts: also the Silence counts."""
    x = np.ascontiguousarray(samples.samples if isinstance(samples, AudioBuffer) else samples, dtype=np.float32).reshape(-1)
    if isinstance(samples, AudioBuffer) and samples.sample_rate != 24000:
        raise ValueError(f"trim_silence takes 24 kHz audio, not {samples.sample_rate} Hz")
    y = np.zeros(max(x.size, 1), np.float32)
    n = ctypes.c_size_t(); c = (ctypes.c_int64 * 5)()
    check(lib.q3_silence_trim(x.ctypes.data_as(ctypes.c_void_p), x.size, silence_mb(threshold_db), int(edge_ms), int(pause_ms),
                              y.ctypes.data_as(ctypes.c_void_p), y.size, ctypes.byref(n), c))
    y = y[:int(n.value)].copy()
    out = AudioBuffer(y, 24000) if isinstance(samples, AudioBuffer) else y
    return (out, Silence(*[int(v) for v in c])) if counts else out


class PcmStage:
    """The output stage (q3_pcm_stage): `rows` independent rows, each with its own output rate and format (float32, int16 or G.711
    bytes), fed 24 kHz float32 in pushes of any size; one pass serves every row of a push."""

    def __init__(self, model, rows: int, max_push_samples: int):
        """model: a Qwen3TTS (the stage is created on its device) or a device index."""
        self.device_index = int(model) if isinstance(model, int) else int(model.device_index)
        self.rows = int(rows); self.max_push_samples = int(max_push_samples)
        self._fmt = [(24000, PCM_F32)] * self.rows
        self._tempo = [1000] * self.rows
        self._level = [False] * self.rows
        self._pitch = [0] * self.rows
        self._silence = [None] * self.rows
        self._h = ctypes.c_void_p()
        check(lib.q3_pcm_stage_create(self.device_index, self.rows, self.max_push_samples, ctypes.byref(self._h)))

    def set(self, row: int, rate: int, pcm16: bool = False, fmt: Optional[str] = None):
        """Row's output rate and format (pcm16, or fmt = "f32" / "s16" / "ulaw" / "alaw"); also restarts the row."""
        code = pcm_format(pcm16, fmt)
        check(lib.q3_pcm_stage_set(self._h, int(row), int(rate), code))
        self._fmt[int(row)] = (int(rate), code)

    def set_level(self, row: int, gain_mb: int, ceiling_mb: int):
        """Row's level (q3_pcm_stage_set_level): a gain and the ceiling of its look-ahead peak limiter in millibel (1/100 dB),
        -6000..2400 and -2400..0; (0, 0) = off; also restarts the row. `set`, `reset` and `set_tempo` keep it."""
        check(lib.q3_pcm_stage_set_level(self._h, int(row), int(gain_mb), int(ceiling_mb)))
        self._level[int(row)] = bool(int(gain_mb) or int(ceiling_mb))

    def set_tempo(self, row: int, tempo_permille: int):
        """Row's speaking rate (q3_pcm_stage_set_tempo): 500..2000 permille, 1250 = 1.25 x as fast, 1000 = off; also restarts the
        row. `set` and `reset` keep it."""
        check(lib.q3_pcm_stage_set_tempo(self._h, int(row), int(tempo_permille)))
        self._tempo[int(row)] = int(tempo_permille)

    def set_pitch(self, row: int, cents: int):
        """Row's pitch (q3_pcm_stage_set_pitch): -1200..1200 cents, 0 = off; also restarts the row. The stretcher then runs at
        `pcm_stage_pitch_plan(tempo, cents)[0]` and a varispeed step behind it brings the duration back: formants move with the
        pitch. Refused where that tempo leaves 500..2000. `set`, `reset` and the other `set_*` keep it."""
        check(lib.q3_pcm_stage_set_pitch(self._h, int(row), int(cents)))
        self._pitch[int(row)] = int(cents)

    def set_loudness(self, row: int, mode: int, target_mb: int = -1900, prior_mb: int = 0):
        """Row's loudness step (q3_pcm_stage_set_loudness): LOUD_OFF, LOUD_METER (measure, the samples pass) or LOUD_NORMALIZE
        (steer the row to target_mb, millibel of LUFS, from the gain prior_mb); also restarts the row. `set`, `reset`, `set_tempo`
        and `set_level` keep it."""
        check(lib.q3_pcm_stage_set_loudness(self._h, int(row), int(mode), int(target_mb), int(prior_mb)))

    def set_silence(self, row: int, threshold_db: float, edge_ms: int = 50, pause_ms: int = 400):
        """Row's silence step (q3_pcm_stage_set_silence): hops of 10 ms whose mean square is under threshold_db (dB re full scale,
        -90..-20; 0 or None = off) for more than 20 ms around them are cut at the stream's two ends down to edge_ms and inside it
        down to pause_ms; also restarts the row. `set`, `reset` and the other `set_*` keep it."""
        thr = silence_mb(threshold_db)
        check(lib.q3_pcm_stage_set_silence(self._h, int(row), thr, int(edge_ms), int(pause_ms)))
        self._silence[int(row)] = (int(edge_ms), int(pause_ms)) if thr else None

    def set_mark(self, row: int, key, db: float = MARK_DB_DEFAULT):
        """Row's keyed watermark (q3_pcm_stage_set_mark): key 0 or None = off; db: its strength in dB re the local signal level,
        -40..-10; also restarts the row. `set`, `reset` and the other `set_*` keep it. No count or bound changes."""
        check(lib.q3_pcm_stage_set_mark(self._h, int(row), mark_key(key), mark_mb(db)))

    def silence(self, row: int) -> "Silence":
        """The row's counts after its last successful push (q3_pcm_stage_silence)."""
        v = [ctypes.c_int64() for _ in range(5)]
        check(lib.q3_pcm_stage_silence(self._h, int(row), *[ctypes.byref(x) for x in v]))
        return Silence(*[int(x.value) for x in v])

    def loudness(self, row: int) -> Loudness:
        """The row's reading after its last successful push (q3_pcm_stage_loudness)."""
        m = ctypes.c_float(); g = ctypes.c_float(); nb = ctypes.c_int(); cg = ctypes.c_int()
        check(lib.q3_pcm_stage_loudness(self._h, int(row), ctypes.byref(m), ctypes.byref(g), ctypes.byref(nb), ctypes.byref(cg)))
        return Loudness.of(m.value, g.value, nb.value, cg.value)

    def loudness_blocks(self, row: int) -> np.ndarray:
        """The row's stored block values z_3 .. (q3_pcm_stage_loudness_blocks), float32."""
        n = ctypes.c_size_t()
        check(lib.q3_pcm_stage_loudness_blocks(self._h, int(row), None, 0, ctypes.byref(n)))      # the count
        z = np.zeros(int(n.value), np.float32)
        check(lib.q3_pcm_stage_loudness_blocks(self._h, int(row), z.ctypes.data_as(ctypes.c_void_p), z.size, ctypes.byref(n)))
        return z

    def tempo_lags(self, row: int) -> Tuple[int, np.ndarray]:
        """(k0, lags) of the frames k0 .. the row's last successful push computed (q3_pcm_stage_tempo_lags)."""
        k0 = ctypes.c_int64(); n = ctypes.c_size_t()
        check(lib.q3_pcm_stage_tempo_lags(self._h, int(row), ctypes.byref(k0), None, 0, ctypes.byref(n)))      # the count
        lags = np.zeros(int(n.value), np.int32)
        check(lib.q3_pcm_stage_tempo_lags(self._h, int(row), ctypes.byref(k0), lags.ctypes.data_as(ctypes.c_void_p), lags.size, ctypes.byref(n)))
        return int(k0.value), lags

    def reset(self, row: int):
        check(lib.q3_pcm_stage_reset(self._h, int(row)))

    def rate(self, row: int) -> int:
        return self._fmt[int(row)][0]

    def dtype(self, row: int):
        return PCM_DTYPE[self._fmt[int(row)][1]]

    def bound(self, row: int, n_in: int) -> int:
        return pcm_stage_bound(self._fmt[int(row)][0], n_in, self._tempo[int(row)], self._level[int(row)], self._pitch[int(row)],
                               self._silence[int(row)])

    def push(self, samples: dict, last=()) -> dict:
        """{row: 24 kHz f32 samples} -> {row: samples at the row's rate and format}, every row in one pass; rows in `last` are
        flushed (their input ends here)."""
        return self._push_lists(list(samples.keys()), list(samples.values()), [r in last for r in samples.keys()])

    def _push_lists(self, rows: Sequence[int], samples: Sequence[np.ndarray], last: Sequence[bool], cap: Optional[Sequence[int]] = None) -> dict:
        """push with the rows as given (a row may be listed twice: the call is then refused); cap overrides the buffer sizes."""
        n = len(rows)
        xs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in samples]
        ok = [0 <= int(r) < self.rows for r in rows]
        outs = [np.zeros(self.bound(r, x.size) if k else 1, dtype=self.dtype(r) if k else np.float32) for r, x, k in zip(rows, xs, ok)]
        r_ = (ctypes.c_int * n)(*[int(x) for x in rows])
        ip = (ctypes.c_void_p * n)(*[x.ctypes.data_as(ctypes.c_void_p) for x in xs])
        ni = (ctypes.c_size_t * n)(*[x.size for x in xs])
        ls = (ctypes.c_int * n)(*[1 if l else 0 for l in last])
        op = (ctypes.c_void_p * n)(*[o.ctypes.data_as(ctypes.c_void_p) for o in outs])
        cp = (ctypes.c_size_t * n)(*[int(c) for c in (cap if cap is not None else [o.size for o in outs])])
        ns = (ctypes.c_size_t * n)()
        check(lib.q3_pcm_stage_push(self._h, n, r_, ip, ni, ls, op, cp, ns))
        return {int(rows[i]): outs[i][:ns[i]].copy() for i in range(n)}

    def close(self):
        if getattr(self, "_h", None):
            lib.q3_pcm_stage_free(self._h); self._h = None

    __del__ = close


def resample_gpu(audio, rate: int, pcm16: bool = False, device: int = 0, tempo_permille: int = 1000, fmt: Optional[str] = None,
                 gain_mb: int = 0, ceiling_mb: int = 0, target_mb: Optional[int] = None, prior_mb: int = 0, pitch_cents: int = 0, silence=None,
                 mark=None) -> AudioBuffer:
    """One-shot use of the output stage: a whole 24 kHz clip (AudioBuffer or array) at `rate`, int16 when asked (fmt: "f32" /
    "s16" / "ulaw" / "alaw") — what a caller of the whole-utterance paths (`run`, `decode`, `Batcher.fetch`) applies to their
    result. tempo_permille: the clip's speaking rate (1250 = 1.25 x as fast, 1000 = as it is). gain_mb / ceiling_mb: its level. target_mb / prior_mb: the loudness it is
    steered to (millibel of LUFS) and the gain it starts from — a causal normaliser: the first 400 ms leave at the prior.
    pitch_cents: its pitch (-1200..1200 cents, 0 = as it is; the duration stays that of the tempo). silence = (threshold_db, edge_ms,
    pause_ms): its edges and pauses cut first, as `trim_silence` does. mark = (key, db) or key: its keyed watermark, as `mark_embed`
    adds it, behind the loudness and in front of the level."""
    code = pcm_format(pcm16, fmt)
    x = np.ascontiguousarray(audio.samples if isinstance(audio, AudioBuffer) else audio, dtype=np.float32).reshape(-1)
    if isinstance(audio, AudioBuffer) and audio.sample_rate != 24000:
        raise ValueError(f"resample_gpu takes the engine's 24 kHz audio, not {audio.sample_rate} Hz")
    ps = PcmStage(int(device), 1, max(x.size, 1))
    try:
        ps.set(0, rate, fmt=PCM_NAMES[code])
        if int(tempo_permille) != 1000:
            ps.set_tempo(0, tempo_permille)
        if int(pitch_cents):
            ps.set_pitch(0, pitch_cents)
        if int(gain_mb) or int(ceiling_mb):
            ps.set_level(0, gain_mb, ceiling_mb)
        if target_mb is not None:
            ps.set_loudness(0, LOUD_NORMALIZE, target_mb, prior_mb)
        if silence is not None:
            ps.set_silence(0, *silence)
        if mark is not None:
            ps.set_mark(0, *(mark if isinstance(mark, (tuple, list)) else (mark,)))
        return AudioBuffer(ps.push({0: x}, last=(0,))[0], int(rate))
    finally:
        ps.close()


def loudness(pcm_24k, device: int = 0) -> float:
    """Integrated loudness (ITU-R BS.1770-4, LUFS) of a whole 24 kHz clip (AudioBuffer or array), measured by a one-row output stage
    in meter mode — for a reference clip at enrolment. -inf for a clip shorter than 400 ms or below the absolute gate."""
    x = np.ascontiguousarray(pcm_24k.samples if isinstance(pcm_24k, AudioBuffer) else pcm_24k, dtype=np.float32).reshape(-1)
    if isinstance(pcm_24k, AudioBuffer) and pcm_24k.sample_rate != 24000:
        raise ValueError(f"loudness takes 24 kHz audio, not {pcm_24k.sample_rate} Hz (resample it first)")
    ps = PcmStage(int(device), 1, max(x.size, 1))
    try:
        ps.set_loudness(0, LOUD_METER)
        ps.push({0: x}, last=(0,))
        return ps.loudness(0).lufs
    finally:
        ps.close()


def pcm16(samples: np.ndarray) -> np.ndarray:
    """`(clamp(x, -1, 1) * 32767) as i16` (audio/io.rs:158-160)."""
    a = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    out = np.empty(a.size, dtype=np.int16)
    check(lib.q3_pcm16_from_f32(a.ctypes.data_as(ctypes.c_void_p), a.size, out.ctypes.data_as(ctypes.c_void_p)))
    return out


def g711(samples_i16: np.ndarray, law: str) -> np.ndarray:
    """ITU-T G.711 of int16 samples, one uint8 each (q3_g711_from_pcm16): law "ulaw" or "alaw"."""
    if law not in ("ulaw", "alaw"):
        raise ValueError(f"law must be \"ulaw\" or \"alaw\", not {law!r}")
    a = np.ascontiguousarray(samples_i16, dtype=np.int16).reshape(-1)
    out = np.empty(a.size, dtype=np.uint8)
    check(lib.q3_g711_from_pcm16(a.ctypes.data_as(ctypes.c_void_p), a.size, PCM_NAMES.index(law), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def save_wav_g711(path: str, g711_bytes: np.ndarray, sample_rate: int = 8000, law: str = "ulaw"):
    """Mono G.711 WAV (q3_wav_write_g711): format tag 7 for "ulaw", 6 for "alaw"."""
    if law not in ("ulaw", "alaw"):
        raise ValueError(f"law must be \"ulaw\" or \"alaw\", not {law!r}")
    a = np.ascontiguousarray(g711_bytes, dtype=np.uint8).reshape(-1)
    check(lib.q3_wav_write_g711(str(path).encode(), a.ctypes.data_as(ctypes.c_void_p), a.size, int(sample_rate), PCM_NAMES.index(law)))


def save_wav(path: str, samples: np.ndarray, sample_rate: int = 24000):
    """save_wav (audio/io.rs:143-165): mono PCM16."""
    a = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    check(lib.q3_wav_write_pcm16(str(path).encode(), a.ctypes.data_as(ctypes.c_void_p), a.size, int(sample_rate)))


def load_wav(path: str) -> AudioBuffer:
    """load_wav (audio/io.rs:106-141): PCM/float WAV → mono f32."""
    n = ctypes.c_int64(); rate = ctypes.c_uint32()
    check(lib.q3_wav_read(str(path).encode(), None, 0, ctypes.byref(n), ctypes.byref(rate)))
    out = np.empty(n.value, dtype=np.float32)
    check(lib.q3_wav_read(str(path).encode(), out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n), ctypes.byref(rate)))
    return AudioBuffer(out, int(rate.value))


def resample(audio: AudioBuffer, target_rate: int) -> AudioBuffer:
    """audio::resample (audio/resample.rs:164-171): windowed-sinc resampling (q3_resample); a copy when rates match."""
    x = np.ascontiguousarray(audio.samples, dtype=np.float32)
    n = ctypes.c_int64()
    check(lib.q3_resample(x.ctypes.data_as(ctypes.c_void_p), x.size, audio.sample_rate, target_rate, None, 0, ctypes.byref(n)))
    out = np.empty(n.value, np.float32)
    check(lib.q3_resample(x.ctypes.data_as(ctypes.c_void_p), x.size, audio.sample_rate, target_rate,
                          out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n)))
    return AudioBuffer(out, target_rate)


def resample_to_24k(audio: AudioBuffer) -> AudioBuffer:      # audio/resample.rs:174-176
    return resample(audio, 24000)


# ---- reference audio intake (q3_intake.hip) ----
SRC_NAMES = ("u8", "s16", "s24", "s32", "f32", "ulaw", "alaw")      # Q3_SRC_*
SRC_BYTES = (1, 2, 3, 4, 4, 1, 1)


class WavInfo(NamedTuple):
    fmt: str                 # one of SRC_NAMES
    channels: int
    bits: int
    sample_rate: int
    frames: int
    data_offset: int
    data_bytes: int


def wav_info(path: str) -> WavInfo:
    """What a WAV file holds, without decoding it (q3_wav_info): PCM 8 / 16 / 24 / 32, float32, G.711."""
    d = _lib.CWavDesc()
    check(lib.q3_wav_info(str(path).encode(), ctypes.byref(d)))
    return WavInfo(SRC_NAMES[d.format], d.channels, d.bits, int(d.sample_rate), d.frames, d.data_offset, d.data_bytes)


def g711_expand(g711_bytes: np.ndarray, law: str) -> np.ndarray:
    """ITU-T G.711 expansion of uint8 bytes to int16 (q3_g711_to_pcm16): law "ulaw" or "alaw"."""
    if law not in ("ulaw", "alaw"):
        raise ValueError(f"law must be \"ulaw\" or \"alaw\", not {law!r}")
    a = np.ascontiguousarray(g711_bytes, dtype=np.uint8).reshape(-1)
    out = np.empty(a.size, dtype=np.int16)
    check(lib.q3_g711_to_pcm16(a.ctypes.data_as(ctypes.c_void_p), a.size, PCM_NAMES.index(law), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def intake_taps(rate: int) -> Tuple[np.ndarray, int, int]:
    """(taps [L, 128] f32, L, M) of the intake's resampler for an input rate: L / M = 24000 / rate (q3_intake_taps)."""
    L = ctypes.c_int(); M = ctypes.c_int()
    check(lib.q3_intake_taps(int(rate), None, 0, ctypes.byref(L), ctypes.byref(M)))
    taps = np.empty((L.value, 128), np.float32)
    check(lib.q3_intake_taps(int(rate), taps.ctypes.data_as(ctypes.c_void_p), taps.size, ctypes.byref(L), ctypes.byref(M)))
    return taps, L.value, M.value


def intake_count(rate: int, n_in: int) -> int:
    """24 kHz samples that n_in frames at `rate` become (q3_intake_count)."""
    n = ctypes.c_int64()
    check(lib.q3_intake_count(int(rate), int(n_in), ctypes.byref(n)))
    return n.value


def _clip_of(data, sample_rate: int, fmt: str, channels: int, keep: list) -> "_lib.CClip":
    if fmt not in SRC_NAMES:
        raise ValueError(f"fmt must be one of {SRC_NAMES}, not {fmt!r}")
    raw = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    keep.append(raw)
    c = _lib.CClip()
    c.data = raw.ctypes.data if raw.size else None
    c.frames = raw.size // (SRC_BYTES[SRC_NAMES.index(fmt)] * max(1, int(channels)))
    c.channels = int(channels); c.sample_rate = int(sample_rate); c.format = SRC_NAMES.index(fmt)
    return c


class RefAudio:
    """A reference clip converted to 24 kHz mono f32 on the device by one launch (k_intake), where it stays for
    SpeakerEncoder.encode_ref / SpeechEncoder.encode_ref / Qwen3TTS.create_voice_clone_prompt. Decode and downmix are load_wav's,
    the filter is resample's."""

    def __init__(self, handle):
        self._h = handle
        n = ctypes.c_int64(); dev = ctypes.c_int(); sr = ctypes.c_uint32(); f = ctypes.c_int(); ch = ctypes.c_int()
        check(lib.q3_ref_audio_info(handle, ctypes.byref(n), ctypes.byref(dev), ctypes.byref(sr), ctypes.byref(f), ctypes.byref(ch)))
        self.n_samples, self.device_index, self.source_rate, self.source_format, self.source_channels = \
            n.value, dev.value, int(sr.value), SRC_NAMES[f.value], ch.value
        self.sample_rate = 24000

    @classmethod
    def from_wav(cls, path: str, device: int = 0) -> "RefAudio":
        h = ctypes.c_void_p()
        check(lib.q3_ref_audio_from_wav(str(path).encode(), device, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def from_samples(cls, data, sample_rate: int, fmt: str, channels: int = 1, device: int = 0) -> "RefAudio":
        """`data`: the clip's interleaved samples as they lie on disk — bytes, or an array whose memory is exactly that."""
        keep = []
        c = _clip_of(data, sample_rate, fmt, channels, keep)
        h = ctypes.c_void_p()
        check(lib.q3_ref_audio_create(device, ctypes.byref(c), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def many(cls, clips, device: int = 0) -> List["RefAudio"]:
        """One upload and one launch for all of `clips`: each (data, sample_rate, fmt) or (data, sample_rate, fmt, channels).
        All or nothing."""
        keep = []
        cs = [_clip_of(c[0], c[1], c[2], c[3] if len(c) > 3 else 1, keep) for c in clips]
        arr = (_lib.CClip * max(1, len(cs)))(*cs)
        hs = (ctypes.c_void_p * max(1, len(cs)))()
        check(lib.q3_ref_audio_create_many(device, len(cs), arr, hs))
        return [cls(ctypes.c_void_p(h)) for h in hs[:len(cs)]]

    def samples(self) -> np.ndarray:
        out = np.empty(self.n_samples, np.float32); n = ctypes.c_int64()
        check(lib.q3_ref_audio_read(self._h, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n)))
        return out

    def mark_score(self, key) -> "MarkScore":
        """The watermark detector on the device (q3_ref_audio_mark_score: k_mark_fold, k_mark_corr), on the clip where the intake
        left it; `mark_detect`'s definition."""
        sc = ctypes.c_double(); off = ctypes.c_int()
        check(lib.q3_ref_audio_mark_score(self._h, mark_key(key), ctypes.byref(sc), ctypes.byref(off)))
        return MarkScore(sc.value, off.value, sc.value >= MARK_SCORE_DETECT)

    def __len__(self) -> int:
        return self.n_samples

    def duration(self) -> float:
        return self.n_samples / 24000.0

    def close(self):
        if getattr(self, "_h", None):
            lib.q3_ref_audio_free(self._h); self._h = None

    __del__ = close


def save_codes_binary(path: str, codes: np.ndarray):
    """save_codes_binary (bin/generate_audio.rs:788-801): [n_frames][16] codes as i64 LE, frame-major."""
    a = np.ascontiguousarray(codes, dtype=np.uint32)
    assert a.ndim == 2
    check(lib.q3_codes_write_bin(str(path).encode(), a.ctypes.data_as(ctypes.c_void_p), a.shape[0], a.shape[1]))


def load_codes_binary(path: str, n_groups: int = 16) -> np.ndarray:
    n = ctypes.c_int()
    check(lib.q3_codes_read_bin(str(path).encode(), None, 0, n_groups, ctypes.byref(n)))
    out = np.empty((n.value, n_groups), dtype=np.uint32)
    check(lib.q3_codes_read_bin(str(path).encode(), out.ctypes.data_as(ctypes.c_void_p), n.value, n_groups, ctypes.byref(n)))
    return out


def save_audio_binary(path: str, samples: np.ndarray):
    """save_audio_binary (bin/generate_audio.rs:804-813): f32 LE."""
    a = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    check(lib.q3_audio_write_bin(str(path).encode(), a.ctypes.data_as(ctypes.c_void_p), a.size))


def load_audio_binary(path: str) -> np.ndarray:
    """the reader of save_audio_binary's format (generate_audio.rs:880-886): f32 LE samples."""
    n = ctypes.c_int64()
    check(lib.q3_audio_read_bin(str(path).encode(), None, 0, ctypes.byref(n)))
    out = np.empty(n.value, dtype=np.float32)
    if n.value:
        check(lib.q3_audio_read_bin(str(path).encode(), out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
    return out


def codes_to_tensor(codes: np.ndarray) -> np.ndarray:
    """codes_to_tensor (lib.rs:1417-1431): [n][16] u32 → [1][16][n] i64."""
    c = np.ascontiguousarray(codes, dtype=np.uint32).reshape(-1, 16)
    out = np.zeros((16, c.shape[0]), dtype=np.int64)
    lib.q3_codes_to_tensor(c.ctypes.data_as(ctypes.c_void_p), c.shape[0], out.ctypes.data_as(ctypes.c_void_p))
    return out.reshape(1, 16, c.shape[0])


# ---- standalone ops (parity tests) ----
def fused_residual_rmsnorm(x: np.ndarray, res: np.ndarray, w: np.ndarray, eps: float, device: int = 0):
    """FusedRmsNorm::forward_residual (fused_ops.rs:49-96) on the GPU. f32 arrays, or uint16 = bf16 bits."""
    rows, cols = x.shape
    dt = 1 if x.dtype == np.uint16 else 0
    x = np.ascontiguousarray(x); res = np.ascontiguousarray(res); w = np.ascontiguousarray(w)
    normed = np.zeros_like(x); summ = np.zeros_like(x)
    check(lib.q3_fused_residual_rmsnorm(device, dt, x.ctypes.data_as(ctypes.c_void_p), res.ctypes.data_as(ctypes.c_void_p),
                                        w.ctypes.data_as(ctypes.c_void_p), rows, cols, eps,
                                        normed.ctypes.data_as(ctypes.c_void_p), summ.ctypes.data_as(ctypes.c_void_p)))
    return normed, summ


def linear(x: np.ndarray, w_bf16: np.ndarray, bias: Optional[np.ndarray] = None, device: int = 0) -> np.ndarray:
    M, K = x.shape; N = w_bf16.shape[0]
    x = np.ascontiguousarray(x, dtype=np.float32); w = np.ascontiguousarray(w_bf16, dtype=np.uint16)
    y = np.zeros((M, N), dtype=np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    check(lib.q3_linear(device, x.ctypes.data_as(ctypes.c_void_p), w.ctypes.data_as(ctypes.c_void_p),
                        None if b is None else b.ctypes.data_as(ctypes.c_void_p), M, N, K, y.ctypes.data_as(ctypes.c_void_p)))
    return y


def linear_ex(x: np.ndarray, w_bf16: np.ndarray, *, w2_bf16: Optional[np.ndarray] = None, bias: Optional[np.ndarray] = None,
              norm_w: Optional[np.ndarray] = None, eps: float = 1e-6, resid: Optional[np.ndarray] = None, epi: int = 0,
              tiled: int = -1, ksplit: int = 1, use_ws: bool = True, y: Optional[np.ndarray] = None, M: Optional[int] = None,
              zero_buf: Optional[np.ndarray] = None, zero_n: int = 0, device: int = 0) -> np.ndarray:
    """q3_linear_ex: one launch of the GEMV family with the dispatcher's arguments spelled out (parity tests). x [M][ldx] and
    resid [M][ldr] carry their pitches as their second dimension, K and N are those of w [N][K]. y ([M_alloc][ldy] f32, C order)
    is uploaded, written in place and returned whole; zero_buf ([zero_n + guard] f32) likewise. Raises Q3Error (status 7) when
    the dispatcher refuses the arguments."""
    def f32(a):
        assert a.dtype == np.float32 and a.flags.c_contiguous
        return a
    w = np.ascontiguousarray(w_bf16, dtype=np.uint16); N, K = w.shape
    x = np.ascontiguousarray(x, dtype=np.float32)
    M = x.shape[0] if M is None else M
    assert x.ndim == 2 and x.shape[0] >= M
    if y is None:
        y = np.zeros((M, N), dtype=np.float32)
    f32(y); assert y.ndim == 2
    a = _lib.CLinearEx()
    a.M, a.N, a.K, a.ldx, a.ldy, a.M_alloc = M, N, K, x.shape[1], y.shape[1], y.shape[0]
    a.epi, a.tiled, a.ksplit, a.use_ws, a.eps = epi, tiled, ksplit, 1 if use_ws else 0, eps
    keep = [x, w, y]
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    a.x, a.w, a.y = ptr(x), ptr(w), ptr(y)
    if w2_bf16 is not None:
        w2 = np.ascontiguousarray(w2_bf16, dtype=np.uint16); assert w2.shape == w.shape
        keep.append(w2); a.w2 = ptr(w2)
    if bias is not None:
        b = np.ascontiguousarray(bias, dtype=np.float32); assert b.shape == (N,)
        keep.append(b); a.bias = ptr(b)
    if norm_w is not None:
        nw = np.ascontiguousarray(norm_w, dtype=np.float32); assert nw.shape == (K,)
        keep.append(nw); a.norm_w = ptr(nw)
    if resid is not None:
        r = np.ascontiguousarray(resid, dtype=np.float32); assert r.ndim == 2 and r.shape[0] >= M
        keep.append(r); a.resid = ptr(r); a.ldr = r.shape[1]
    if zero_buf is not None:
        f32(zero_buf); assert zero_buf.ndim == 1 and zero_buf.size >= zero_n
        a.zero_buf = ptr(zero_buf); a.zero_n = zero_n; a.zero_guard = zero_buf.size - zero_n
    check(lib.q3_linear_ex(device, ctypes.byref(a)))
    return y


def attn_step(variant: int, qkv: np.ndarray, pos, q_norm_w: np.ndarray, k_norm_w: np.ndarray, eps: float, rope_cos: np.ndarray,
              rope_sin: np.ndarray, kcache: np.ndarray, vcache: np.ndarray, nh: int, nkv: int, n_splits: int, device: int = 0):
    """q3_attn_step: one decode-attention step over a contiguous cache [B][nkv][max_seq][128] (parity tests). variant 0 = the
    one-launch kernel (+ merge), 1 = the three-launch path, 2 = the code predictor's kernel. Returns (out [B][nh*128], kcache,
    vcache) — the caches are copies of the arguments with the new position appended."""
    qkv = np.ascontiguousarray(qkv, dtype=np.float32); B = qkv.shape[0]
    assert qkv.shape == (B, (nh + 2 * nkv) * 128)
    kc = np.array(kcache, dtype=np.float32, order="C"); vc = np.array(vcache, dtype=np.float32, order="C")
    max_seq = kc.shape[2]
    assert kc.shape == (B, nkv, max_seq, 128) and vc.shape == kc.shape
    pos = np.ascontiguousarray(pos, dtype=np.int32); assert pos.shape == (B,)
    qw = np.ascontiguousarray(q_norm_w, dtype=np.float32); kw = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    rc = np.ascontiguousarray(rope_cos, dtype=np.float32); rs = np.ascontiguousarray(rope_sin, dtype=np.float32)
    assert qw.shape == (128,) and kw.shape == (128,) and rc.shape == (max_seq, 64) and rs.shape == (max_seq, 64)
    out = np.zeros((B, nh * 128), dtype=np.float32)
    a = _lib.CAttnStep()
    a.variant, a.B, a.nh, a.nkv, a.n_splits, a.max_seq, a.eps = variant, B, nh, nkv, n_splits, max_seq, eps
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    a.pos, a.qkv, a.q_norm_w, a.k_norm_w, a.rope_cos, a.rope_sin = ptr(pos), ptr(qkv), ptr(qw), ptr(kw), ptr(rc), ptr(rs)
    a.kcache, a.vcache, a.out = ptr(kc), ptr(vc), ptr(out)
    check(lib.q3_attn_step(device, ctypes.byref(a)))
    return out, kc, vc


def attn_step_ex(variant: int, pos, q_norm_w: np.ndarray, k_norm_w: np.ndarray, eps: float, rope_cos: np.ndarray, rope_sin: np.ndarray,
                 kcache: np.ndarray, vcache: np.ndarray, nh: int, nkv: int, n_splits: int = 1, *, qkv: Optional[np.ndarray] = None,
                 B: Optional[int] = None, layout: int = 0, rows_per_seq: int = 1, n_layers: int = 1, layer: int = 0, n_slabs: int = 1,
                 kv_row_pages: int = 0, page_slots=None, qkv_part: Optional[np.ndarray] = None, qkv_ssq: Optional[np.ndarray] = None,
                 qkv_K: int = 0, qkv_eps: float = 0.0, g_logits: Optional[np.ndarray] = None, g_tok=None,
                 g_qkv_tab: Optional[np.ndarray] = None, g_proj_tab: Optional[np.ndarray] = None, g_x: Optional[np.ndarray] = None,
                 g_codes: Optional[np.ndarray] = None, g_frame_idx=None, g_code_slot: int = 0, zero_buf: Optional[np.ndarray] = None,
                 zero_n: int = 0, device: int = 0) -> dict:
    """q3_attn_step_ex: one decode-attention step in the forms a session runs (parity tests; include/q3tts.h describes the
    arguments). kcache / vcache are the LOGICAL caches [n_seq][nkv][max_seq][128] f32 whatever the layout (0 contiguous, 1 f32 pages,
    2 bf16 pages). Returns a dict: out [B][nh*128], kcache, vcache (copies with the step's rows appended), stray / stray_at (paged
    layouts: elements outside the cache rows that changed, and the first one's offset), rot_used [n_seq][pages][nkv], and copies
    of g_x / g_codes / zero_buf as the step left them. Raises Q3Error (1 / 7) for what the entry refuses."""
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    f32 = lambda arr: np.ascontiguousarray(arr, dtype=np.float32)
    kc = np.array(kcache, dtype=np.float32, order="C"); vc = np.array(vcache, dtype=np.float32, order="C")
    assert kc.ndim == 4 and kc.shape[3] == 128 and kc.shape[1] == nkv and vc.shape == kc.shape
    n_seq, max_seq = kc.shape[0], kc.shape[2]
    ld = (nh + 2 * nkv) * 128
    a = _lib.CAttnStepEx()
    keep = []
    if qkv is not None:
        qkv = f32(qkv); assert qkv.ndim == 2 and qkv.shape[1] == ld
        B = qkv.shape[0] if B is None else B; assert qkv.shape[0] == B
        a.qkv = ptr(qkv)
    if qkv_part is not None:
        qkv_part = f32(qkv_part); qkv_ssq = f32(qkv_ssq); assert qkv_part.ndim == 3 and qkv_part.shape[2] == ld
        B = qkv_part.shape[1] if B is None else B
        assert qkv_part.shape[1] == B and qkv_ssq.shape == qkv_part.shape[:2]
        a.qkv_part, a.qkv_ssq, a.qkv_S, a.qkv_K, a.qkv_eps = ptr(qkv_part), ptr(qkv_ssq), qkv_part.shape[0], qkv_K, qkv_eps
    if g_logits is not None:
        g_logits = f32(g_logits); assert g_logits.ndim == 2
        B = g_logits.shape[0] if B is None else B; assert g_logits.shape[0] == B
        a.g_logits = ptr(g_logits)
    assert B is not None, "no source of q|k|v"
    pos = np.ascontiguousarray(pos, dtype=np.int32); assert pos.shape == (n_seq,)
    qw = f32(q_norm_w); kw = f32(k_norm_w); rc = f32(rope_cos); rs = f32(rope_sin)
    assert qw.shape == (128,) and kw.shape == (128,) and rc.shape == (max_seq, 64) and rs.shape == (max_seq, 64)
    out = np.zeros((B, nh * 128), dtype=np.float32)
    n_pg = (max_seq + 127) // 128
    stray = np.array([0, -1], dtype=np.int64)
    rot = np.full((n_seq, n_pg, nkv), -1, dtype=np.int32)
    a.variant, a.layout, a.B, a.nh, a.nkv, a.n_splits, a.max_seq, a.rows_per_seq = variant, layout, B, nh, nkv, n_splits, max_seq, rows_per_seq
    a.n_layers, a.layer, a.n_slabs, a.kv_row_pages, a.eps = n_layers, layer, n_slabs, kv_row_pages, eps
    a.pos, a.q_norm_w, a.k_norm_w, a.rope_cos, a.rope_sin = ptr(pos), ptr(qw), ptr(kw), ptr(rc), ptr(rs)
    a.kcache, a.vcache, a.out, a.stray, a.rot_used = ptr(kc), ptr(vc), ptr(out), ptr(stray), ptr(rot)
    if page_slots is not None:
        page_slots = np.ascontiguousarray(page_slots, dtype=np.int32); assert page_slots.shape == (n_seq, n_pg)
        a.page_slots = ptr(page_slots)
    res = dict(out=out, kcache=kc, vcache=vc, rot_used=rot)
    if g_logits is not None or g_tok is not None:
        tq = f32(g_qkv_tab); tp = f32(g_proj_tab); gx = np.array(g_x, dtype=np.float32, order="C")
        assert tq.ndim == 2 and tq.shape[1] == ld and tp.ndim == 2 and tp.shape[0] == tq.shape[0] and gx.ndim == 2
        if g_logits is not None:
            assert g_logits.shape[1] == tq.shape[0]
        keep += [tq, tp]
        a.g_qkv_tab, a.g_proj_tab, a.g_x, a.g_vocab, a.g_proj_dim, a.g_ldx = ptr(tq), ptr(tp), ptr(gx), tq.shape[0], tp.shape[1], gx.shape[1]
        res["g_x"] = gx
    if g_logits is not None:
        gc = np.array(g_codes, dtype=np.uint32, order="C"); gf = np.ascontiguousarray(g_frame_idx, dtype=np.int32)
        assert gc.ndim == 3 and gc.shape[0] == B and gc.shape[2] == 16 and gf.shape == (B,)
        keep.append(gf)
        a.g_codes, a.g_frame_idx, a.g_max_frames, a.g_code_slot = ptr(gc), ptr(gf), gc.shape[1], g_code_slot
        res["g_codes"] = gc
    if g_tok is not None:
        gt = np.ascontiguousarray(g_tok, dtype=np.uint32); assert gt.shape == (n_seq,)
        keep.append(gt); a.g_tok = ptr(gt)
    if zero_buf is not None:
        zb = np.array(zero_buf, dtype=np.float32, order="C"); assert zb.ndim == 1 and zb.size >= zero_n
        a.zero_buf, a.zero_n, a.zero_guard = ptr(zb), zero_n, zb.size - zero_n
        res["zero_buf"] = zb
    check(lib.q3_attn_step_ex(device, ctypes.byref(a)))
    res["stray"], res["stray_at"] = int(stray[0]), int(stray[1])
    return res


def kv_pages_to_bf16_ex(src: np.ndarray, src_slots, dst_slots, device: int = 0):
    """q3_kv_pages_to_bf16_ex: launch_kv_pages_to_bf16 over src [n_pages][n_layers][2][nkv][128][128] f32, scattered into the
    f32 slots src_slots and converted into the bf16 slots dst_slots (parity tests). Returns (dst uint16 of the same shape, stray,
    stray_at, rot_used [2 (src, dst)][n_pages][nkv])."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    assert src.ndim == 6 and src.shape[2] == 2 and src.shape[4:] == (128, 128)
    n_pages, n_layers, nkv = src.shape[0], src.shape[1], src.shape[3]
    ss = np.ascontiguousarray(src_slots, dtype=np.int32); ds = np.ascontiguousarray(dst_slots, dtype=np.int32)
    assert ss.shape == (n_pages,) and ds.shape == (n_pages,)
    dst = np.zeros(src.shape, dtype=np.uint16)
    rot = np.full((2, n_pages, nkv), -1, dtype=np.int32); stray = np.array([0, -1], dtype=np.int64)
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    check(lib.q3_kv_pages_to_bf16_ex(device, n_layers, nkv, n_pages, ptr(ss), ptr(ds), ptr(src), ptr(dst), ptr(rot), ptr(stray)))
    return dst, int(stray[0]), int(stray[1]), rot


def conv_path(cout: int, cin: int, L: int, k: int, dil: int = 1, phases: int = 1, packed: bool = True, has_resid: bool = False,
              planes: int = 3, aligned16: bool = True) -> int:
    """q3_conv_path: the ConvPath code launch_conv1d (phases == 1) / launch_transconv1d_taps (phases = stride, k = taps) picks for a
    shape — kernel in the low 5 bits, flags 32 PRE, 64 SEG, 128 CIS = 128, 256 NP = 2; 0 = refused. No GPU needed."""
    return lib.q3_conv_path(cout, cin, L, k, dil, phases, int(packed), int(has_resid), planes, int(aligned16))


def gemm_path(M: int, N: int, K: int, epi: int = 0, norm: bool = False, w2: bool = False, planes: bool = True):
    """q3_gemm_path: (geometry, k_ranges, k_split, n_split) launch_lm_gemm picks for a shape, or None when it refuses the
    arguments. geometry 0 = geometry 1 with the split in the kernel, 1 = geometry 1 over planes, 2, 3. No GPU needed."""
    path = (ctypes.c_int32 * 4)()
    g = lib.q3_gemm_path(M, N, K, epi, int(norm), int(w2), int(planes), path)
    return None if g < 0 else tuple(path)


def gemm_ex(x: np.ndarray, w_bf16: np.ndarray, *, w2_bf16: Optional[np.ndarray] = None, bias: Optional[np.ndarray] = None,
            norm_w: Optional[np.ndarray] = None, eps: float = 1e-6, resid: Optional[np.ndarray] = None, epi: int = 0, geometry: int = -1,
            k_split: int = 0, sup: Tuple[int, int] = (0, 0), y: Optional[np.ndarray] = None, M: Optional[int] = None, device: int = 0):
    """q3_gemm_ex: one launch of the long-prompt prefill GEMM (parity tests); arguments as linear_ex. geometry -1 = the engine's
    pick, 0 = geometry 1 with the split in the kernel, 1 / 2 / 3 forced over planes; k_split / sup = (sup_m, sup_n): 0 = the
    engine's. Returns (y, path) with path = (geometry, k_ranges, k_split, n_split) that ran. Raises Q3Error (status 7) when the
    launcher refuses."""
    w = np.ascontiguousarray(w_bf16, dtype=np.uint16); N, K = w.shape
    x = np.ascontiguousarray(x, dtype=np.float32)
    M = x.shape[0] if M is None else M
    assert x.ndim == 2 and x.shape[0] >= M
    if y is None:
        y = np.zeros((M, N), dtype=np.float32)
    assert y.dtype == np.float32 and y.flags.c_contiguous and y.ndim == 2
    path = (ctypes.c_int32 * 4)()
    a = _lib.CGemmEx()
    a.M, a.N, a.K, a.ldx, a.ldy, a.M_alloc = M, N, K, x.shape[1], y.shape[1], y.shape[0]
    a.epi, a.geometry, a.k_split, a.sup_m, a.sup_n, a.eps = epi, geometry, k_split, sup[0], sup[1], eps
    a.path = ctypes.cast(path, ctypes.POINTER(ctypes.c_int32))
    keep = [x, w, y]
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    a.x, a.w, a.y = ptr(x), ptr(w), ptr(y)
    if w2_bf16 is not None:
        w2 = np.ascontiguousarray(w2_bf16, dtype=np.uint16); assert w2.shape == w.shape
        keep.append(w2); a.w2 = ptr(w2)
    if bias is not None:
        b = np.ascontiguousarray(bias, dtype=np.float32); assert b.shape == (N,)
        keep.append(b); a.bias = ptr(b)
    if norm_w is not None:
        nw = np.ascontiguousarray(norm_w, dtype=np.float32); assert nw.shape == (K,)
        keep.append(nw); a.norm_w = ptr(nw)
    if resid is not None:
        r = np.ascontiguousarray(resid, dtype=np.float32); assert r.ndim == 2 and r.shape[0] >= M
        keep.append(r); a.resid = ptr(r); a.ldr = r.shape[1]
    check(lib.q3_gemm_ex(device, ctypes.byref(a)))
    return y, tuple(path)


def attn_prefill_path(nh: int, nkv: int, use_planes: bool, halves: int = 1):
    """q3_attn_prefill_path: (kernel, halves) launch_attn_prefill picks, or None when it refuses. No GPU needed."""
    path = (ctypes.c_int32 * 2)()
    k = lib.q3_attn_prefill_path(nh, nkv, int(use_planes), halves, path)
    return None if k < 0 else tuple(path)


def attn_prefill_ex(qkv: np.ndarray, n_seq: int, base_pos: int, q_norm_w: np.ndarray, k_norm_w: np.ndarray, eps: float, rope_cos: np.ndarray,
                    rope_sin: np.ndarray, kcache: np.ndarray, vcache: np.ndarray, nh: int, nkv: int, *, kernel: int = -1, halves: int = 1,
                    use_planes: bool = False, out: Optional[np.ndarray] = None, layout: int = 0, n_layers: int = 1, layer: int = 0,
                    n_slabs: int = 1, page_slots=None, device: int = 0):
    """q3_attn_prefill_ex: one prefill attention step over the LOGICAL cache [n_seq][nkv][max_seq][128] (parity tests): qkv
    [n_seq * rps][ld_qkv] are the rows of n_seq sequences at positions base_pos .. base_pos + rps - 1. kernel -1 = the engine's pick
    (with K/V planes when use_planes), 0 VALU / 1 gen2 MFMA / 2 transposed f32 MFMA / 3 bf16x3. out ([rows][ld_out] f32) is uploaded,
    written in place and returned whole. layout 0 (contiguous): returns (out, kcache, vcache, (kernel, halves)) — the caches are
    copies. layout 1 (f32 pages; page_slots [n_seq][ceil(max_seq / 128)], n_layers, layer, n_slabs as include/q3tts.h describes):
    returns (out, kcache, vcache, (kernel, halves), info) with info = dict(stray, stray_at, rot_used [n_seq][pages][nkv])."""
    qkv = np.ascontiguousarray(qkv, dtype=np.float32); rows = qkv.shape[0]
    assert qkv.ndim == 2 and rows % n_seq == 0
    rps = rows // n_seq
    kc = np.array(kcache, dtype=np.float32, order="C"); vc = np.array(vcache, dtype=np.float32, order="C")
    max_seq = kc.shape[2]
    assert kc.shape == (n_seq, nkv, max_seq, 128) and vc.shape == kc.shape
    qw = np.ascontiguousarray(q_norm_w, dtype=np.float32); kw = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    rc = np.ascontiguousarray(rope_cos, dtype=np.float32); rs = np.ascontiguousarray(rope_sin, dtype=np.float32)
    assert qw.shape == (128,) and kw.shape == (128,) and rc.shape == (max_seq, 64) and rs.shape == (max_seq, 64)
    if out is None:
        out = np.zeros((rows, nh * 128), dtype=np.float32)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.ndim == 2 and out.shape[0] == rows
    path = (ctypes.c_int32 * 2)()
    a = _lib.CAttnPrefillEx()
    a.n_seq, a.rps, a.base_pos, a.nh, a.nkv, a.max_seq, a.ld_qkv, a.ld_out = n_seq, rps, base_pos, nh, nkv, max_seq, qkv.shape[1], out.shape[1]
    a.kernel, a.halves, a.use_planes, a.eps = kernel, halves, int(use_planes), eps
    a.path = ctypes.cast(path, ctypes.POINTER(ctypes.c_int32))
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    a.qkv, a.q_norm_w, a.k_norm_w, a.rope_cos, a.rope_sin = ptr(qkv), ptr(qw), ptr(kw), ptr(rc), ptr(rs)
    a.kcache, a.vcache, a.out = ptr(kc), ptr(vc), ptr(out)
    if layout == 0:
        check(lib.q3_attn_prefill_ex(device, ctypes.byref(a)))
        return out, kc, vc, tuple(path)
    n_pg = (max_seq + 127) // 128
    stray = np.array([0, -1], dtype=np.int64)
    rot = np.full((n_seq, n_pg, nkv), -1, dtype=np.int32)
    a.layout, a.n_layers, a.layer, a.n_slabs, a.stray, a.rot_used = layout, n_layers, layer, n_slabs, ptr(stray), ptr(rot)
    if page_slots is not None:
        page_slots = np.ascontiguousarray(page_slots, dtype=np.int32); assert page_slots.shape == (n_seq, n_pg)
        a.page_slots = ptr(page_slots)
    check(lib.q3_attn_prefill_ex(device, ctypes.byref(a)))
    return out, kc, vc, tuple(path), dict(stray=int(stray[0]), stray_at=int(stray[1]), rot_used=rot)


def attn_prefill_packed_ex(qkv: np.ndarray, seq_len, q_norm_w: np.ndarray, k_norm_w: np.ndarray, eps: float, rope_cos: np.ndarray,
                           rope_sin: np.ndarray, kcache: np.ndarray, vcache: np.ndarray, nh: int, nkv: int, *, kernel: int = -1,
                           out: Optional[np.ndarray] = None, layout: int = 0, n_layers: int = 1, layer: int = 0, n_slabs: int = 1,
                           page_slots=None, device: int = 0):
    """q3_attn_prefill_packed_ex: the packed prefill attention step (parity tests). qkv [sum(seq_len)][ld_qkv] holds the sequences end
    to end, every one from position 0; kcache / vcache are the LOGICAL cache [n_seq][nkv][max_seq][128]. kernel -1 = per sequence by
    its length, 2 = transposed f32 MFMA, 3 = bf16x3. Returns (out, kcache, vcache, (launches of kernel 2, of kernel 3), info) with
    info = dict(stray, stray_at, rot_used, plane_tail = (bytes still NaN fill, bytes) behind the last plane tile)."""
    lens = np.ascontiguousarray(list(seq_len), dtype=np.int32); n_seq = int(lens.size)
    qkv = np.ascontiguousarray(qkv, dtype=np.float32); rows = qkv.shape[0]
    assert qkv.ndim == 2 and rows == int(lens.sum())
    kc = np.array(kcache, dtype=np.float32, order="C"); vc = np.array(vcache, dtype=np.float32, order="C")
    max_seq = kc.shape[2]
    assert kc.shape == (n_seq, nkv, max_seq, 128) and vc.shape == kc.shape
    qw = np.ascontiguousarray(q_norm_w, dtype=np.float32); kw = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    rc = np.ascontiguousarray(rope_cos, dtype=np.float32); rs = np.ascontiguousarray(rope_sin, dtype=np.float32)
    assert qw.shape == (128,) and kw.shape == (128,) and rc.shape == (max_seq, 64) and rs.shape == (max_seq, 64)
    if out is None:
        out = np.zeros((rows, nh * 128), dtype=np.float32)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.ndim == 2 and out.shape[0] == rows
    path = (ctypes.c_int32 * 2)()
    tail = np.zeros(2, dtype=np.int64)
    a = _lib.CAttnPrefillPackedEx()
    a.n_seq, a.nh, a.nkv, a.max_seq, a.ld_qkv, a.ld_out, a.kernel, a.eps = n_seq, nh, nkv, max_seq, qkv.shape[1], out.shape[1], kernel, eps
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    a.path = ctypes.cast(path, ctypes.c_void_p)
    a.seq_len, a.plane_tail = ptr(lens), ptr(tail)
    a.qkv, a.q_norm_w, a.k_norm_w, a.rope_cos, a.rope_sin = ptr(qkv), ptr(qw), ptr(kw), ptr(rc), ptr(rs)
    a.kcache, a.vcache, a.out = ptr(kc), ptr(vc), ptr(out)
    n_pg = (max_seq + 127) // 128
    stray = np.array([0, -1], dtype=np.int64)
    rot = np.full((n_seq, n_pg, nkv), -1, dtype=np.int32)
    a.layout, a.n_layers, a.layer, a.n_slabs, a.stray, a.rot_used = layout, n_layers, layer, n_slabs, ptr(stray), ptr(rot)
    if page_slots is not None:
        page_slots = np.ascontiguousarray(page_slots, dtype=np.int32); assert page_slots.shape == (n_seq, n_pg)
        a.page_slots = ptr(page_slots)
    check(lib.q3_attn_prefill_packed_ex(device, ctypes.byref(a)))
    return out, kc, vc, tuple(path), dict(stray=int(stray[0]), stray_at=int(stray[1]), rot_used=rot, plane_tail=(int(tail[0]), int(tail[1])))


PREFILL_PACK_ROWS = 4224      # the default row budget of a packed prefill pass (Q3_PREFILL_ROWS)


def prefill_pack_plan(lengths, hit_pages=None, *, row_budget: int = PREFILL_PACK_ROWS, gemm_ok: bool = True):
    """q3_prefill_pack_plan: which rows of a ragged first batch share a packed prefill pass (host arithmetic, no GPU). Returns
    (passes [n] — the row's pass or -1 for the equal-length groups —, row0 [n] — its first activation row in the pass —, n_passes)."""
    ln = np.ascontiguousarray(list(lengths), dtype=np.int32); n = int(ln.size)
    hp = None if hit_pages is None else np.ascontiguousarray(list(hit_pages), dtype=np.int32)
    assert hp is None or hp.size == n
    ps = np.full(max(n, 1), -1, dtype=np.int32); r0 = np.zeros(max(n, 1), dtype=np.int32); npass = ctypes.c_int32(0)
    i32 = lambda arr: arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    check(lib.q3_prefill_pack_plan(i32(ln) if n else None, None if hp is None else i32(hp), n, int(row_budget), int(bool(gemm_ok)), i32(ps), i32(r0),
                                   ctypes.byref(npass)))
    return ps[:n].tolist(), r0[:n].tolist(), int(npass.value)


ROWS_GATHER, ROWS_ASSEMBLE, ROWS_COPY, ROWS_SCATTER, ROWS_PUBLISH = 0, 1, 2, 3, 4
ROWS_GUARD = 64


def prompt_rows_ex(mode: int, *, out: Optional[np.ndarray] = None, cols: int = 0, table: Optional[np.ndarray] = None, ids=None,
                   src: Optional[np.ndarray] = None, text_row=None, codec_id=None, xvec: Optional[np.ndarray] = None, ref_codes=None,
                   cp_embs: Optional[np.ndarray] = None, dst_row=None, ent=None, n_rows: int = 0, ldd: int = 0, trail_len=None, text_ready=None,
                   limit=None, device: int = 0):
    """q3_prompt_rows_ex: ONE launch of a prompt-row kernel over host arrays (parity tests; include/q3tts.h describes the modes:
    ROWS_GATHER / ROWS_ASSEMBLE / ROWS_COPY / ROWS_SCATTER / ROWS_PUBLISH). `out` (flat f32) and the publish arrays (flat int32) carry
    ROWS_GUARD elements in front of and behind their payload and are written in place. Returns out, or (trail_len, text_ready, limit)."""
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    a = _lib.CPromptRowsEx()
    keep = []

    def put(name, arr, dtype, shape=None):
        if arr is None:
            return None
        arr = np.ascontiguousarray(arr, dtype=dtype)
        assert shape is None or arr.shape == shape, (name, arr.shape, shape)
        keep.append(arr); setattr(a, name, ptr(arr))
        return arr
    a.mode, a.cols, a.n_rows, a.ldd = mode, cols, n_rows, ldd
    payload = None
    if mode == ROWS_GATHER:
        t = put("table", table, np.uint16); i_ = put("ids", ids, np.uint32)
        assert t.ndim == 2 and t.shape[1] == cols and i_.ndim == 1
        a.n, a.n_table = i_.size, t.shape[0]; payload = i_.size * cols
    elif mode == ROWS_ASSEMBLE:
        r = put("src", src, np.float32); t = put("table", table, np.uint16)
        tr = put("text_row", text_row, np.int32); ci = put("codec_id", codec_id, np.int32)
        assert r.ndim == 2 and r.shape[1] == cols and t.ndim == 2 and t.shape[1] == cols and tr.ndim == 1 and ci.shape == tr.shape
        a.n, a.n_rows, a.n_table = tr.size, r.shape[0], t.shape[0]; payload = tr.size * cols
        put("xvec", xvec, np.float32, (cols,))
        rcod = put("ref_codes", ref_codes, np.uint32); ce = put("cp_embs", cp_embs, np.uint16)
        if rcod is not None:
            assert rcod.ndim == 2 and rcod.shape[1] == 16; a.n_ref = rcod.shape[0]
        if ce is not None:
            assert ce.ndim == 3 and ce.shape[0] == 15 and ce.shape[2] == cols; a.cp_vocab = ce.shape[1]
    elif mode == ROWS_COPY:
        s_ = put("src", src, np.float32); assert s_.ndim == 2
        a.n, a.lds = s_.shape[0], s_.shape[1]
        a.ldd = ldd if ldd else cols; payload = s_.shape[0] * a.ldd
    elif mode == ROWS_SCATTER:
        s_ = put("src", src, np.float32); d = put("dst_row", dst_row, np.int32)
        assert s_.ndim == 2 and s_.shape[1] == cols and d.shape == (s_.shape[0],)
        a.n = s_.shape[0]; payload = n_rows * cols
    else:
        e = put("ent", ent, np.int32); assert e.ndim == 2 and e.shape[1] == 4
        a.n = e.shape[0]
        for name, arr in (("trail_len", trail_len), ("text_ready", text_ready), ("limit", limit)):
            assert arr.dtype == np.int32 and arr.flags.c_contiguous and arr.shape == (n_rows + 2 * ROWS_GUARD,)
            setattr(a, name, ptr(arr))
        check(lib.q3_prompt_rows_ex(device, ctypes.byref(a)))
        return trail_len, text_ready, limit
    assert out is not None and out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (payload + 2 * ROWS_GUARD,), (out.shape, payload)
    a.out = ptr(out)
    check(lib.q3_prompt_rows_ex(device, ctypes.byref(a)))
    return out


def _vp(arr):
    return None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)


def attn_c_path(kernel: int = -1, hd: int = 64):
    """q3_attn_c_path: the kernel launch_attn_c runs (0 = k_attn_c, VALU; 1 = k_attn_c_mfma) for kernel -1 (the engine's pick) / 0 /
    1, or None for what the launcher refuses. No GPU needed."""
    k = lib.q3_attn_c_path(hd, kernel)
    return None if k < 0 else k


def attn_c_ex(mode: int, q_: np.ndarray, o: np.ndarray, *, nh: int, hd: int = 64, scale: Optional[float] = None, k: Optional[np.ndarray] = None,
              v: Optional[np.ndarray] = None, kernel: int = -1, window: int = 0, rows=None, caches: Optional[np.ndarray] = None, layer: int = 0,
              tabs=None, tab0=None, tab_n=None, device: int = 0) -> np.ndarray:
    """q3_attn_c_ex: one launch of the codec transformer's attention family (parity tests). mode 0 = launch_attn_c over q / k / v
    [nh*hd][L] (kernel -1 = the engine's pick, 0 VALU, 1 MFMA), 3 = launch_mimi_attn with `window`; 1 = launch_attn_cs: q / o
    [nh*hd][N], rows [(a0, e, qcol)], caches [n_rows][layers][2][nh*hd][cap]; 2 = launch_attn_cb: caches is the pool
    [n_blocks][layers][2][nh*hd][bf], row r's blocks are tabs[tab0[r] : tab0[r] + tab_n[r]]. o (f32, C order) is uploaded, written in
    place and returned whole. Raises Q3Error (status 1) for a shape the entry refuses."""
    qq = np.ascontiguousarray(q_, dtype=np.float32)
    assert qq.ndim == 2 and o.dtype == np.float32 and o.flags.c_contiguous and o.shape == qq.shape and qq.shape[0] == nh * hd
    a = _lib.CAttnCEx()
    a.mode, a.nh, a.hd, a.kernel, a.window, a.layer = mode, nh, hd, kernel, window, layer
    a.scale = float(hd) ** -0.5 if scale is None else scale
    keep = [qq]
    a.q, a.o = _vp(qq), _vp(o)
    if mode in (0, 3):
        a.L = qq.shape[1]
        kk = np.ascontiguousarray(k, dtype=np.float32); vv = np.ascontiguousarray(v, dtype=np.float32)
        assert kk.shape == qq.shape and vv.shape == qq.shape
        keep += [kk, vv]; a.k, a.v = _vp(kk), _vp(vv)
    elif mode in (1, 2):
        rr = np.ascontiguousarray(rows, dtype=np.int32); assert rr.ndim == 2 and rr.shape[1] == 3
        cc = np.ascontiguousarray(caches, dtype=np.float32); assert cc.ndim == 5 and cc.shape[2] == 2 and cc.shape[3] == nh * hd
        a.N, a.n_rows, a.layers, a.cap = qq.shape[1], rr.shape[0], cc.shape[1], cc.shape[4]
        keep += [rr, cc]; a.rows, a.caches = _vp(rr), _vp(cc)
        if mode == 2:
            tt = np.ascontiguousarray(tabs, dtype=np.int32); t0 = np.ascontiguousarray(tab0, dtype=np.int32); tn = np.ascontiguousarray(tab_n, dtype=np.int32)
            assert tt.ndim == 1 and t0.shape == (rr.shape[0],) and tn.shape == t0.shape
            a.n_blocks, a.n_tabs = cc.shape[0], tt.size
            keep += [tt, t0, tn]; a.tabs, a.tab0, a.tab_n = _vp(tt), _vp(t0), _vp(tn)
        else:
            assert cc.shape[0] == rr.shape[0]
    check(lib.q3_attn_c_ex(device, ctypes.byref(a)))
    return o


def rope_c_ex(q_: np.ndarray, k: np.ndarray, cs: np.ndarray, sn: np.ndarray, nh: int, pos=None, device: int = 0):
    """q3_rope_c_ex: launch_rope_c (pos None) / launch_rope_c_pos on copies of q and k [nh*hd][L]; cs / sn [n_pos][hd/2]. Returns
    the rotated (q, k)."""
    qq = np.array(q_, dtype=np.float32, order="C"); kk = np.array(k, dtype=np.float32, order="C")
    cs = np.ascontiguousarray(cs, dtype=np.float32); sn = np.ascontiguousarray(sn, dtype=np.float32)
    assert qq.ndim == 2 and kk.shape == qq.shape and qq.shape[0] % nh == 0 and cs.ndim == 2 and sn.shape == cs.shape
    hd = qq.shape[0] // nh; assert cs.shape[1] * 2 == hd
    pp = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
    assert pp is None or pp.shape == (qq.shape[1],)
    check(lib.q3_rope_c_ex(device, _vp(qq), _vp(kk), _vp(cs), _vp(sn), _vp(pp), nh, hd, qq.shape[1], cs.shape[0]))
    return qq, kk


def copy_cols_ex(src: np.ndarray, dst: np.ndarray, C: int, s_off, d_off, sp, dp, src_off: int = 0, dst_off: int = 0, device: int = 0) -> np.ndarray:
    """q3_copy_cols_ex: one launch_copy_cols over flat f32 buffers; column j: dst[dst_off + d_off[j] + c * dp[j]] = src[src_off +
    s_off[j] + c * sp[j]], c < C, or 0 for s_off[j] < 0. dst is written in place and returned."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    assert dst.dtype == np.float32 and dst.flags.c_contiguous and dst.ndim == 1 and src.ndim == 1
    so = np.ascontiguousarray(s_off, dtype=np.int64); do = np.ascontiguousarray(d_off, dtype=np.int64)
    spp = np.ascontiguousarray(sp, dtype=np.int32); dpp = np.ascontiguousarray(dp, dtype=np.int32)
    n = so.size; assert do.shape == (n,) and spp.shape == (n,) and dpp.shape == (n,)
    check(lib.q3_copy_cols_ex(device, _vp(src), src.size, _vp(dst), dst.size, n, C, _vp(so), _vp(do), _vp(spp), _vp(dpp), src_off, dst_off))
    return dst


def copy_segs_ex(src: np.ndarray, dst: np.ndarray, segs, device: int = 0) -> np.ndarray:
    """q3_copy_segs_ex: one launch_copy_segs; segs [(src offset, dst offset, n)] in floats. dst is written in place and returned."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    assert dst.dtype == np.float32 and dst.flags.c_contiguous and dst.ndim == 1 and src.ndim == 1
    sg = np.ascontiguousarray(segs, dtype=np.uint64); assert sg.ndim == 2 and sg.shape[1] == 3
    check(lib.q3_copy_segs_ex(device, _vp(src), src.size, _vp(dst), dst.size, sg.shape[0], _vp(sg)))
    return dst


def gather_frames_ex(src: np.ndarray, s_off, dst: np.ndarray, device: int = 0) -> np.ndarray:
    """q3_gather_frames_ex: one launch_gather_frames; frame j = src[s_off[j] : s_off[j] + 16] (u32) to dst[16 j ..]."""
    src = np.ascontiguousarray(src, dtype=np.uint32)
    assert dst.dtype == np.uint32 and dst.flags.c_contiguous and dst.ndim == 1 and src.ndim == 1
    so = np.ascontiguousarray(s_off, dtype=np.int64); assert so.ndim == 1
    check(lib.q3_gather_frames_ex(device, _vp(src), src.size, _vp(so), so.size, _vp(dst), dst.size))
    return dst


def rvq_embed_ex(frames: np.ndarray, first_cb: np.ndarray, rest_cbs: np.ndarray, first_out: np.ndarray, rest_out: np.ndarray, out_front: int = 0,
                 device: int = 0):
    """q3_rvq_embed_ex: one launch_rvq_embed; frames [n][16] u32, first_cb [cb_size][cb_dim], rest_cbs [15][cb_size][cb_dim]; the two
    flat f32 outputs hold [cb_dim][n] at out_front, are written in place and returned."""
    fr = np.ascontiguousarray(frames, dtype=np.uint32); assert fr.ndim == 2 and fr.shape[1] == 16
    fc = np.ascontiguousarray(first_cb, dtype=np.float32); rc = np.ascontiguousarray(rest_cbs, dtype=np.float32)
    assert fc.ndim == 2 and rc.shape == (15,) + fc.shape
    for buf in (first_out, rest_out):
        assert buf.dtype == np.float32 and buf.flags.c_contiguous and buf.ndim == 1 and buf.size == first_out.size
    check(lib.q3_rvq_embed_ex(device, _vp(fr), fr.shape[0], _vp(fc), _vp(rc), fc.shape[1], fc.shape[0], _vp(first_out), _vp(rest_out), out_front,
                              first_out.size))
    return first_out, rest_out


def silu_mul_ex(g: np.ndarray, u: np.ndarray, y: np.ndarray, device: int = 0) -> np.ndarray:
    """q3_silu_mul_ex: one launch_silu_mul over g, u [n]; y (flat f32, >= n) is written in place and returned whole."""
    g = np.ascontiguousarray(g, dtype=np.float32); u = np.ascontiguousarray(u, dtype=np.float32)
    assert g.ndim == 1 and u.shape == g.shape and y.dtype == np.float32 and y.flags.c_contiguous and y.ndim == 1
    check(lib.q3_silu_mul_ex(device, _vp(g), _vp(u), _vp(y), g.size, y.size))
    return y


SPK_PAD, SPK_COLS, SPK_MEAN, SPK_SE_APPLY, SPK_ASP_IN, SPK_ASP_POOL = range(6)      # ops of q3_spk_op_ex
MIMI_ELU, MIMI_FOLD, MIMI_CODEBOOK = range(3)                                       # ops of q3_mimi_op_ex


def _clone_op(args, call, a, b, out, out_front, device):
    aa = np.ascontiguousarray(a, dtype=np.float32)
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.float32)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.ndim == 1
    args.a_elems, args.b_elems, args.out_front, args.out_elems = aa.size, 0 if bb is None else bb.size, out_front, out.size
    args.a, args.b, args.out = _vp(aa), _vp(bb), _vp(out)
    check(call(device, ctypes.byref(args)))
    return out


def spk_op_ex(op: int, a: np.ndarray, out: np.ndarray, *, C: int, T: int, b: Optional[np.ndarray] = None, pl: int = 0, Tp: int = 0, ld: int = 0,
              off: int = 0, out_front: int = 0, device: int = 0) -> np.ndarray:
    """q3_spk_op_ex: one launch of a speaker-encoder kernel (op = SPK_PAD: a [C][T] (+ b) -> [C][Tp] with pl columns on the left; SPK_COLS:
    a [C][ld] -> [C][T] from column off; SPK_MEAN: a [C][T] -> [C]; SPK_SE_APPLY: a = o, b = g [C], out holds h; SPK_ASP_IN: a -> [3C][T];
    SPK_ASP_POOL: a = logits, b = m -> [2C]). out: flat f32 with the result at out_front, uploaded, written in place and returned whole.
    Raises Q3Error (status 1) for a shape the entry refuses."""
    args = _lib.CSpkOpEx()
    args.op, args.C, args.T, args.pl, args.Tp, args.ld, args.off = op, C, T, pl, Tp, ld, off
    return _clone_op(args, lib.q3_spk_op_ex, a, b, out, out_front, device)


def mimi_op_ex(op: int, a: np.ndarray, out: np.ndarray, *, L: int, C: int = 1, r: int = 1, Lf: int = 0, elu: bool = False, replicate: bool = False,
               b: Optional[np.ndarray] = None, out_front: int = 0, device: int = 0) -> np.ndarray:
    """q3_mimi_op_ex: one launch of a speech-encoder kernel (op = MIMI_ELU: a [L] -> [L]; MIMI_FOLD: a [C][L] -> [C*r][Lf (+ 1 in
    replicate mode)]; MIMI_CODEBOOK: a = embed_sum [C][L], b = cluster_usage [C] -> [C][L]). out as in spk_op_ex."""
    args = _lib.CMimiOpEx()
    args.op, args.C, args.L, args.r, args.Lf, args.elu, args.replicate = op, C, L, r, Lf, int(elu), int(replicate)
    return _clone_op(args, lib.q3_mimi_op_ex, a, b, out, out_front, device)


def mimi_rvq_ex(proj: np.ndarray, books: np.ndarray, codes: np.ndarray, q0: int = 0, device: int = 0) -> np.ndarray:
    """q3_mimi_rvq_ex: one launch_mimi_rvq; proj [CD][T], books [n_layers][CB][CD], codes [T][n_q] u32: columns q0 .. q0 + n_layers - 1
    are written in place, the array is returned whole."""
    pp = np.ascontiguousarray(proj, dtype=np.float32); bk = np.ascontiguousarray(books, dtype=np.float32)
    assert pp.ndim == 2 and bk.ndim == 3 and bk.shape[2] == pp.shape[0]
    assert codes.dtype == np.uint32 and codes.flags.c_contiguous and codes.ndim == 2 and codes.shape[0] == pp.shape[1]
    check(lib.q3_mimi_rvq_ex(device, _vp(pp), pp.shape[1], _vp(bk), bk.shape[0], bk.shape[1], bk.shape[2], _vp(codes), codes.shape[1], q0))
    return codes


def resunit_path(C: int, L: int, dil: int, packed: bool = True, ya_is_xa: bool = False, planes: int = 3) -> int:
    """q3_resunit_path: launch_resunit's acceptance rule as a ConvPath code (0 = refused). No GPU needed."""
    return lib.q3_resunit_path(C, L, dil, int(packed), int(ya_is_xa), planes)


def conv_path_name(code: int) -> str:
    return lib.q3_conv_path_name(code).decode()


def conv_ex(kind: int, x: np.ndarray, w: np.ndarray, *, dil: int = 1, stride: int = 1, b: Optional[np.ndarray] = None, snake=None,
            post=None, mid=None, resid: Optional[np.ndarray] = None, resid_in_place: bool = False, scale: Optional[np.ndarray] = None,
            act: int = 0, planes: int = 3, packed: bool = True, snake_raw: bool = False, w2: Optional[np.ndarray] = None,
            b2: Optional[np.ndarray] = None, y: Optional[np.ndarray] = None, y2: Optional[np.ndarray] = None, y_front: int = 0,
            y2_is_x: bool = False, device: int = 0, resident: Optional[int] = None):
    """q3_conv_ex: one launch of the vocoder conv family (parity tests). kind 0 = causal conv (w [cout][cin][k]), 1 = transposed conv
    (w [cin][cout][k], k = stride * taps), 2 = residual unit (w [C][C][7], w2 [C][C], y holds the raw tensor and is updated in place).
    x [cin][L]. snake / post / mid: pairs of [C] arrays — (a, 1/b) tables, or (alpha, beta) with snake_raw. y / y2: flat f32 buffers
    whose result starts at y_front; uploaded, written in place and returned whole (y defaults to zeros without guards). Returns
    (y, y2, path). Raises Q3Error (status 7, with .path) when the launcher refuses the arguments.
    resident = n (q3_test_conv_resident): the same launch under a residency cap of n workgroups per CU (0 = none); returns
    (y, y2, path, lds_bytes) with the dynamic LDS the launch asked for."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    x = f(x); w = f(w)
    assert x.ndim == 2 and w.ndim == 3
    cin, L = x.shape
    cout = w.shape[1] if kind == 1 else w.shape[0]
    assert (w.shape[0] if kind == 1 else w.shape[1]) == cin
    a = _lib.CConvEx()
    a.kind, a.cin, a.cout, a.L, a.k, a.dil, a.stride = kind, cin, cout, L, w.shape[2], dil, stride
    a.act, a.planes, a.packed, a.resid_in_place, a.snake_raw, a.y2_is_x = act, planes, int(packed), int(resid_in_place), int(snake_raw), int(y2_is_x)
    n_out = cout * L * (stride if kind == 1 else 1)
    if y is None:
        y = np.zeros(n_out, dtype=np.float32); y_front = 0
    for buf in (y, y2):
        assert buf is None or (buf.dtype == np.float32 and buf.flags.c_contiguous and buf.ndim == 1 and buf.size == y.size)
    a.y_front, a.y_elems = y_front, y.size
    path = ctypes.c_int32(0)
    a.path = ctypes.pointer(path)
    keep = [x, w]
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    a.x, a.w, a.y = ptr(x), ptr(w), ptr(y)
    if y2 is not None:
        a.y2 = ptr(y2)

    def opt(name, arr, n):
        if arr is not None:
            arr = f(arr); assert arr.size == n, (name, arr.size, n)
            keep.append(arr); setattr(a, name, ptr(arr))
    opt("b", b, cout); opt("b2", b2, cout); opt("scale", scale, cout); opt("resid", resid, n_out)
    if w2 is not None:
        opt("w2", w2, cout * cin)
    for (na, nb, pr, n) in (("snake_a", "snake_b", snake, cin), ("post_a", "post_ib", post, cout), ("mid_a", "mid_ib", mid, cout)):
        if pr is not None:
            opt(na, pr[0], n); opt(nb, pr[1], n)
    lds = ctypes.c_int32(0)
    try:
        if resident is None:
            check(lib.q3_conv_ex(device, ctypes.byref(a)))
        else:
            check(lib.q3_test_conv_resident(device, ctypes.byref(a), int(resident), ctypes.byref(lds)))
    except _lib.Q3Error as e:
        e.path = path.value
        raise
    return (y, y2, path.value) if resident is None else (y, y2, path.value, lds.value)


def norm_c(x: np.ndarray, w: np.ndarray, b: Optional[np.ndarray] = None, eps: float = 1e-6, y: Optional[np.ndarray] = None,
           y_front: int = 0, device: int = 0) -> np.ndarray:
    """q3_norm_c: LayerNorm (b given) / RMSNorm over the channels of x [C][L]; y as in conv_ex."""
    x = np.ascontiguousarray(x, dtype=np.float32); C, L = x.shape
    w = np.ascontiguousarray(w, dtype=np.float32); assert w.shape == (C,)
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.float32)
    if y is None:
        y = np.zeros(C * L, dtype=np.float32); y_front = 0
    assert y.dtype == np.float32 and y.flags.c_contiguous and y.ndim == 1
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    check(lib.q3_norm_c(device, 0 if bb is None else 1, ptr(x), ptr(w), None if bb is None else ptr(bb), C, L, eps, ptr(y), y_front, y.size))
    return y


def dwconv7(x: np.ndarray, w: np.ndarray, b: np.ndarray, y: Optional[np.ndarray] = None, y_front: int = 0, device: int = 0) -> np.ndarray:
    """q3_dwconv7: depthwise causal conv with 7 taps, x [C][L], w [C][7], b [C]; y as in conv_ex."""
    x = np.ascontiguousarray(x, dtype=np.float32); C, L = x.shape
    w = np.ascontiguousarray(w, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
    assert w.shape == (C, 7) and b.shape == (C,)
    if y is None:
        y = np.zeros(C * L, dtype=np.float32); y_front = 0
    assert y.dtype == np.float32 and y.flags.c_contiguous and y.ndim == 1
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    check(lib.q3_dwconv7(device, ptr(x), ptr(w), ptr(b), C, L, ptr(y), y_front, y.size))
    return y


def _io(arr, dtype, n, name):
    """a caller's in/out buffer: flat, C order, exactly n elements of dtype (written in place)"""
    assert isinstance(arr, np.ndarray) and arr.dtype == dtype and arr.flags.c_contiguous and arr.ndim == 1 and arr.size == n, (name, n)
    return _vp(arr)


def prompt_shape(u: Utterance, options: SynthesisOptions, n_text: Optional[int] = None, tables: bool = False):
    """q3_prompt_shape: the prompt layout a session derives from a request (host only) — the record and, with `tables`, per prefill
    position the projected text row and the codec embedding (-1: none, -2: the x-vector, -3 - i: reference frame i), row base 0.
    n_text: the text tokens counted (default: the utterance's own; an open row's text so far)."""
    r = CRequest(); keep = []; rec = _lib.CPromptShape()
    fill_request(r, u, options, keep)
    n = r.n_text if n_text is None else int(n_text)
    check(lib.q3_prompt_shape(ctypes.byref(r), n, ctypes.byref(rec), None, None, 0))
    if not tables:
        return rec
    tr = np.zeros(rec.prefill_len, np.int32); ci = np.zeros(rec.prefill_len, np.int32)
    check(lib.q3_prompt_shape(ctypes.byref(r), n, ctypes.byref(rec), tr.ctypes.data_as(ctypes.c_void_p), ci.ctypes.data_as(ctypes.c_void_p), rec.prefill_len))
    return rec, tr, ci


def sample_row(options: SynthesisOptions) -> "_lib.CSampleRow":
    """q3_sample_row: the sampler's per-row record as a session derives it from a request's options (host only)."""
    r = _lib.CSampleRow(); o = options.to_c()
    check(lib.q3_sample_row(ctypes.byref(o), ctypes.byref(r)))
    return r


def sample_ex(logits: np.ndarray, u: np.ndarray, vocab: int, tok: np.ndarray, scalar, *, rows=None, seen: Optional[np.ndarray] = None,
              u_stride: int = 1, draw_idx=None, token_count: Optional[np.ndarray] = None, token_count_static: int = 0, advance: bool = False,
              frame_idx: Optional[np.ndarray] = None, pos: Optional[np.ndarray] = None, limit=None, text_ready=None,
              logits_hist: Optional[np.ndarray] = None, hist_stride_b: int = 0, hist_cap: int = 0, codec_eos: int = 2150,
              use_suppress: bool = True, guard: int = 0, device: int = 0) -> np.ndarray:
    """q3_sample_ex: ONE launch_sample through a complete SampleArgs. logits [B][ld] (ld >= vocab), u flat, scalar / rows[b]:
    CSampleRow records (sample_row()). The in/out buffers are flat arrays with `guard` elements on both sides of the payload and are
    written in place: tok u32 [B], seen u8 [B * vocab], token_count / frame_idx / pos i32 [B], logits_hist f32 [B * hist_stride_b].
    Returns tok. Raises Q3Error (status 1) for arguments the entry refuses."""
    lg = np.ascontiguousarray(logits, dtype=np.float32); assert lg.ndim == 2
    B, ld = lg.shape
    uu = np.ascontiguousarray(u, dtype=np.float32).reshape(-1)
    a = _lib.CSampleEx()
    a.B, a.vocab, a.ld, a.u_stride, a.u_elems, a.advance, a.token_count_static = B, vocab, ld, u_stride, uu.size, int(advance), token_count_static
    a.hist_stride_b, a.hist_cap, a.codec_eos, a.use_suppress, a.guard = hist_stride_b, hist_cap, codec_eos, int(use_suppress), guard
    a.scalar = scalar
    keep = [lg, uu]
    a.logits, a.u = _vp(lg), _vp(uu)
    a.tok = _io(tok, np.uint32, B + 2 * guard, "tok")
    if seen is not None:
        a.seen = _io(seen, np.uint8, B * vocab + 2 * guard, "seen")
    for name, arr in (("token_count", token_count), ("frame_idx", frame_idx), ("pos", pos)):
        if arr is not None:
            setattr(a, name, _io(arr, np.int32, B + 2 * guard, name))
    if logits_hist is not None:
        a.logits_hist = _io(logits_hist, np.float32, B * hist_stride_b + 2 * guard, "logits_hist")
    for name, arr in (("draw_idx", draw_idx), ("limit", limit), ("text_ready", text_ready)):
        if arr is not None:
            v = np.ascontiguousarray(arr, dtype=np.int32); assert v.shape == (B,), name
            keep.append(v); setattr(a, name, _vp(v))
    if rows is not None:
        assert len(rows) == B
        rr = (_lib.CSampleRow * B)(*rows); keep.append(rr)
        a.rows = ctypes.cast(rr, ctypes.c_void_p)
    check(lib.q3_sample_ex(device, ctypes.byref(a)))
    return tok


def frame_embed_ex(codec_emb: np.ndarray, cp_embs: np.ndarray, tok, cp_logits_last: np.ndarray, codes: np.ndarray, frame_idx, max_frames: int,
                   text_rows: np.ndarray, trail_base, trail_len, pad_row, out: np.ndarray, text_ready=None, guard: int = 0, device: int = 0):
    """q3_frame_embed_ex: ONE launch_frame_embed. codec_emb [n_sem][H] / cp_embs [15][cp_vocab][H] bf16 bits (u16), tok [B], cp_logits_last
    [B][cp_vocab], text_rows [n][H] f32, per-row i32 lists. codes (u32, flat, guard + B * max_frames * 16 + guard) and out (f32, flat,
    guard + B * H + guard) are written in place. Returns (out, codes)."""
    ce = np.ascontiguousarray(codec_emb, dtype=np.uint16); pe = np.ascontiguousarray(cp_embs, dtype=np.uint16)
    lg = np.ascontiguousarray(cp_logits_last, dtype=np.float32); tx = np.ascontiguousarray(text_rows, dtype=np.float32)
    assert ce.ndim == 2 and pe.ndim == 3 and pe.shape[0] == 15 and pe.shape[2] == ce.shape[1] and lg.ndim == 2 and lg.shape[1] == pe.shape[1]
    assert tx.ndim == 2 and tx.shape[1] == ce.shape[1]
    B, H = lg.shape[0], ce.shape[1]
    a = _lib.CFrameEmbedEx()
    a.B, a.H, a.n_sem, a.cp_vocab, a.max_frames, a.n_text_rows, a.guard = B, H, ce.shape[0], pe.shape[1], max_frames, tx.shape[0], guard
    tk = np.ascontiguousarray(tok, dtype=np.uint32); assert tk.shape == (B,)
    keep = [ce, pe, lg, tx, tk]
    a.codec_emb, a.cp_embs, a.cp_logits_last, a.text_rows, a.tok = _vp(ce), _vp(pe), _vp(lg), _vp(tx), _vp(tk)
    for name, arr in (("frame_idx", frame_idx), ("trail_base", trail_base), ("trail_len", trail_len), ("pad_row", pad_row), ("text_ready", text_ready)):
        if arr is not None:
            v = np.ascontiguousarray(arr, dtype=np.int32); assert v.shape == (B,), name
            keep.append(v); setattr(a, name, _vp(v))
    a.codes = _io(codes, np.uint32, B * max_frames * 16 + 2 * guard, "codes")
    a.out = _io(out, np.float32, B * H + 2 * guard, "out")
    check(lib.q3_frame_embed_ex(device, ctypes.byref(a)))
    return out, codes


def cp_gather_ex(pass_: int, out: np.ndarray, ld_out: int, B: int, H: int, *, last_hidden=None, codec_emb=None, tok=None, cp_emb=None,
                 cp_logits=None, proj_tab=None, qkv_tab=None, qkv_out: Optional[np.ndarray] = None, ld_qkv_out: int = 0,
                 codes: Optional[np.ndarray] = None, frame_idx=None, max_frames: int = 0, guard: int = 0, device: int = 0):
    """q3_cp_gather_ex: ONE launch_cp_gather for pass `pass_`. Tables: codec_emb [n_sem][H] / cp_emb [cp_vocab][H] bf16 bits, proj_tab
    [rows][proj_dim] / qkv_tab [rows][qkv_dim] f32. out (f32, flat, guard + B * ld_out + guard), qkv_out (guard + B * ld_qkv_out + guard)
    and codes (u32, guard + B * max_frames * 16 + guard) are written in place. Returns (out, qkv_out, codes)."""
    a = _lib.CCpGatherEx()
    a.pass_, a.B, a.H, a.max_frames, a.ld_out, a.ld_qkv_out, a.guard = pass_, B, H, max_frames, ld_out, ld_qkv_out, guard
    keep = []

    def put(name, arr, dtype, ndim):
        if arr is None:
            return None
        v = np.ascontiguousarray(arr, dtype=dtype); assert v.ndim == ndim, name
        keep.append(v); setattr(a, name, _vp(v))
        return v
    put("last_hidden", last_hidden, np.float32, 2)
    ce = put("codec_emb", codec_emb, np.uint16, 2); pe = put("cp_emb", cp_emb, np.uint16, 2)
    put("tok", tok, np.uint32, 1); lg = put("cp_logits", cp_logits, np.float32, 2); put("frame_idx", frame_idx, np.int32, 1)
    pt = put("proj_tab", proj_tab, np.float32, 2); qt = put("qkv_tab", qkv_tab, np.float32, 2)
    tabs = [t for t in (pt, qt, ce if pass_ == 1 else pe) if t is not None]
    n_rows = tabs[0].shape[0] if tabs else 0
    assert all(t.shape[0] == n_rows for t in tabs)
    a.n_sem = n_rows if pass_ == 1 else 0
    a.cp_vocab = lg.shape[1] if lg is not None else 0
    assert pass_ < 2 or not tabs or n_rows == a.cp_vocab
    a.proj_dim = 0 if pt is None else pt.shape[1]; a.qkv_dim = 0 if qt is None else qt.shape[1]
    a.out = _io(out, np.float32, B * ld_out + 2 * guard, "out")
    if qkv_out is not None:
        a.qkv_out = _io(qkv_out, np.float32, B * ld_qkv_out + 2 * guard, "qkv_out")
    if codes is not None:
        a.codes = _io(codes, np.uint32, B * max_frames * 16 + 2 * guard, "codes")
    check(lib.q3_cp_gather_ex(device, ctypes.byref(a)))
    return out, qkv_out, codes


def rmsnorm_ex(x: np.ndarray, w: np.ndarray, y: np.ndarray, rows: int, cols: int, *, x_off: int = 0, ldx: Optional[int] = None, y_front: int = 0,
               ldy: Optional[int] = None, eps: float = 1e-6, frame_idx=None, text_ready=None, device: int = 0) -> np.ndarray:
    """q3_rmsnorm_ex: ONE launch_rmsnorm (or launch_rmsnorm_hold with frame_idx / text_ready [rows]): row r reads x[x_off + r * ldx ..
    + cols) and writes y[y_front + r * ldy ..). x, y: flat f32; y is written in place and returned whole."""
    xx = np.ascontiguousarray(x, dtype=np.float32).reshape(-1); ww = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    assert y.dtype == np.float32 and y.flags.c_contiguous and y.ndim == 1
    fi = None if frame_idx is None else np.ascontiguousarray(frame_idx, dtype=np.int32)
    tr = None if text_ready is None else np.ascontiguousarray(text_ready, dtype=np.int32)
    check(lib.q3_rmsnorm_ex(device, _vp(xx), xx.size, x_off, cols if ldx is None else ldx, _vp(ww), _vp(y), y.size, y_front,
                            cols if ldy is None else ldy, rows, cols, eps, _vp(fi), _vp(tr)))
    return y


def sample(logits: np.ndarray, u: np.ndarray, options: SynthesisOptions, seen: Optional[np.ndarray] = None,
           token_count: int = -1, device: int = 0) -> np.ndarray:
    """apply_generation_penalties + sample on the GPU (token_count < 0: plain `sample`, sampling.rs:140)."""
    lg = np.ascontiguousarray(logits, dtype=np.float32); rows, vocab = lg.shape
    uu = np.ascontiguousarray(u, dtype=np.float32)
    out = np.zeros(rows, dtype=np.uint32)
    o = options.to_c()
    sn = None if seen is None else np.ascontiguousarray(seen, dtype=np.uint8)
    check(lib.q3_sample(device, lg.ctypes.data_as(ctypes.c_void_p), None if sn is None else sn.ctypes.data_as(ctypes.c_void_p),
                        uu.ctypes.data_as(ctypes.c_void_p), rows, vocab, ctypes.byref(o), token_count,
                        out.ctypes.data_as(ctypes.c_void_p)))
    return out


def bench_linear(M: int, N: int, K: int, epi: int = 0, rms=False, tiled: int = -1, iters: int = 200,
                 n_copies: int = 0, device: int = 0) -> float:
    """µs per launch of one GEMV shape: mean over 5 hipGraph replays of `iters` launches cycling over HBM-resident weight
    copies. rms: fused input RMSNorm (norm weight applied in the kernel) or none."""
    nbytes = N * K * 2 * (2 if epi == 3 else 1)
    if n_copies <= 0:
        n_copies = max(2, int(600e6 // nbytes))
    us = ctypes.c_double()
    check(lib.q3_bench_linear(device, M, N, K, epi, 1 if rms else 0, tiled, iters, n_copies, ctypes.byref(us)))
    return us.value


def auto_device() -> int:
    """auto_device (lib.rs:1854-1926): this build has exactly one backend — an MI355X. No CPU path."""
    n = lib.q3_device_count()
    if n <= 0:
        raise RuntimeError("no HIP device visible: the MI355X-native build has no CPU fallback")
    return 0


def row_move(src: np.ndarray, dst: np.ndarray, segments, device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """One launch of the row-state kernel over host byte buffers (q3_row_move, test API of Session.park_row / resume_row).
    segments: (src_offset, dst_offset, n_bytes, mode) with mode 0 = copy src -> dst, 1 = exchange. Returns (src, dst) after it."""
    a = np.ascontiguousarray(src, dtype=np.uint8).reshape(-1).copy()
    b = np.ascontiguousarray(dst, dtype=np.uint8).reshape(-1).copy()
    n = len(segments)
    so = (ctypes.c_size_t * n)(*[int(g[0]) for g in segments]); do = (ctypes.c_size_t * n)(*[int(g[1]) for g in segments])
    nb = (ctypes.c_size_t * n)(*[int(g[2]) for g in segments]); md = (ctypes.c_int * n)(*[int(g[3]) for g in segments])
    check(lib.q3_row_move(int(device), a.ctypes.data_as(ctypes.c_void_p), a.size, b.ctypes.data_as(ctypes.c_void_p), b.size, n, so, do, nb, md))
    return a, b
