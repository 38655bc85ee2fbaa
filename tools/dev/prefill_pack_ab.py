"""Packed prefill of a ragged first batch against the grouped path: the 1.7B synthetic model, sessions of 4, 8 and 16
requests — half VoiceDesign, half ICL voice clones, every prefill length different, about 100 .. 700 positions (printed).
  arm parent  a build of the parent commit (`--parent-root DIR`: a checkout with its own libq3tts.so; groups only)
  arm off     this build with Q3_PREFILL_PACK=0 (the grouped path: it must not have moved)
  arm pack    this build as it is
Timed on the host clock: `prefill` = q3_session_prefill from the call to its return (it ends in a stream synchronise); `first audio`
= Session.run of the same rows at max_length = 4 frames (prefill, four frames, vocoder: the first audio a run hands out). Every arm
is ONE worker process that keeps its model; the driver alternates the arms per repetition, after a warm-up of every arm and mix.
Uses only calls the parent build has. Prints a table; `--out PATH` also writes it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

MIXES = {
    4: dict(vd=(150, 500), icl=(300, 640)),
    8: dict(vd=(100, 270, 440, 610), icl=(180, 350, 520, 680)),
    16: dict(vd=tuple(range(100, 700, 80)), icl=tuple(range(140, 740, 80))),
}


def worker(root):
    sys.path.insert(0, os.path.abspath(root))
    import qwen3_tts_rs_amd as q
    from qwen3_tts_rs_amd import synth

    cfg = q.qwen3_tts_1_7b()
    gm = q.Qwen3TTS.from_synthetic(cfg, seed=synth.DEFAULT_SEED)
    rng = np.random.default_rng(3)
    xv = rng.standard_normal(cfg.hidden).astype(np.float32)
    ids = lambda n, salt: ((np.arange(n) * 7919 + salt * 104729) % 20000 + 1000).astype(np.uint32)

    def rows(k):
        m = MIXES[k]; out = []
        for i, (a, b) in enumerate(zip(m["vd"], m["icl"])):      # VoiceDesign and ICL rows alternate
            out.append(q.Utterance(ids(12, i), language=q.Language.German, instruct_ids=ids(a, 50 + i), seed=20 + i))
            ref = rng.integers(0, 2048, size=(b, 16)).astype(np.uint32)
            out.append(q.Utterance(ids(11, 30 + i), language=q.Language.French, xvector=xv, ref_codes=ref, ref_text_ids=ids(3, 90 + i), seed=40 + i))
        return out
    utts = {k: rows(k) for k in MIXES}
    opts = q.SynthesisOptions(max_length=4, eos_token_id=None, seed=1)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        k = int(cmd[1])
        s = gm.session(utts[k], opts)
        if cmd[0] == "lens":
            print(json.dumps([s.prefill_len(b)[0] for b in range(k)]), flush=True)
        elif cmd[0] == "prefill":
            t0 = time.perf_counter(); s.prefill(); ms = (time.perf_counter() - t0) * 1e3
            info = s.prefill_info() if hasattr(s, "prefill_info") else {}
            print(json.dumps(dict(ms=ms, info=info)), flush=True)
        else:
            t0 = time.perf_counter(); s.run(); ms = (time.perf_counter() - t0) * 1e3
            print(json.dumps(dict(ms=ms)), flush=True)
        s.close()
    gm.close()


def fmt(v):
    return f"{np.median(v):7.2f} ({np.min(v):.2f} .. {np.max(v):.2f})"


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit with its own build (arm parent)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    root = os.path.join(here, "..", "..")
    arms = ([("parent", args.parent_root, {})] if args.parent_root else []) + [("off", root, {"Q3_PREFILL_PACK": "0"}), ("pack", root, {})]
    procs = {}
    for name, r, env in arms:
        e = dict(os.environ); e.pop("Q3_PREFILL_PACK", None); e.update(env)
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", r], env=e, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(name, what, k):
        p = procs[name]
        p.stdin.write(f"{what} {k}\n"); p.stdin.flush()
        line = p.stdout.readline()
        if not line:
            raise RuntimeError(f"arm {name} ended (exit {p.poll()})")
        return json.loads(line)
    try:
        lens = {k: ask("pack", "lens", k) for k in MIXES}
        for name, _, _ in arms:                                   # warm-up: code objects, workspaces, the size-class cache
            for k in MIXES:
                for what in ("prefill", "run"):
                    ask(name, what, k)
        acc = {(name, k, what): [] for name, _, _ in arms for k in MIXES for what in ("prefill", "run")}
        info = {}
        for rep in range(args.reps):
            for k in MIXES:
                for what in ("prefill", "run"):
                    for name, _, _ in arms:                       # the arms alternate
                        r = ask(name, what, k)
                        acc[(name, k, what)].append(r["ms"])
                        if what == "prefill":
                            info[(name, k)] = r["info"]
            print(f"repetition {rep} done", file=sys.stderr, flush=True)
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n"); p.stdin.flush()
            except Exception:
                pass
        for p in procs.values():
            p.wait(timeout=120)
    lines = [f"prefill_pack_ab: 1.7B synthetic, ragged first batch, {args.reps} repetitions per arm (alternated), ms: median (min .. max)"]
    for k in MIXES:
        lines.append(f"{k} rows, prefill lengths {lens[k]} (sum {sum(lens[k])}); pack arm: {info.get(('pack', k))}")
        for what, title in (("prefill", "q3_session_prefill"), ("run", "first audio (run, 4 frames)")):
            row = f"  {title:28s}"
            for name, _, _ in arms:
                row += f"  {name}: {fmt(acc[(name, k, what)])}"
            base = "parent" if args.parent_root else "off"
            b, p = np.array(acc[(base, k, what)]), np.array(acc[("pack", k, what)])
            row += f"  pack / {base}: {np.median(p) / np.median(b):.3f}; every pack repeat faster than every {base} repeat: {'yes' if p.max() < b.min() else 'NO'}"
            lines.append(row)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
