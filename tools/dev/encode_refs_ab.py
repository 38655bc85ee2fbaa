"""Many reference clips per encoder pass: a 1.7B-width synthetic speaker encoder and the full Mimi configuration on
sets of 1, 2, 4, 8 and 16 clips drawn from 10 s, 3 s and 5 s (in that order, repeating), already on the device as RefAudio objects:
  leg a  a loop of encode_ref over the clips (one pass of the encoder per clip)
  leg b  one encode_refs over the clips (one packed pass)
Each leg is timed per encoder on the host clock around calls that end in a device synchronise. After a warm-up of every leg and
set the legs alternate in one process, five repetitions; median (minimum .. maximum) in ms, clips per second from the median, and
the ratio b / a per repetition.

`--root DIR` imports the package from another checkout (a build of the parent commit, which has leg a only: `--legs a`), `--json
PATH` writes the samples, and `--parent-json PATH` reads such a file of the parent build from the same visit and reports leg b
against ITS leg a, beside this build's own. Prints a table; `--out PATH` also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

SETS, DURS, REPS = (1, 2, 4, 8, 16), (10, 3, 5), 5


def fmt_stat(v):
    return f"{np.median(v):8.2f} ({np.min(v):.2f} .. {np.max(v):.2f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."), help="checkout to import the package from")
    ap.add_argument("--legs", choices=["ab", "a"], default="ab")
    ap.add_argument("--label", default="this build", help="what the table's first line calls the build")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--json", default=None, help="write every sample to this file")
    ap.add_argument("--parent-json", default=None, help="samples of a --legs a run of the parent build")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import qwen3_tts_rs_amd as q
    from qwen3_tts_rs_amd import api

    spk = q.SpeakerEncoder.from_synthetic(q.SpeakerEncoderConfig(enc_dim=2048))
    mimi = q.SpeechEncoder.from_synthetic(None)
    rng = np.random.default_rng(11)
    clips = []
    for i in range(max(SETS)):
        n = 24000 * DURS[i % len(DURS)]
        t = np.arange(n) / 24000.0
        x = 0.3 * np.sin(2 * np.pi * (150.0 + 13 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.3 * t)) + 0.05 * rng.standard_normal(n)
        clips.append((x.astype(np.float32), 24000, "f32"))
    refs = api.RefAudio.many(clips)

    def leg_a(enc, rs):
        t0 = time.perf_counter()
        for r in rs:
            enc.encode_ref(r)
        return (time.perf_counter() - t0) * 1e3

    def leg_b(enc, rs):
        t0 = time.perf_counter()
        enc.encode_refs(rs)
        return (time.perf_counter() - t0) * 1e3

    legs = [("a", leg_a)] + ([("b", leg_b)] if args.legs == "ab" else [])
    encs = [("speaker", spk), ("mimi", mimi)]
    for k in SETS:                                            # warm-up: workspaces at their largest, code objects, RoPE tables
        for _, enc in encs:
            for _, f in legs:
                f(enc, refs[:k])
    acc = {(e, k, l): [] for e, _ in encs for k in SETS for l, _ in legs}
    for rep in range(REPS):
        for k in SETS:
            for e, enc in encs:
                for l, f in legs:
                    acc[(e, k, l)].append(f(enc, refs[:k]))
        print(f"repetition {rep} done", file=sys.stderr, flush=True)
    parent = None
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
    audio = {k: sum(DURS[i % len(DURS)] for i in range(k)) for k in SETS}
    lines = [f"encode_refs_ab ({args.label}): 1.7B-width speaker encoder + full Mimi, clips of {DURS} s repeating, "
             f"{REPS} repetitions, ms: median (min .. max)",
             f"{'encoder':8s} {'clips':>5s} {'audio s':>7s} {'leg a: encode_ref loop':>30s} {'clips/s':>8s} {'leg b: one encode_refs':>30s} {'clips/s':>8s} "
             f"{'b / a':>22s} {'parent leg a':>30s} {'b / parent a':>22s}"]
    for e, _ in encs:
        for k in SETS:
            a = np.array(acc[(e, k, "a")])
            row = f"{e:8s} {k:5d} {audio[k]:7d} {fmt_stat(a):>30s} {1e3 * k / np.median(a):8.1f}"
            if args.legs == "ab":
                b = np.array(acc[(e, k, "b")])
                ratio = b / a
                row += f" {fmt_stat(b):>30s} {1e3 * k / np.median(b):8.1f} {np.median(b) / np.median(a):7.3f} ({ratio.min():.3f} .. {ratio.max():.3f})"
                if parent is not None:
                    pa = np.array(parent[f"{e}/{k}/a"])
                    rp = b / pa
                    row += f" {fmt_stat(pa):>30s} {np.median(b) / np.median(pa):7.3f} ({rp.min():.3f} .. {rp.max():.3f})"
            lines.append(row)
    for r in refs:
        r.close()
    spk.close(); mimi.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({f"{e}/{k}/{l}": v for (e, k, l), v in acc.items()}, f)


if __name__ == "__main__":
    main()
