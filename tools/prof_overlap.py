"""A rocprofv3 --kernel-trace CSV of a q3_session_run with segments decoded beside the frame loop (Q3_DECODE_OVERLAP=1): which
vocoder launches ran BESIDE frame kernels and how long they took there against the same launches in the tail after the loop, and
what the frame kernels cost while a vocoder launch was resident. Usage: prof_overlap.py <kernel_trace.csv>
Frame loop = first to last k_sample launch; vocoder launches = everything of the codec family (k_conv*, k_resunit*, k_lin_small*,
k_dwconv7, k_attn_c / _mfma / cb / cs, the [C][L] norms, RoPE, SiLU, the quantiser, the latent copy)."""
import bisect, collections, csv, sys

CODEC = {"k_conv_bf16x3", "k_conv1d", "k_conv1d_mfma", "k_conv_out1", "k_conv_out1_v4", "k_resunit_bf16x3", "k_lin_small_bf16x3", "k_dwconv7",
         "k_attn_c", "k_attn_c_mfma", "k_attn_cb", "k_attn_cs", "k_norm_c", "k_norm_c2", "k_rope_c", "k_silu_mul", "k_rvq_embed", "k_copy_rows",
         "k_copy_cols"}


def is_codec(name):
    return name.split("<")[0].strip() in CODEC


def short(name):
    return name.replace("(anonymous namespace)::", "").replace("void q3::", "").replace("q3::", "").replace("void ", "").split("(")[0]


rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in csv.DictReader(open(sys.argv[1])))
samp = [r for r in rows if r[2].startswith("k_sample")]
if len(samp) < 8:
    sys.exit("no frame loop in this trace")
# the last step of the run (a warm-up step would come first): its samplers are the last burst without a gap above 50 ms
last = len(samp) - 1
first = last
while first > 0 and samp[first][0] - samp[first - 1][1] < 50_000_000:
    first -= 1
t_a, t_b = samp[first][0], samp[last][1]
codec = [r for r in rows if is_codec(r[2]) and r[0] >= t_a]
frame = [r for r in rows if not is_codec(r[2]) and t_a <= r[0] <= t_b]
beside = [r for r in codec if r[0] < t_b]
tail = [r for r in codec if r[0] >= t_b]
print(f"frame loop of the last step: {len(samp[first:last + 1])} frames, {(t_b - t_a) / 1e6:.1f} ms; vocoder launches beside it {len(beside)} "
      f"({sum(e - s for s, e, _ in beside) / 1e6:.1f} ms of kernel time, last one ends {(max(e for _, e, _ in beside) - t_b) / 1e6 if beside else 0:+.1f} ms "
      f"relative to the last sampler), in the tail {len(tail)} ({sum(e - s for s, e, _ in tail) / 1e6:.1f} ms; tail ends {(max(e for _, e, _ in tail) - t_b) / 1e6 if tail else 0:.1f} ms after the last sampler)")
# the frame kernels, with and without a vocoder launch in flight at their start
cs = [r[0] for r in codec]
run_end = []                      # prefix maximum of end times: a vocoder launch is in flight at t if one started before t ends after t
m = 0
for r in codec:
    m = max(m, r[1]); run_end.append(m)
agg = collections.defaultdict(lambda: [0, 0, 0, 0])
for s, e, n in frame:
    i = bisect.bisect_right(cs, s) - 1
    busy = i >= 0 and run_end[i] > s
    a = agg[n]
    a[0 if busy else 2] += 1; a[1 if busy else 3] += e - s
print(f"\n{'frame kernel':46s} {'beside: calls':>14s} {'avg us':>8s} {'alone: calls':>13s} {'avg us':>8s} {'ratio':>6s}")
tb = ta = 0
for n, (nb, db, na, da) in sorted(agg.items(), key=lambda kv: -(kv[1][1] + kv[1][3])):
    tb += db; ta += da
    if nb and na:
        print(f"{n:46s} {nb:14d} {db / nb / 1e3:8.2f} {na:13d} {da / na / 1e3:8.2f} {(db / nb) / (da / na):6.2f}")
print(f"frame kernel time: {tb / 1e6:.1f} ms beside a vocoder launch, {ta / 1e6:.1f} ms alone")
# the vocoder launches, beside the frames and in the tail
va = collections.defaultdict(lambda: [0, 0, 0, 0])
for grp, off in ((beside, 0), (tail, 2)):
    for s, e, n in grp:
        va[n][off] += 1; va[n][off + 1] += e - s
print(f"\n{'vocoder kernel':72s} {'beside: calls':>14s} {'avg us':>9s} {'tail: calls':>12s} {'avg us':>9s}")
for n, (nb, db, nt, dt) in sorted(va.items(), key=lambda kv: -(kv[1][1] + kv[1][3]))[:24]:
    print(f"{n[:72]:72s} {nb:14d} {db / max(nb, 1) / 1e3:9.2f} {nt:12d} {dt / max(nt, 1) / 1e3:9.2f}")
