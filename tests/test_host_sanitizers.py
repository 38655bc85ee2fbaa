"""The C ABI's host-only paths and the CPU oracle under AddressSanitizer + UndefinedBehaviorSanitizer.

CPU only, and never on a GPU: tests/hostsan/build.sh compiles the HOST code of every unit of the library (and the oracle's three C
files) under both sanitizers into build/hostsan/ and links two STAND-ALONE programs; each sub-command runs as a child
process. Nothing sanitized is loaded into python, nothing is preloaded. The harness refuses to run where a device is visible (exit
status 77), and so does this module: it skips when the ordinary library reports a device or when hipcc is missing.

Every sub-command must exit 0 with no sanitizer report and print "<name>: N cases, ..." with N at least the count its tables
imply — the figures below are what the tables of tests/hostsan/harness.cpp and oracle_harness.c give; a sub-command that silently
does nothing, or a table that was dropped, fails here.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = os.path.join(ROOT, "tests", "hostsan", "build.sh")
OUT = os.path.join(ROOT, "build", "hostsan")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HAS_DEVICE = 77          # the harness's exit status when q3_device_count() > 0

# sub-command -> the fewest cases its tables give
LIB_CASES = {"sizes": 588342, "files": 176884, "dsp": 5660, "refusals": 595}
ORACLE_CASES = {"primitives": 5083}                     # (e2e: one case per tensor of its job and 48 calls, below)


def _skip_reason():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        return "hipcc is missing: the sanitized host objects cannot be built"
    from qwen3_tts_rs_amd import _lib
    n = _lib.lib.q3_device_count()
    if n > 0:
        return f"{n} device(s) visible: the sanitizer harness runs only where there is none"
    return None


_reason = _skip_reason()
pytestmark = pytest.mark.skipif(_reason is not None, reason=_reason or "")


def _build(target):
    r = subprocess.run(["bash", RECIPE, target], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.search(r"^compiled (\d+)$", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    return int(m.group(1)), r.stdout


@pytest.fixture(scope="module")
def lib_harness():
    _build("lib")
    return os.path.join(OUT, "harness")


@pytest.fixture(scope="module")
def oracle_harness():
    _build("oracle")
    return os.path.join(OUT, "oracle_harness")


def _run(argv, name, least, timeout=300):
    r = subprocess.run(argv, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, errors="replace", timeout=timeout)
    out = r.stdout
    assert r.returncode != HAS_DEVICE, out
    assert "runtime error:" not in out and "Sanitizer" not in out, out[-6000:]
    assert r.returncode == 0, (r.returncode, out[-6000:])
    m = re.search(rf"^{name}: (\d+) cases, (\d+) accepted, (\d+) refused$", out, re.M)
    assert m, out[-2000:]
    cases, ok, refused = (int(g) for g in m.groups())
    assert cases >= least and ok + refused == cases, (cases, least, ok, refused)
    return cases, ok, refused


@pytest.mark.parametrize("name", ["sizes", "dsp", "refusals"])
def test_library_host_paths(lib_harness, name):
    cases, ok, refused = _run([lib_harness, name], name, LIB_CASES[name])
    if name == "refusals":
        assert ok == 0          # with no device nothing of this table may be accepted
    else:
        assert ok > 0 and refused > 0


def test_library_file_readers(lib_harness, tmp_path):
    cases, ok, refused = _run([lib_harness, "files", str(tmp_path)], "files", LIB_CASES["files"])
    assert ok > 0 and refused > 0


def test_oracle_primitives(oracle_harness):
    _run([oracle_harness, "primitives"], "primitives", ORACLE_CASES["primitives"])


def _hex(struct):
    return bytes(struct).hex()


def _moments(a):
    import numpy as np
    a = np.asarray(a, np.float64)
    return float(a.std()), float(a.mean())


def _write_job(path):
    """Names and element counts from the library's manifest-only handles, the configuration structures of tests/oracle.py as bytes;
    per tensor the spread and the centre of the suite's synthetic checkpoint (the harness draws its own values around them)."""
    import qwen3_tts_rs_amd as q
    from qwen3_tts_rs_amd import _lib, synth
    from qwen3_tts_rs_amd.speaker import SpeakerEncoder, synthetic_speaker_checkpoint
    from qwen3_tts_rs_amd.speech_encoder import SpeechEncoder, synthetic_speech_checkpoint
    import oracle as O
    from common import manifest_handle
    lines = []
    cfg = q.tiny()
    lines.append("config " + _hex(O.to_oconfig(cfg)))
    h = manifest_handle(cfg)
    for name, arr, dt in synth.synthetic_checkpoint(cfg, h, synth.DEFAULT_SEED):
        a = synth.bf16_to_f32(arr) if dt == synth.BF16 else arr
        s, m = _moments(a)
        lines.append(f"tensor {name} {a.size} {s!r} {m!r}")
    _lib.lib.q3_model_free(h)
    scfg = q.tiny_speaker_config(enc_dim=cfg.hidden)
    c = O.OSpkConfig()
    c.mel_dim, c.enc_dim = scfg.mel_dim, scfg.enc_dim
    for i in range(5):
        c.channels[i] = scfg.enc_channels[i]; c.kernel_sizes[i] = scfg.enc_kernel_sizes[i]; c.dilations[i] = scfg.enc_dilations[i]
    c.attention_channels, c.res2net_scale, c.se_channels, c.sample_rate = scfg.enc_attention_channels, scfg.enc_res2net_scale, scfg.enc_se_channels, scfg.sample_rate
    lines.append("spk_config " + _hex(c))
    enc = SpeakerEncoder(scfg, device=-1)
    for name, arr in synthetic_speaker_checkpoint(enc, 7):
        s, m = _moments(arr)
        lines.append(f"spk_tensor {name} {arr.size} {s!r} {m!r}")
    enc.close()
    mcfg = q.tiny_speech_config()
    lines.append("mimi_config " + _hex(O.to_omimi_config(mcfg)))
    menc = SpeechEncoder(mcfg, device=-1)
    for name, arr in synthetic_speech_checkpoint(menc, 7):
        s, m = _moments(arr)
        lines.append(f"mimi_tensor {name} {arr.size} {s!r} {m!r}")
    menc.close()
    n_tensors = sum(1 for ln in lines if ln.split(" ", 1)[0].endswith("tensor"))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return n_tensors


def test_oracle_end_to_end(oracle_harness, tmp_path):
    job = tmp_path / "oracle.job"
    n_tensors = _write_job(str(job))
    assert n_tensors > 100
    # one case per tensor; per prompt kind 8 (session, state, generate, single steps, four decodes), 2 for the model, 4 for the
    # speaker encoder, 10 for the speech encoder
    _run([oracle_harness, "e2e", str(job)], "e2e", n_tensors + 4 * 8 + 2 + 4 + 10, timeout=600)


def test_second_build_rebuilds_nothing(lib_harness, oracle_harness):
    """the sanitized objects are cached by source, headers and command line (csrc/build.sh's rule): an unchanged tree compiles and
    links nothing"""
    compiled, out = _build("all")
    assert compiled == 0 and "linked" not in out, out[-2000:]
