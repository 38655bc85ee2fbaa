"""--trim-silence-db / --edge-ms / --max-pause-ms of the CLI: the refusals, which come before anything is loaded, and
on the GPU the streamed run against the restatement of the plain run's PCM."""
import numpy as np
import pytest

from qwen3_tts_rs_amd import cli

ARGS = ["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "9", "--no-eos", "--seed", "7"]


def test_flags_parse_and_have_their_defaults():
    a = cli.build_parser().parse_args(ARGS + ["--streaming", "--trim-silence-db", "-50"])
    assert cli.silence_from_args(a) == (-50.0, 50, 400)
    a = cli.build_parser().parse_args(ARGS + ["--streaming", "--trim-silence-db", "-42.5", "--edge-ms", "0", "--max-pause-ms", "2000"])
    assert cli.silence_from_args(a) == (-42.5, 0, 2000)
    assert cli.silence_from_args(cli.build_parser().parse_args(ARGS + ["--streaming"])) is None


@pytest.mark.parametrize("extra, word", [
    (["--trim-silence-db", "-50"], "--streaming"),                                          # not without --streaming
    (["--streaming", "--edge-ms", "50"], "--trim-silence-db"),                              # the companions alone
    (["--streaming", "--max-pause-ms", "400"], "--trim-silence-db"),
    (["--streaming", "--trim-silence-db", "-95"], "out of range"),
    (["--streaming", "--trim-silence-db", "-10"], "out of range"),
    (["--streaming", "--trim-silence-db", "-50", "--edge-ms", "55"], "--edge-ms"),
    (["--streaming", "--trim-silence-db", "-50", "--edge-ms", "1010"], "--edge-ms"),
    (["--streaming", "--trim-silence-db", "-50", "--max-pause-ms", "10"], "--max-pause-ms"),
    (["--streaming", "--trim-silence-db", "-50", "--max-pause-ms", "405"], "--max-pause-ms"),
])
def test_refusals_come_before_anything_is_loaded(extra, word, capsys, tmp_path):
    assert cli.main(ARGS + ["--output-dir", str(tmp_path / "o")] + extra) == 2
    cap = capsys.readouterr()
    assert word in cap.err and "Loaded model" not in cap.out
    assert not (tmp_path / "o").exists()


@pytest.mark.gpu
def test_streamed_run_is_the_restatement_of_the_plain_run(tmp_path, capsys):
    from test_silence_layers import one_shot, pick
    assert cli.main(ARGS + ["--output-dir", str(tmp_path / "o"), "--streaming"]) == 0
    pcm24 = np.fromfile(tmp_path / "o" / "audio_seed7_frames9.bin", dtype="<f4")
    thr, y, counts = pick(pcm24, 0, 20)
    capsys.readouterr()
    assert cli.main(ARGS + ["--output-dir", str(tmp_path / "o2"), "--streaming", "--trim-silence-db", str(thr / 100.0), "--edge-ms", "0",
                            "--max-pause-ms", "20", "--output-rate", "16000"]) == 0
    out = capsys.readouterr().out
    got = np.fromfile(tmp_path / "o2" / "audio_seed7_frames9.bin", dtype="<f4")
    np.testing.assert_array_equal(got.view(np.uint32), one_shot(y, 16000).view(np.uint32))
    assert f"Silence: {counts[2]} samples cut at the front, {counts[3]} in pauses, {counts[4]} at the end" in out
    assert counts[1] < counts[0]
