"""The CLI's loudness flags: --target-lufs / --prior-gain-db, parsed and refused before anything is loaded. No GPU."""
import pytest

from qwen3_tts_rs_amd import cli


def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_flag_surface_and_defaults():
    a = _args()
    assert a.target_lufs is None and a.prior_gain_db == 0.0 and a.ceiling_db == 0.0
    assert cli.loudness_from_args(a) is None                              # nothing asked: the stage is left alone
    a = _args("--streaming", "--target-lufs", "-19")
    assert cli.loudness_from_args(a) == (-1900, 0, -100)                  # a -1 dB ceiling unless --ceiling-db is given
    a = _args("--streaming", "--target-lufs", "-23.5", "--prior-gain-db", "7.25", "--ceiling-db", "-3")
    assert cli.loudness_from_args(a) == (-2350, 725, -300)
    a = _args("--streaming", "--target-lufs", "-16", "--ceiling-db", "0")
    assert cli.loudness_from_args(a) == (-1600, 0, 0)                     # given, and off
    a = _args("--streaming", "--target-lufs=-40", "--prior-gain-db=-60")
    assert cli.loudness_from_args(a) == (-4000, -6000, -100)


def test_refusals():
    with pytest.raises(ValueError, match="--streaming"):
        cli.loudness_from_args(_args("--target-lufs", "-19"))
    with pytest.raises(ValueError, match="--target-lufs"):
        cli.loudness_from_args(_args("--streaming", "--prior-gain-db", "3"))
    for bad in (("--target-lufs", "-4"), ("--target-lufs", "-41"), ("--target-lufs", "-19", "--prior-gain-db", "25"),
                ("--target-lufs", "-19", "--prior-gain-db", "-61")):
        with pytest.raises(ValueError, match="out of range"):
            cli.loudness_from_args(_args("--streaming", *bad))


def test_main_exits_before_anything_is_loaded(capsys):
    assert cli.main(["--synthetic", "tiny", "--frames", "9", "--target-lufs", "-19"]) == 2
    assert "--target-lufs applies to --streaming" in capsys.readouterr().err
    assert cli.main(["--synthetic", "tiny", "--frames", "9", "--streaming", "--target-lufs", "-3"]) == 2
    assert "out of range" in capsys.readouterr().err
