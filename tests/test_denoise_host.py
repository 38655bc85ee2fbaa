"""The spectral noise suppressor, the parts that need no device: q3_denoise_plan against the definition's formulas,
the refusals of the new entry points, and the CLI's --ref-denoise argument errors."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api, cli
from denoise_cases import LENGTHS, plan


@pytest.mark.parametrize("n", LENGTHS + [24000 * 120])
def test_plan_is_the_definitions(n):
    assert tuple(api.denoise_plan(n)) == plan(n)


def test_refusals_need_no_device():
    L = _lib.lib
    assert L.q3_abi_version() == 1
    t = ctypes.c_int(); d = ctypes.c_double()
    null1 = (ctypes.c_void_p * 1)(); out = (ctypes.c_void_p * 1)()
    db = lambda v: (ctypes.c_float * 1)(v)
    calls = [lambda: L.q3_denoise_plan(0, ctypes.byref(t), None, None, None),
             lambda: L.q3_denoise_plan(24000 * 120 + 1, ctypes.byref(t), None, None, None),
             lambda: L.q3_ref_audio_denoise(None, 1, None, out),
             lambda: L.q3_ref_audio_denoise(null1, 1, None, None),
             lambda: L.q3_ref_audio_denoise(null1, 0, None, out),
             lambda: L.q3_ref_audio_denoise(null1, 65, None, out),
             lambda: L.q3_ref_audio_denoise(null1, 1, None, out),                     # a null handle
             lambda: L.q3_ref_audio_denoise(null1, 1, db(-0.5), out),
             lambda: L.q3_ref_audio_denoise(null1, 1, db(30.5), out),
             lambda: L.q3_ref_audio_denoise(null1, 1, db(float("nan")), out),
             lambda: L.q3_ref_audio_noise(None, ctypes.byref(d), ctypes.byref(d))]
    for k, f in enumerate(calls):
        assert f() == 1 and L.q3_last_error(), k                                      # Q3_INVALID_ARG, with a message
    assert b"reduce_db" in (L.q3_ref_audio_denoise(null1, 1, db(31.0), out), L.q3_last_error())[1]
    assert not out[0]                                                                 # nothing was created
    assert L.q3_denoise_plan(1, None, None, None, None) == 0                          # every out pointer is optional


@pytest.mark.parametrize("extra", [[], ["--ref-intake", "host"], ["--ref-intake", "device", "--ref-denoise", "31"]])
def test_cli_ref_denoise_argument_errors(extra, capsys):
    argv = ["--synthetic", "tiny", "--text", "hi", "--ref-audio", "a.wav", "--x-vector-only", "--ref-denoise", "12"] + extra
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and "--ref-denoise" in capsys.readouterr().err
