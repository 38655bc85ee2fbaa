"""The tone step's host side (no GPU): q3_tone_design against the cookbook formulas in numpy float64, the refusals
and the words they name, the names, and the parsing of a --tone string."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api
import tone_cases as tc

L = _lib.lib
Q3_INVALID_ARG = 1


@pytest.mark.parametrize("band", [("peak", 3000, 3.0, 1.0), ("ls", 200, 4.0, 0.8), ("hs", 8000, -2.0, 0.707), ("hp", 120, 0.0, 0.707),
                                  ("lp", 3400, 0.0, 0.707), tc.HP20[0], tc.PEAK[0], ("hs", 11000, -24.0, 0.1), ("peak", 20, 24.0, 10.0)])
def test_design_is_the_cookbook(band):
    got, want = api.tone_design(band), tc.rbj(*band)
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (got, want)
    poles = np.roots(got[3:])
    assert (np.abs(poles) < 1.0).all()


@pytest.mark.parametrize("band,word", [((5, 1000, 0, 1), "kind"), ((-1, 1000, 0, 1), "kind"), (("peak", 19, 0, 1), "freq_hz"),
                                       (("peak", 11001, 0, 1), "freq_hz"), (("ls", 1000, 24.01, 1), "gain_mB"), (("hs", 1000, -24.01, 1), "gain_mB"),
                                       (("hp", 1000, 0, 0.099), "q_milli"), (("lp", 1000, 0, 10.001), "q_milli")])
def test_refusals_name_the_field(band, word):
    with pytest.raises(_lib.Q3Error) as e:
        api.tone_design(band)
    assert e.value.status == Q3_INVALID_ARG and word in str(e.value)


def test_a_pass_kind_does_not_read_its_gain():
    np.testing.assert_array_equal(api.tone_design(("hp", 120, 99.0, 0.707)), api.tone_design(("hp", 120)))
    with pytest.raises(_lib.Q3Error, match="half the rate"):
        api.tone_design(("peak", 4000, 0.0, 1.0), rate=8000)


def test_names_and_null_handles():
    band = _lib.CToneBand(0, 1000, 0, 1000)
    for name in ("q3_pcm_stage_set_tone", "q3_tone_design", "q3_session_set_tone", "q3_batcher_ticket_tone"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.q3_pcm_stage_set_tone(None, 0, 1, ctypes.byref(band)) == Q3_INVALID_ARG
    assert L.q3_session_set_tone(None, 0, 1, ctypes.byref(band)) == Q3_INVALID_ARG
    assert L.q3_batcher_ticket_tone(None, 1, 1, ctypes.byref(band)) == Q3_INVALID_ARG
    assert L.q3_tone_design(24000, None, None) == Q3_INVALID_ARG


def test_tone_string():
    assert api.tone_bands("hp:120,peak:3000:+3:1.0,hs:8000:-2") == ((3, 120, 0, 707), (0, 3000, 300, 1000), (2, 8000, -200, 707))
    assert api.tone_bands(None) == () and api.tone_bands("") == ()
    for bad in ("bp:100", "hp", "hp:1:2:3:4"):
        with pytest.raises(ValueError):
            api.tone_bands(bad)
