"""Prefix cache, the parts that need no device: the three symbols are declared, bound, documented and in the Rust shim, and a
model handle without a device answers with an error status instead of crashing."""
import ctypes
import os

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import manifest_handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["q3_model_prefix_cache", "q3_model_prefix_cache_info", "q3_session_prefix_info"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_symbols_declared_bound_documented():
    header, integ, shim = _read("include", "q3tts.h"), _read("INTEGRATION.md"), _read("shim", "src", "lib.rs")
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
        assert f"q3_status {n}(" in header, n
        assert f"`{n}`" in integ, n
        assert f"pub fn {n}(" in shim, n
    assert "pub fn set_prefix_cache(" in shim
    assert _lib.lib.q3_abi_version() == 1


def test_python_surface():
    assert callable(api.Qwen3TTS.prefix_cache) and callable(api.Qwen3TTS.prefix_cache_info) and callable(api.Session.prefix_info)


def test_manifest_only_handle_and_null_handles_return_status():
    L = _lib.lib
    h = manifest_handle(q.tiny())
    try:
        i = ctypes.c_int()
        calls = [
            lambda: L.q3_model_prefix_cache(h, 4),
            lambda: L.q3_model_prefix_cache_info(h, ctypes.byref(i), None, None, None, None, None),
            lambda: L.q3_model_prefix_cache(None, 4),
            lambda: L.q3_model_prefix_cache_info(None, None, None, None, None, None, None),
            lambda: L.q3_session_prefix_info(None, 0, ctypes.byref(i)),
        ]
        for k, f in enumerate(calls):
            assert f() != 0, k
            assert L.q3_last_error(), k
    finally:
        L.q3_model_free(h)
