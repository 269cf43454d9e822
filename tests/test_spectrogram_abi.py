"""Host-side checks of the fused linear spectrogram that need no GPU: svcmi_linear_spectrogram_f32 rejects bad arguments before it
touches the device (against the hipcc-built library, like tests/test_abi.py) and the ABI number is unchanged by the addition."""
import ctypes
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -3


@pytest.fixture(scope="module")
def lib():
    from svcmi import _lib
    spec = importlib.util.spec_from_file_location("svcmi_build", os.path.join(ROOT, "whisper-vits-svc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return _lib.load_library(mod.build_hip())


def test_abi_version_unchanged(lib):
    from svcmi import _lib
    assert _lib.ABI_VERSION == 22 and lib.svcmi_abi_version() == 22
    assert "svcmi_linear_spectrogram_f32" in _lib.SIGNATURES


def test_argument_validation_needs_no_gpu(lib):
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base)
    f = lib.svcmi_linear_spectrogram_f32
    # a valid call would be f(p, 203, 1, 203, p, 64, 20, 22, 1e-6, p, 10, None): 1 + (203 + 44 - 64) // 20 = 10 frames
    assert f(None, 203, 1, 203, p, 64, 20, 22, 1e-6, p, 10, None) == EINVAL          # null x
    assert f(p, 203, 1, 203, None, 64, 20, 22, 1e-6, p, 10, None) == EINVAL          # null basis
    assert f(p, 203, 1, 203, p, 64, 20, 22, 1e-6, None, 10, None) == EINVAL          # null out
    assert f(p, 203, 0, 203, p, 64, 20, 22, 1e-6, p, 10, None) == EINVAL             # batch < 1
    assert f(p, 203, 1, 22, p, 64, 20, 22, 1e-6, p, 1, None) == EINVAL               # n <= pad: the reference's reflect pad raises
    assert f(p, 203, 1, 21, p, 64, 20, 22, 1e-6, p, 1, None) == EINVAL
    assert f(p, 203, 1, 30, p, 64, 20, 10, 1e-6, p, 0, None) == EINVAL               # n + 2 pad < n_fft: frames < 1
    assert f(p, 203, 1, 30, p, 64, 20, 10, 1e-6, p, 1, None) == EINVAL
    assert f(p, 203, 1, 203, p, 64, 0, 22, 1e-6, p, 10, None) == EINVAL              # hop < 1
    assert f(p, 203, 1, 203, p, 64, -20, 22, 1e-6, p, 10, None) == EINVAL
    assert f(p, 203, 1, 203, p, 63, 20, 22, 1e-6, p, 10, None) == EINVAL             # n_fft odd
    assert f(p, 203, 1, 203, p, 0, 20, 22, 1e-6, p, 10, None) == EINVAL
    assert f(p, 203, 1, 203, p, 64, 20, -1, 1e-6, p, 10, None) == EINVAL             # pad < 0
    assert f(p, 203, 1, 203, p, 64, 20, 22, 1e-6, p, 11, None) == EINVAL             # another frame count
    assert f(p, 100, 3, 203, p, 64, 20, 22, 1e-6, p, 10, None) == EINVAL             # batch stride shorter than a row
    q = ctypes.c_void_p(base + 2)
    assert f(q, 203, 1, 203, p, 64, 20, 22, 1e-6, p, 10, None) == EALIGN
    assert f(p, 203, 1, 203, p, 64, 20, 22, 1e-6, q, 10, None) == EALIGN
