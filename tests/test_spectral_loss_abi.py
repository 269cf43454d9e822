"""Host-side checks of the checkpoint-scoring entry points that need no GPU: exported, declared in the header and in the ctypes table,
the ABI number unchanged by the addition, and bad arguments rejected before the device is touched (against the hipcc-built library, like
tests/test_spectrogram_abi.py)."""
import ctypes
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -3
NAMES = ("svcmi_stft_distance_f32", "svcmi_log_mel_f32", "svcmi_abs_diff_sum_f32")


@pytest.fixture(scope="module")
def lib():
    from svcmi import _lib
    spec = importlib.util.spec_from_file_location("svcmi_build", os.path.join(ROOT, "whisper-vits-svc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return _lib.load_library(mod.build_hip())


def test_names_exported_declared_and_bound_under_the_same_abi(lib):
    from svcmi import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svcmi.h")).read(), flags=re.S)
    for name in NAMES + ("svcmi_stft_distance_workspace_bytes", "svcmi_abs_diff_sum_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.ABI_VERSION == 22 and lib.svcmi_abi_version() == 22


def test_workspace_queries(lib):
    q = lib.svcmi_stft_distance_workspace_bytes
    assert q(1, 200, 64, 16, 32) == 12                                  # 13 frames, 33 bins: one block
    assert q(3, 320000, 1024, 120, 512) == 3 * 12 * 84 * 9              # 2667 frames -> 84 tiles, 513 bins -> 9 columns
    assert q(1, 32, 64, 16, 32) == EINVAL and q(0, 200, 64, 16, 32) == EINVAL and q(1, 200, 63, 16, 32) == EINVAL and q(1, 200, 64, 0, 32) == EINVAL
    a = lib.svcmi_abs_diff_sum_workspace_bytes
    assert a(1, 1) == 4 and a(2, 4096) == 8 and a(2, 4097) == 16 and a(0, 5) == EINVAL and a(1, 0) == EINVAL


def test_argument_validation_needs_no_gpu(lib):
    buf = (ctypes.c_double * 4096)()
    base = ctypes.addressof(buf)
    p, q4, q2 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)
    f = lib.svcmi_stft_distance_f32
    # a valid call would be f(p, 200, p, 200, 1, 200, p, 64, 16, 32, 1e-7, 13, p, 12, p, None): 1 + 200 // 16 = 13 frames, one 12-byte slot
    assert f(None, 200, p, 200, 1, 200, p, 64, 16, 32, 1e-7, 13, p, 12, p, None) == EINVAL        # null x
    assert f(p, 200, None, 200, 1, 200, p, 64, 16, 32, 1e-7, 13, p, 12, p, None) == EINVAL        # null y
    assert f(p, 200, p, 200, 1, 200, None, 64, 16, 32, 1e-7, 13, p, 12, p, None) == EINVAL        # null basis
    assert f(p, 200, p, 200, 1, 200, p, 64, 16, 32, 1e-7, 13, None, 12, p, None) == EINVAL        # null workspace
    assert f(p, 200, p, 200, 1, 200, p, 64, 16, 32, 1e-7, 13, p, 12, None, None) == EINVAL        # null out
    assert f(p, 200, p, 200, 0, 200, p, 64, 16, 32, 1e-7, 13, p, 12, p, None) == EINVAL           # batch < 1
    assert f(p, 200, p, 200, 1, 32, p, 64, 16, 32, 1e-7, 3, p, 12, p, None) == EINVAL             # n <= pad
    assert f(p, 200, p, 200, 1, 200, p, 64, 0, 32, 1e-7, 13, p, 12, p, None) == EINVAL            # hop < 1
    assert f(p, 200, p, 200, 1, 200, p, 63, 16, 32, 1e-7, 13, p, 12, p, None) == EINVAL           # n_fft odd
    assert f(p, 200, p, 200, 1, 200, p, 64, 16, -1, 1e-7, 13, p, 12, p, None) == EINVAL           # pad < 0
    assert f(p, 200, p, 200, 1, 200, p, 64, 16, 32, 1e-7, 14, p, 12, p, None) == EINVAL           # another frame count
    assert f(p, 200, p, 200, 1, 200, p, 64, 16, 32, 0.0, 13, p, 12, p, None) == EINVAL            # floor <= 0
    assert f(p, 200, p, 200, 1, 200, p, 64, 16, 32, 1e-7, 13, p, 8, p, None) == EINVAL            # workspace too small
    assert f(p, 100, p, 200, 2, 200, p, 64, 16, 32, 1e-7, 13, p, 24, p, None) == EINVAL           # batch stride shorter than a row
    assert f(q2, 200, p, 200, 1, 200, p, 64, 16, 32, 1e-7, 13, p, 12, p, None) == EALIGN
    assert f(p, 200, q2, 200, 1, 200, p, 64, 16, 32, 1e-7, 13, p, 12, p, None) == EALIGN
    assert f(p, 200, p, 200, 1, 200, p, 64, 16, 32, 1e-7, 13, p, 12, q4, None) == EALIGN          # doubles: 8-byte aligned
    g = lib.svcmi_log_mel_f32
    # a valid call would be g(p, 1, 33, 12, p, 32, 10, 1e-5, p, None)
    assert g(None, 1, 33, 12, p, 32, 10, 1e-5, p, None) == EINVAL and g(p, 1, 33, 12, None, 32, 10, 1e-5, p, None) == EINVAL
    assert g(p, 1, 33, 12, p, 32, 10, 1e-5, None, None) == EINVAL and g(p, 0, 33, 12, p, 32, 10, 1e-5, p, None) == EINVAL
    assert g(p, 1, 0, 12, p, 32, 10, 1e-5, p, None) == EINVAL and g(p, 1, 33, 0, p, 32, 10, 1e-5, p, None) == EINVAL
    assert g(p, 1, 33, 12, p, 32, 0, 1e-5, p, None) == EINVAL and g(p, 1, 33, 12, p, 96, 100, 1e-5, p, None) == EINVAL      # 100 rows need ldm 128
    assert g(p, 1, 33, 12, p, 32, 10, 0.0, p, None) == EINVAL
    assert g(q2, 1, 33, 12, p, 32, 10, 1e-5, p, None) == EALIGN and g(p, 1, 33, 12, p, 32, 10, 1e-5, q2, None) == EALIGN
    h = lib.svcmi_abs_diff_sum_f32
    # a valid call would be h(p, 396, p, 396, 1, 396, p, 4, p, None)
    assert h(None, 396, p, 396, 1, 396, p, 4, p, None) == EINVAL and h(p, 396, None, 396, 1, 396, p, 4, p, None) == EINVAL
    assert h(p, 396, p, 396, 1, 396, None, 4, p, None) == EINVAL and h(p, 396, p, 396, 1, 396, p, 4, None, None) == EINVAL
    assert h(p, 396, p, 396, 0, 396, p, 4, p, None) == EINVAL and h(p, 396, p, 396, 1, 0, p, 4, p, None) == EINVAL
    assert h(p, 396, p, 396, 1, 4097, p, 4, p, None) == EINVAL and h(p, 100, p, 396, 2, 396, p, 8, p, None) == EINVAL
    assert h(q2, 396, p, 396, 1, 396, p, 4, p, None) == EALIGN and h(p, 396, p, 396, 1, 396, p, 4, q4, None) == EALIGN
