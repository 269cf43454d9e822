"""Host-side checks of the GPU wav loader that need no GPU: svcmi_pcm_resample_f32 rejects bad arguments before it touches the device
(against the hipcc-built library, like tests/test_abi.py), the ABI number is unchanged by the addition, and the filter the kernel is
handed is scipy's default resample_poly design, checked against its closed form."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


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
    assert "svcmi_pcm_resample_f32" in _lib.SIGNATURES


def test_argument_validation_needs_no_gpu(lib):
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.svcmi_pcm_resample_f32
    # a valid call would be f(p, 1, 2, 441, p, 160, 441, 56, 4410, p, 160, None): 441 stereo int16 frames at 44.1 kHz -> 160 outputs
    assert f(None, 1, 2, 441, p, 160, 441, 56, 4410, p, 160, None) == EINVAL          # null pcm
    assert f(p, 1, 2, 441, p, 160, 441, 56, 4410, None, 160, None) == EINVAL          # null out
    assert f(p, 1, 2, 0, p, 160, 441, 56, 4410, p, 0, None) == EINVAL                 # frames <= 0
    assert f(p, 1, 2, -5, p, 160, 441, 56, 4410, p, 0, None) == EINVAL
    assert f(p, 4, 2, 441, p, 160, 441, 56, 4410, p, 160, None) == EINVAL             # fmt outside 0..3
    assert f(p, -1, 2, 441, p, 160, 441, 56, 4410, p, 160, None) == EINVAL
    assert f(p, 1, 0, 441, p, 160, 441, 56, 4410, p, 160, None) == EINVAL             # channels outside 1..8
    assert f(p, 1, 9, 441, p, 160, 441, 56, 4410, p, 160, None) == EINVAL
    assert f(p, 1, 2, 441, p, 0, 441, 56, 4410, p, 160, None) == EINVAL               # up < 1
    assert f(p, 1, 2, 441, p, 160, 0, 56, 4410, p, 160, None) == EINVAL               # down < 1
    assert f(p, 1, 2, 441, p, 160, 441, 56, 4410, p, 161, None) == EINVAL             # n_out != ceil(frames * up / down)
    assert f(p, 1, 2, 442, p, 160, 441, 56, 4410, p, 160, None) == EINVAL             # (442 frames -> 161)
    assert f(p, 1, 2, 441, None, 160, 441, 56, 4410, p, 160, None) == EINVAL          # no taps, but a rate change
    assert f(p, 1, 2, 441, None, 1, 3, 61, 30, p, 147, None) == EINVAL
    assert f(p, 1, 2, 441, p, 160, 441, 55, 4410, p, 160, None) == EINVAL             # taps_per_phase != ceil((2 * half + 1) / up)
    assert f(p, 1, 2, 441, p, 160, 441, 57, 4410, p, 160, None) == EINVAL
    assert f(p, 1, 2, 441, p, 160, 441, 56, -1, p, 160, None) == EINVAL


def test_resample_taps_are_scipys_default_design():
    from svcmi.whisper import audio as A
    taps, half = A.resample_taps(160, 441)
    assert tuple(taps.shape) == (160, 56) and half == 4410
    assert A.resample_taps(16000, 44100)[0] is taps                                   # reduced by the gcd, made once
    h, half2, up, down = A.resample_filter(16000, 44100)
    assert (half2, up, down) == (4410, 160, 441) and h.shape == (2 * 4410 + 1,) and h.dtype == np.float64
    # closed form of firwin(N, 1 / 441, window=("kaiser", 5.0)) scaled by up: windowed sinc, unit gain at DC
    n = np.arange(2 * half + 1) - half
    w = np.i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (n / half) ** 2))) / np.i0(5.0)
    closed = np.sinc(n / 441.0) * w
    closed *= 160.0 / closed.sum()
    assert np.abs(h - closed).max() <= 1e-12 * np.abs(closed).max()
    # the packed image: taps[p, k] = h[p + k * up], zero past the end of h
    img = taps.numpy()
    flat = np.zeros(160 * 56)
    flat[:h.shape[0]] = h
    assert np.array_equal(img, flat.reshape(56, 160).T.astype(np.float32))
    for (u, d, k) in ((1, 3, 61), (320, 441, 28), (640, 441, 21), (2, 1, 21)):
        t, hf = A.resample_taps(u, d)
        assert tuple(t.shape) == (u, k) and hf == 10 * max(u, d)


def test_closed_form_filter_reproduces_resample_poly():
    """The polyphase sum the kernel evaluates, in float64 on the host, against scipy.signal.resample_poly itself."""
    from scipy.signal import resample_poly
    from svcmi.whisper import audio as A
    rng = np.random.default_rng(3)
    for rate in (44100, 48000, 11025, 8000):
        h, half, up, down = A.resample_filter(16000, rate)
        x = rng.uniform(-1, 1, 700)
        n_out = -(-700 * up // down)
        k_taps = -(-(2 * half + 1) // up)
        hp = np.zeros(up * k_taps)
        hp[:h.shape[0]] = h
        xp = np.concatenate([np.zeros(k_taps), x, np.zeros(k_taps)])
        y = np.zeros(n_out)
        for m in range(n_out):
            c = m * down + half
            p, j = c % up, c // up
            idx = j - np.arange(k_taps)
            ok = (idx >= -k_taps) & (idx < 700 + k_taps)
            y[m] = np.dot(xp[idx[ok] + k_taps], hp[p + np.arange(k_taps)[ok] * up])
        assert np.abs(y - resample_poly(x, up, down)).max() <= 1e-13


def test_cli_parsers_take_a_loader_choice():
    from svcmi import svc_inference, svc_inference_batch
    base = ["--config", "c", "--model", "m", "--wave", "w", "--spk", "s"]
    for mod in (svc_inference, svc_inference_batch):
        assert mod.build_parser().parse_args(base).loader == "host"
        assert mod.build_parser().parse_args(base + ["--loader", "gpu"]).loader == "gpu"
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(base + ["--loader", "nope"])
