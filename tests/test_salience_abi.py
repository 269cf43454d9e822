"""Host-side checks of the salience F0 extractor that need no GPU: the new symbols are there under the unchanged ABI number, the plan's
layout matches the binding, every entry point rejects bad arguments before it touches the device, the host-made plan has its documented
contents, and the command lines take ``--f0``."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
NEW = ("svcmi_salience_plan_bytes", "svcmi_salience_stft_f32", "svcmi_salience_map_f32", "svcmi_salience_dp_f64",
       "svcmi_salience_workspace_bytes", "svcmi_salience_f0_fwd")


@pytest.fixture(scope="module")
def lib():
    from svcmi import _lib
    spec = importlib.util.spec_from_file_location("svcmi_build", os.path.join(ROOT, "whisper-vits-svc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return _lib.load_library(mod.build_hip())


def test_new_symbols_under_the_same_abi_version(lib):
    from svcmi import _lib
    assert _lib.ABI_VERSION == 22 and lib.svcmi_abi_version() == 22
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "svcmi.h")).read()
    assert "#define SVCMI_SALIENCE_MAX_BINS 1024" in header and _lib.SALIENCE_MAX_BINS == 1024


def test_plan_size_matches_ctypes(lib):
    from svcmi import _lib
    assert lib.svcmi_salience_plan_bytes() == ctypes.sizeof(_lib.SaliencePlan) == 4 * 8 + 8 * 4 + 4 * 4 + 3 * 8


def _aligned(nfloats):
    buf = (ctypes.c_float * (nfloats + 64))()
    return buf, (ctypes.addressof(buf) + 255) & ~255


def _plan(p, **over):
    """A plan whose pointers all aim at one host buffer: enough for the argument checks, nothing is launched."""
    from svcmi import _lib
    s = _lib.SaliencePlan()
    s.basis = s.smooth = s.harm_off = s.harm_w = p
    s.n_fft, s.hop, s.k_lo, s.n_bins, s.n_pitch, s.smooth_len, s.n_harm, s.tol = 2048, 320, 2, 228, 636, 11, 90, 5
    s.fs, s.f_min, s.f_max, s.bins_per_octave = 16000.0, 45.0, 1760.0, 120.0
    s.thresh, s.log_hi, s.log_lo = 1.0, 1.19e-7, -4.6
    for k, v in over.items():
        setattr(s, k, v)
    return s


def test_kernel_entry_points_validate_without_a_gpu(lib):
    keep, p = _aligned(4096)
    st, mp, dp = lib.svcmi_salience_stft_f32, lib.svcmi_salience_map_f32, lib.svcmi_salience_dp_f64
    ok = _plan(p)
    M = ctypes.byref(ok)
    n, frames = 640, 3
    # null pointers, plan members included
    assert st(None, p, n, p, frames, None) == EINVAL and st(M, None, n, p, frames, None) == EINVAL and st(M, p, n, None, frames, None) == EINVAL
    for member in ("basis", "smooth", "harm_off", "harm_w"):
        assert st(ctypes.byref(_plan(p, **{member: None})), p, n, p, frames, None) == EINVAL, member
    assert mp(None, p, frames, p, p, p, None) == EINVAL
    for hole in range(4):
        a = [p, p, p, p]
        a[hole] = None
        assert mp(M, a[0], frames, a[1], a[2], a[3], None) == EINVAL, hole
    assert dp(None, frames, 636, 5, 0.0, -4.6, p, p, None) == EINVAL and dp(p, frames, 636, 5, 0.0, -4.6, None, p, None) == EINVAL
    assert dp(p, frames, 636, 5, 0.0, -4.6, p, None, None) == EINVAL
    # fewer than two frames, another frame count, geometry
    assert st(M, p, 319, p, 1, None) == EINVAL and st(M, p, n, p, frames + 1, None) == EINVAL and st(M, p, 0, p, 1, None) == EINVAL
    assert mp(M, p, 1, p, p, p, None) == EINVAL and dp(p, 1, 636, 5, 0.0, -4.6, p, p, None) == EINVAL
    assert dp(p, frames, 0, 5, 0.0, -4.6, p, p, None) == EINVAL and dp(p, frames, 636, -1, 0.0, -4.6, p, p, None) == EINVAL
    for bad in (dict(hop=0), dict(n_fft=2047), dict(n_fft=0), dict(n_bins=0), dict(k_lo=-1), dict(k_lo=900, n_bins=228), dict(n_pitch=0),
                dict(n_harm=0), dict(smooth_len=10), dict(tol=-1), dict(f_min=0.0), dict(f_max=45.0)):
        assert st(ctypes.byref(_plan(p, **bad)), p, n, p, frames, None) == EINVAL, bad
    # above the limits
    for big in (dict(n_bins=1025, k_lo=0, n_fft=4096), dict(n_pitch=1025), dict(tol=1025), dict(n_harm=1025), dict(smooth_len=67)):
        assert st(ctypes.byref(_plan(p, **big)), p, n, p, frames, None) == EUNSUPPORTED, big
        assert mp(ctypes.byref(_plan(p, **big)), p, frames, p, p, p, None) == EUNSUPPORTED, big
    assert dp(p, frames, 1025, 5, 0.0, -4.6, p, p, None) == EUNSUPPORTED and dp(p, frames, 636, 1025, 0.0, -4.6, p, p, None) == EUNSUPPORTED
    assert dp(p, 2 ** 31 // 636 + 1, 636, 5, 0.0, -4.6, p, p, None) == EUNSUPPORTED
    # misalignment
    assert st(M, p + 2, n, p, frames, None) == EALIGN and st(M, p, n, p + 4, frames, None) == EALIGN
    assert st(ctypes.byref(_plan(p, basis=p + 1)), p, n, p, frames, None) == EALIGN
    assert mp(M, p + 4, frames, p, p, p, None) == EALIGN and mp(M, p, frames, p + 2, p, p, None) == EALIGN and mp(M, p, frames, p, p, p + 1, None) == EALIGN
    assert dp(p + 2, frames, 636, 5, 0.0, -4.6, p, p, None) == EALIGN and dp(p, frames, 636, 5, 0.0, -4.6, p + 1, p, None) == EALIGN
    assert dp(p, frames, 636, 5, 0.0, -4.6, p, p + 2, None) == EALIGN


def test_stage_and_workspace_validate_without_a_gpu(lib):
    keep, p = _aligned(4096)
    ok = _plan(p)
    M = ctypes.byref(ok)
    wsb, st = lib.svcmi_salience_workspace_bytes, lib.svcmi_salience_f0_fwd
    n = 3200                                                          # 11 frames
    need = wsb(M, n)
    rows = lambda b: (b + 255) // 256 * 256                            # every piece starts on a 256-byte boundary
    assert need == rows(11 * 228 * 8) + rows(11 * 636 * 4) * 2 + rows(11 * 636 * 2) + 256 + 256
    assert wsb(None, n) == EINVAL and wsb(M, 319) == EINVAL and wsb(M, 0) == EINVAL
    big, ws = _aligned(need // 4 + 64)
    assert st(None, p, n, p, None, ws, need, None) == EINVAL and st(M, None, n, p, None, ws, need, None) == EINVAL
    assert st(M, p, n, None, None, ws, need, None) == EINVAL and st(M, p, n, p, None, None, need, None) == EINVAL
    assert st(M, p, 319, p, None, ws, need, None) == EINVAL
    assert st(M, p, n, p, None, ws, need - 256, None) == EINVAL and st(M, p, n, p, None, ws + 16, need, None) == EINVAL
    assert st(M, p + 2, n, p, None, ws, need, None) == EALIGN and st(M, p, n, p + 2, None, ws, need, None) == EALIGN
    assert st(ctypes.byref(_plan(p, n_pitch=1025)), p, n, p, None, ws, 1 << 30, None) == EUNSUPPORTED


def test_plan_contents():
    """The host-made plan for compute_f0_salience's parameters: the bin range derived from the parameters, 636 pitch bins, the table's
    convention, the sparse harmonic weights, the transition constants."""
    from svcmi.pitch.core import salience as S
    pl = S.salience_plan(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, device="cpu")
    assert (pl.k_lo, pl.n_bins, pl.B) == (2, 228, 636) and pl.F_coef_hertz.dtype == np.float64 and pl.F_coef_hertz[0] == 45.0
    # the function's own defaults: reach 22050 / 512 = 43.07 Hz, bin width 10.77 Hz: ceil(11.93 / 10.77) - 1 = 1, floor(1803.07 / 10.77) + 1 = 168
    assert S.stft_bin_range(22050, 2048, 256, 55.0, 1760.0) == (1, 168)
    t = pl.basis.numpy()
    assert t.shape == (2048, 456) and t.dtype == np.float32
    i, k = 517, 100
    w = 0.5 - 0.5 * np.cos(2 * np.pi * i / 2048)
    assert t[i, 2 * (k - 2)] == np.float32(w * np.cos(2 * np.pi * ((k * i) % 2048) / 2048))
    assert t[i, 2 * (k - 2) + 1] == np.float32(-w * np.sin(2 * np.pi * ((k * i) % 2048) / 2048))
    off, hw = pl.harm_off.numpy(), pl.harm_w.numpy()
    assert len(off) == 110 and off[0] == -4 and off[-1] == 399 + 10 - 4 and bool((np.diff(off) > 0).all()) and bool((hw > 0).all())
    assert abs(hw.max() - 1.0) < 1e-7 and pl.struct.n_harm == 110 and pl.struct.thresh == 1.0
    eps = np.finfo(np.float32).eps
    assert pl.log_hi == float(np.log(np.float64(1.0) + eps)) and pl.log_lo == float(np.log(np.float64(0.01) + eps))
    assert S.salience_plan(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, device="cpu") is pl
    for bad in (dict(N=2047), dict(freq_smooth_len=10), dict(F_min=0.0), dict(alpha=0.0), dict(tol=2000), dict(N=8192, H=64, F_max=7000.0)):
        with pytest.raises(ValueError):
            S.salience_plan(**{**dict(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, device="cpu"), **bad})


def test_exports_and_move_average():
    import svcmi.pitch as P
    from svcmi.pitch.core.salience import salience
    assert callable(P.compute_f0_salience) and callable(P.compute_f0_salience_begin) and callable(salience)
    a = np.arange(7, dtype=np.float64)
    assert np.array_equal(P.move_average(a, 3), np.convolve(a, np.ones(3) / 3, mode="same"))


def test_parsers_take_f0():
    from svcmi import svc_inference as SI
    from svcmi import svc_inference_batch as SB
    base = ["--config", "c", "--model", "m", "--wave", "w", "--spk", "s"]
    for mod in (SI, SB):
        assert mod.build_parser().parse_args(base).f0 == "crepe"
        assert mod.build_parser().parse_args(base + ["--f0", "salience"]).f0 == "salience"
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(base + ["--f0", "yin"])
