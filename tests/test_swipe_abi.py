"""Host-side checks of the SWIPE' F0 extractor that need no GPU: the new symbols are there under the unchanged ABI number, the plan's
layout matches the binding, every entry point rejects bad arguments before it touches the device (nothing is launched: the hipcc-built
library has no device here, and every output buffer keeps its fill), the host-made plan has its documented contents, and the command lines
take ``--f0 swipe``."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
NEW = ("svcmi_swipe_plan_bytes", "svcmi_swipe_frames", "svcmi_swipe_mag_f32", "svcmi_swipe_resample_f32", "svcmi_swipe_strength_f32",
       "svcmi_swipe_accum_f32", "svcmi_swipe_finish_f64", "svcmi_swipe_workspace_bytes", "svcmi_swipe_f0_fwd")


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
    for name, value in (("WINDOWS", 8), ("NFFT", 4096), ("LOGBINS", 1024), ("CANDIDATES", 1024)):
        assert f"#define SVCMI_SWIPE_MAX_{name} {value}" in header and getattr(_lib, f"SWIPE_MAX_{name}") == value


def test_plan_size_matches_ctypes(lib):
    from svcmi import _lib
    assert ctypes.sizeof(_lib.SwipeWindow) == 5 * 8 + 2 * 4
    assert lib.svcmi_swipe_plan_bytes() == ctypes.sizeof(_lib.SwipePlan) == 8 * 48 + 4 * 4 + 3 * 8


FILL = 0x5A


def _buffer(nbytes=1 << 16):
    buf = (ctypes.c_ubyte * (nbytes + 512))(*([FILL] * (nbytes + 512)))
    return buf, (ctypes.addressof(buf) + 255) & ~255


def _plan(p, n_win=6, win=None, **over):
    """A plan whose pointers all aim at one host buffer: enough for the argument checks, nothing is launched."""
    from svcmi import _lib
    s = _lib.SwipePlan()
    for o in range(min(n_win, 8)):
        w = s.win[o]
        w.basis = w.resample = w.kernels = w.cand = w.mu = p
        w.n_fft, w.n_cand = 64 << min(o, 5), 100
    s.n_win, s.hop, s.n_log, s.n_pitch = n_win, 320, 897, 635
    s.f_min, s.step, s.threshold = 45.0, 10 / 1200, 0.0
    for k, v in (win or {}).items():
        setattr(s.win[1], k, v)
    for k, v in over.items():
        setattr(s, k, v)
    return s


BAD_PLAN = (dict(n_win=0), dict(n_win=9), dict(hop=0), dict(n_log=1), dict(n_log=1025), dict(n_pitch=0), dict(n_pitch=1025), dict(f_min=0.0),
            dict(step=0.0), dict(threshold=float("nan")))
BAD_WINDOW = (dict(n_fft=8192), dict(n_fft=4), dict(n_fft=96), dict(n_cand=0), dict(n_cand=636), dict(basis=None), dict(resample=None),
              dict(kernels=None), dict(cand=None), dict(mu=None))


def _calls(lib, plan, p, n=640, frames=3):
    """Every entry point on ``plan`` with otherwise valid arguments: the list of return codes."""
    M = ctypes.byref(plan)
    return [lib.svcmi_swipe_frames(M, 0, n), lib.svcmi_swipe_mag_f32(M, 0, p, n, p, None), lib.svcmi_swipe_resample_f32(M, 0, p, frames, p, None),
            lib.svcmi_swipe_strength_f32(M, 0, p, frames, p, None), lib.svcmi_swipe_accum_f32(M, p, n, p, None),
            lib.svcmi_swipe_workspace_bytes(M, n), lib.svcmi_swipe_f0_fwd(M, p, n, p, p, p, p, p, 1 << 40, None)]


def test_entry_points_validate_without_a_gpu(lib):
    keep, p = _buffer()
    ok = _plan(p)
    M = ctypes.byref(ok)
    n, frames = 640, 3
    assert lib.svcmi_swipe_frames(M, -1, 640) == 2 and lib.svcmi_swipe_frames(M, -1, 641) == 3 and lib.svcmi_swipe_frames(M, -1, 1) == 1
    assert lib.svcmi_swipe_frames(M, 0, 640) == 1 + (640 + 64) // 32 and lib.svcmi_swipe_frames(M, 5, 1) == 1 + (1 + 2048) // 1024
    assert lib.svcmi_swipe_workspace_bytes(M, n) > 0
    # the plan: limits and null members, through every entry point
    for bad in BAD_PLAN:
        assert set(_calls(lib, _plan(p, **bad), p)) == {EINVAL}, bad
    for bad in BAD_WINDOW:
        assert set(_calls(lib, _plan(p, win=bad), p)) == {EINVAL}, bad
    for bad_n in (0, -5):                                               # the entry points that take the clip length
        assert {lib.svcmi_swipe_frames(M, 0, bad_n), lib.svcmi_swipe_mag_f32(M, 0, p, bad_n, p, None), lib.svcmi_swipe_accum_f32(M, p, bad_n, p, None),
                lib.svcmi_swipe_workspace_bytes(M, bad_n), lib.svcmi_swipe_f0_fwd(M, p, bad_n, p, p, p, p, p, 1 << 40, None)} == {EINVAL}
    # null pointers
    mag, res, stg, acc, fin, fwd = (lib.svcmi_swipe_mag_f32, lib.svcmi_swipe_resample_f32, lib.svcmi_swipe_strength_f32, lib.svcmi_swipe_accum_f32,
                                    lib.svcmi_swipe_finish_f64, lib.svcmi_swipe_f0_fwd)
    assert mag(None, 0, p, n, p, None) == EINVAL and mag(M, 0, None, n, p, None) == EINVAL and mag(M, 0, p, n, None, None) == EINVAL
    for f in (res, stg):
        assert f(None, 0, p, frames, p, None) == EINVAL and f(M, 0, None, frames, p, None) == EINVAL and f(M, 0, p, frames, None, None) == EINVAL
        assert f(M, 0, p, 0, p, None) == EINVAL and f(M, 6, p, frames, p, None) == EINVAL and f(M, -1, p, frames, p, None) == EINVAL
    assert mag(M, 6, p, n, p, None) == EINVAL and lib.svcmi_swipe_frames(M, 6, n) == EINVAL
    assert acc(None, p, n, p, None) == EINVAL and acc(M, None, n, p, None) == EINVAL and acc(M, p, n, None, None) == EINVAL
    good = [p, frames, 635, 897, 45.0, 10 / 1200, 0.0, p, p, p, p, None]
    for hole in (0, 7, 8, 10):                                          # amax (9) may be null
        a = list(good)
        a[hole] = None
        assert fin(*a) == EINVAL, hole
    for k, v in ((1, 0), (2, 0), (2, 1025), (3, 1), (3, 1025), (4, 0.0), (5, 0.0), (6, float("nan"))):
        a = list(good)
        a[k] = v
        assert fin(*a) == EINVAL, (k, v)
    for hole in (1, 3, 4, 6, 7):                                        # S (5) may be null
        a = [M, p, n, p, p, p, p, p, 1 << 40, None]
        a[hole] = None
        assert fwd(*a) == EINVAL, hole
    assert fwd(None, p, n, p, p, p, p, p, 1 << 40, None) == EINVAL
    need = lib.svcmi_swipe_workspace_bytes(M, n)
    assert fwd(M, p, n, p, p, p, p, p, need - 1, None) == EINVAL and fwd(M, p, n, p, p, p, p, p + 128, 1 << 40, None) == EINVAL
    # alignment and size
    assert mag(M, 0, p + 2, n, p, None) == EALIGN and mag(M, 0, p, n, p + 8, None) == EALIGN and res(M, 0, p + 4, frames, p, None) == EALIGN
    assert stg(M, 0, p, frames, p + 2, None) == EALIGN and fin(*(good[:7] + [p + 4] + good[8:])) == EALIGN
    assert set(_calls(lib, _plan(p, win=dict(resample=p + 4)), p)) == {EALIGN}
    assert lib.svcmi_swipe_workspace_bytes(M, 2 ** 31) == EUNSUPPORTED and mag(M, 0, p, 2 ** 31, p, None) == EUNSUPPORTED
    # nothing was launched or written
    assert bytes(keep) == bytes([FILL]) * len(keep)


def test_plan_contents():
    """The host-made plan at the recipe's parameters: the axes, the six window sizes with their candidate counts, W_N's rows sum to one
    (a spline reproduces constants), the basis is the Hann-windowed DFT, mu in (0, 1]."""
    from svcmi.pitch.core import swipe_slim as W
    pl = W.swipe_plan(Fs=16000, H=320, F_min=45.0, F_max=1760.0, R=10, device="cpu")
    assert pl is W.swipe_plan(Fs=16000, H=320, F_min=45.0, F_max=1760.0, R=10, device="cpu")
    assert pl is not W.swipe_plan(Fs=16000, H=320, F_min=45.0, F_max=1760.0, R=10, strength_threshold=0.2, device="cpu")
    assert (pl.n_log, pl.B, pl.N_pow2) == (897, 635, [64, 128, 256, 512, 1024, 2048])
    assert [len(w["cand"]) for w in pl.windows] == [177, 297, 240, 240, 218, 98]
    assert np.array_equal(pl.F_coef_log_hz[:2], 45.0 * 2 ** (np.arange(2) * (10 / 1200))) and pl.F_coef_log_hz[-1] < 8000.0
    s = pl.struct
    assert (s.n_win, s.hop, s.n_log, s.n_pitch, s.f_min, s.step, s.threshold) == (6, 320, 897, 635, 45.0, 10 / 1200, 0.0)
    for o, w in enumerate(pl.windows):
        assert (s.win[o].n_fft, s.win[o].n_cand) == (w["N"], len(w["cand"]))
        assert np.all(np.diff(w["cand"]) > 0) and w["cand"][-1] < pl.B and bool(((w["mu"] > 0) & (w["mu"] <= 1)).all())
        assert w["W"].shape == (897, w["N"] // 2 + 1) and float(np.abs(w["W"].sum(axis=1) - 1).max()) < 1e-9
        basis, Wt, Kt, cand, mu = pl._keep[o]
        assert basis.shape == (w["N"], w["N"] + 2) and Wt.shape == (897, (w["N"] // 2 + 8) & ~7) and Kt.shape == (len(w["cand"]), 904)
        assert not Wt[:, w["N"] // 2 + 1:].any() and not Kt[:, 897:].any()
    x = np.random.default_rng(0).standard_normal(64)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(64) / 64)
    spec = (x @ W.dft_basis(64)).reshape(33, 2)
    assert np.allclose(spec[:, 0] + 1j * spec[:, 1], np.fft.rfft(x * win), atol=1e-12)
    assert W.prime_and_one(20).tolist() == [1, 2, 3, 5, 7, 11, 13, 17, 19]
    k = W.compute_kernel(100.0, pl.F_coef_log_hz)
    assert abs(np.linalg.norm(k[k > 0]) - 1) < 1e-12 and abs(int(np.argmax(k)) - int(np.argmin(np.abs(pl.F_coef_log_hz - 100.0)))) <= 3      # the 1 / sqrt(f) decay tilts the main lobe


def test_exports():
    import svcmi.pitch as P
    from svcmi.ops import Ops
    from svcmi.pitch.core.swipe_slim import swipe_begin, swipe_plan, swipe_slim
    from svcmi.svc_inference import F0_CHOICES
    assert callable(P.compute_f0_swipe) and callable(P.compute_f0_swipe_begin) and callable(swipe_slim) and callable(swipe_plan) and callable(swipe_begin)
    assert "2 * ceil(n / 320)" in P.compute_f0_swipe.__doc__
    assert F0_CHOICES == ("crepe", "salience", "pyin", "swipe")
    for name in ("swipe_mag", "swipe_resample", "swipe_strength", "swipe_accum", "swipe_finish", "swipe_f0_fwd"):
        assert callable(getattr(Ops, name))


def test_parsers_take_f0_swipe():
    from svcmi import svc_inference as SI
    from svcmi import svc_inference_batch as SB
    base = ["--config", "c", "--model", "m", "--wave", "w", "--spk", "s"]
    for mod in (SI, SB):
        args = mod.build_parser().parse_args(base)
        assert args.f0 == "crepe" and args.swipe_threshold == 0.0
        args = mod.build_parser().parse_args(base + ["--f0", "swipe", "--swipe-threshold", "0.3"])
        assert args.f0 == "swipe" and args.swipe_threshold == 0.3
        assert "swipe" in mod.build_parser().format_help()
