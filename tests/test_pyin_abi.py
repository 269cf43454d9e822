"""Host-side checks of the pYIN F0 extractor that need no GPU: the new symbols are there under the unchanged ABI number, the plan's layout
matches the binding, every entry point rejects bad arguments before it touches the device, the host-made plan has its documented
contents, and the command lines take ``--f0 pyin``."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
NEW = ("svcmi_pyin_plan_bytes", "svcmi_pyin_cmndf_f64", "svcmi_pyin_observe_f64", "svcmi_pyin_viterbi_f64", "svcmi_pyin_finish_f64",
       "svcmi_pyin_workspace_bytes", "svcmi_pyin_f0_fwd")
LT, LX, LC = -708.3964185322641, -4.605170185988091, -7.145196


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
    for name, value in (("BINS", 1024), ("THRESHOLDS", 128), ("NFFT", 4096), ("BAND", 33)):
        assert f"#define SVCMI_PYIN_MAX_{name} {value}" in header and getattr(_lib, f"PYIN_MAX_{name}") == value


def test_plan_size_matches_ctypes(lib):
    from svcmi import _lib
    assert lib.svcmi_pyin_plan_bytes() == ctypes.sizeof(_lib.PyinPlan) == 4 * 8 + 8 * 4 + 8 * 8


def _aligned(ndoubles):
    buf = (ctypes.c_double * (ndoubles + 64))()
    return buf, (ctypes.addressof(buf) + 255) & ~255


def _plan(p, **over):
    """A plan whose pointers all aim at one host buffer: enough for the argument checks, nothing is launched."""
    from svcmi import _lib
    s = _lib.PyinPlan()
    s.thresholds = s.beta = s.f_axis = s.band = p
    s.n_fft, s.hop, s.p_min, s.p_max, s.n_pitch, s.n_thr, s.max_step = 2048, 320, 10, 356, 634, 99, 5
    s.fs, s.tol_cents, s.absolute_min_prob, s.voicing_prob = 16000.0, 10.0, 0.01, 0.5
    s.log_tiny, s.log_cross, s.log_c, s.tiny = LT, LX, LC, 2.2250738585072014e-308
    for k, v in over.items():
        setattr(s, k, v)
    return s


BAD = (dict(hop=0), dict(n_fft=2047), dict(n_fft=0), dict(p_min=0), dict(p_max=9), dict(n_pitch=0), dict(n_thr=0), dict(max_step=0),
       dict(n_pitch=10), dict(fs=0.0), dict(tol_cents=0.0), dict(voicing_prob=1.5), dict(voicing_prob=-0.1), dict(tiny=0.0))
BIG = (dict(n_pitch=1025), dict(n_thr=129), dict(n_fft=4098, p_max=4098), dict(max_step=17), dict(p_max=2049))


def test_kernel_entry_points_validate_without_a_gpu(lib):
    keep, p = _aligned(8192)
    cm, ob, vt, fin = lib.svcmi_pyin_cmndf_f64, lib.svcmi_pyin_observe_f64, lib.svcmi_pyin_viterbi_f64, lib.svcmi_pyin_finish_f64
    ok = _plan(p)
    M = ctypes.byref(ok)
    n, frames = 640, 3
    # null pointers, plan members included
    assert cm(None, p, n, p, p, frames, None) == EINVAL
    for hole in range(3):
        a = [p, p, p]
        a[hole] = None
        assert cm(M, a[0], n, a[1], a[2], frames, None) == EINVAL, hole
    for member in ("thresholds", "beta", "f_axis", "band"):
        bad = ctypes.byref(_plan(p, **{member: None}))
        assert cm(bad, p, n, p, p, frames, None) == EINVAL and ob(bad, p, frames, p, p, p, p, None) == EINVAL, member
        assert fin(bad, p, p, p, p, p, frames, p, p, None) == EINVAL, member
    assert ob(None, p, frames, p, p, p, p, None) == EINVAL
    for hole in (0, 1, 3, 4):                                           # logO (2) may be null
        a = [p] * 5
        a[hole] = None
        assert ob(M, a[0], frames, a[1], a[2], a[3], a[4], None) == EINVAL, hole
    for hole in range(4):
        a = [p] * 4
        a[hole] = None
        assert vt(a[0], frames, 634, 5, a[1], LT, LX, LC, a[2], a[3], None) == EINVAL, hole
    assert fin(None, p, p, p, p, p, frames, p, p, None) == EINVAL
    for hole in range(7):
        a = [p] * 7
        a[hole] = None
        assert fin(M, a[0], a[1], a[2], a[3], a[4], frames, a[5], a[6], None) == EINVAL, hole
    # too few frames, another frame count, geometry
    assert cm(M, p, 319, p, p, 1, None) == EINVAL and cm(M, p, n, p, p, frames + 1, None) == EINVAL and cm(M, p, 0, p, p, 1, None) == EINVAL
    assert ob(M, p, 0, p, p, p, p, None) == EINVAL and fin(M, p, p, p, p, p, 0, p, p, None) == EINVAL
    assert vt(p, 1, 634, 5, p, LT, LX, LC, p, p, None) == EINVAL and vt(p, frames, 0, 5, p, LT, LX, LC, p, p, None) == EINVAL
    assert vt(p, frames, 634, 0, p, LT, LX, LC, p, p, None) == EINVAL
    for bad in BAD:
        B = ctypes.byref(_plan(p, **bad))
        assert cm(B, p, n, p, p, frames, None) == EINVAL and ob(B, p, frames, p, p, p, p, None) == EINVAL, bad
        assert fin(B, p, p, p, p, p, frames, p, p, None) == EINVAL, bad
    # above the limits
    for big in BIG:
        B = ctypes.byref(_plan(p, **big))
        assert cm(B, p, n, p, p, frames, None) == EUNSUPPORTED and ob(B, p, frames, p, p, p, p, None) == EUNSUPPORTED, big
        assert fin(B, p, p, p, p, p, frames, p, p, None) == EUNSUPPORTED, big
    assert vt(p, frames, 1025, 5, p, LT, LX, LC, p, p, None) == EUNSUPPORTED and vt(p, frames, 634, 17, p, LT, LX, LC, p, p, None) == EUNSUPPORTED
    assert vt(p, 2 ** 31 // 1268 + 1, 634, 5, p, LT, LX, LC, p, p, None) == EUNSUPPORTED
    # misalignment
    assert cm(M, p + 2, n, p, p, frames, None) == EALIGN and cm(M, p, n, p + 4, p, frames, None) == EALIGN and cm(M, p, n, p, p + 4, frames, None) == EALIGN
    assert cm(ctypes.byref(_plan(p, beta=p + 4)), p, n, p, p, frames, None) == EALIGN
    for hole in range(5):
        a = [p] * 5
        a[hole] = p + 4
        assert ob(M, a[0], frames, a[1], a[2], a[3], a[4], None) == EALIGN, hole
    assert vt(p + 4, frames, 634, 5, p, LT, LX, LC, p, p, None) == EALIGN and vt(p, frames, 634, 5, p + 4, LT, LX, LC, p, p, None) == EALIGN
    assert vt(p, frames, 634, 5, p, LT, LX, LC, p + 1, p, None) == EALIGN and vt(p, frames, 634, 5, p, LT, LX, LC, p, p + 2, None) == EALIGN
    for hole in range(7):
        a = [p] * 7
        a[hole] = p + (2 if hole == 0 else 4)
        assert fin(M, a[0], a[1], a[2], a[3], a[4], frames, a[5], a[6], None) == EALIGN, hole


def test_stage_and_workspace_validate_without_a_gpu(lib):
    keep, p = _aligned(8192)
    ok = _plan(p)
    M = ctypes.byref(ok)
    wsb, st = lib.svcmi_pyin_workspace_bytes, lib.svcmi_pyin_f0_fwd
    n = 3200                                                          # 11 frames
    need = wsb(M, n)
    rows = lambda b: (b + 255) // 256 * 256                            # every piece starts on a 256-byte boundary
    assert need == rows(11 * 357 * 8) + 2 * rows(11 * 1268 * 8) + rows(11 * 8) + 2 * rows(11 * 99 * 8) + 11 * 1268 * 2 + 256
    assert wsb(None, n) == EINVAL and wsb(M, 319) == EINVAL and wsb(M, 0) == EINVAL
    for bad in BAD:
        assert wsb(ctypes.byref(_plan(p, **bad)), n) == EINVAL, bad
    for big in BIG:
        assert wsb(ctypes.byref(_plan(p, **big)), n) == EUNSUPPORTED, big
    big, ws = _aligned(need // 8 + 64)
    call = lambda plan=M, x=p, n_=n, f0=p, conf=p, path=p, rms=None, O=None, lt=None, vt=None, w=ws, wb=need: st(plan, x, n_, f0, conf, path, rms, O, lt, vt, w, wb, None)
    for hole in ("plan", "x", "f0", "conf", "path", "w"):
        assert call(**{hole: None}) == EINVAL, hole
    assert call(n_=319) == EINVAL and call(wb=need - 256) == EINVAL and call(w=ws + 16) == EINVAL
    for arg, off in (("x", 2), ("path", 2), ("f0", 4), ("conf", 4), ("rms", 4), ("O", 4), ("lt", 4), ("vt", 4)):
        assert call(**{arg: p + off}) == EALIGN, arg
    assert call(plan=ctypes.byref(_plan(p, n_pitch=1025)), wb=1 << 30) == EUNSUPPORTED


def _dense_a(B, max_step):
    """The dense [2B, 2B] matrix from the plan's own rows (voiced and unvoiced blocks, the cross links)."""
    from svcmi.pitch.core import pyin as Y
    rows = Y.transition_rows(B, max_step)
    A = np.zeros((2 * B, 2 * B))
    for i in range(B):
        for d in range(2 * max_step + 1):
            j = i - max_step + d
            if 0 <= j < B:
                A[i, j] = A[i + B, j + B] = rows[i, d]
        A[i, i + B] = A[i + B, i] = 1 - 0.99
    return A


def test_plan_contents():
    """The host-made plan for compute_f0_pyin's parameters: 634 pitch bins, the lag range, the beta weights against scipy's beta-binomial
    distribution, the band table gathered by column with the edge rows' renormalisation and one-column asymmetry, the constants."""
    from scipy.stats import betabinom
    from svcmi.pitch.core import pyin as Y
    pl = Y.pyin_plan(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, device="cpu")
    assert (pl.B, pl.p_min, pl.p_max, pl.max_step) == (634, 10, 356, 5) and pl.F_axis.dtype == np.float64 and pl.F_axis[0] == 45.0
    assert pl.struct.n_thr == 99 and pl.struct.tol_cents == 10.0 and pl.struct.voicing_prob == 0.5 and pl.struct.absolute_min_prob == 0.01
    # comb(n, k) beta(k + a, n - k + b) / beta(a, b) is the beta-binomial pmf with n = 99 trials (the reference evaluates it at k = 0 .. 98)
    assert np.allclose(pl.beta_np, betabinom.pmf(np.arange(99), 99, 1, 18), rtol=1e-10, atol=0) and abs(pl.beta_np.sum() - 1) < 1e-3
    tiny = np.finfo(0.).tiny
    assert pl.struct.tiny == tiny and pl.log_tiny == float(np.log(tiny)) and -708.4 < pl.log_tiny < -708.39
    assert pl.log_cross == float(np.log(np.float64(1 - 0.99) + tiny)) and pl.log_c == float(np.log(1.0 / 1268 + tiny))
    band = pl.band_np
    assert band.shape == (634, 11) and band.dtype == np.float64
    rows = Y.transition_rows(634, 5)
    assert np.array_equal(rows[300], rows[5]) and rows[300, 0] == 0 and rows[300, 10] == 0 and abs(rows[300].sum() - 0.99) < 1e-12
    assert abs(rows[0].sum() - 0.99) < 1e-12 and rows[0, 5] > 0 and rows[0, 10] == 0 and not rows[0, :5].any()       # columns 0 .. 4 only
    assert abs(rows[633].sum() - 0.99) < 1e-12 and not rows[633, 6:].any()
    # gathered by column: state 2's predecessor 0 is row 0's column 2
    assert band[2, 3] == np.log(rows[0, 7] + tiny) and band[300, 0] == pl.log_tiny and band[300, 5] == np.log(rows[300, 5] + tiny)
    assert band[4, 1] == np.log(rows[0, 9] + tiny) and band[5, 0] == pl.log_tiny                                       # row 0 stops one column short (a weight that is 0 anyway)
    assert Y.pyin_plan(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, device="cpu") is pl
    for bad in (dict(N=2047), dict(N=8192), dict(R=1), dict(R=60), dict(thresholds=np.arange(0.001, 1, 0.005)), dict(F_min=0.0), dict(voicing_prob=2.0),
                dict(F_min=1000.0, F_max=1040.0)):
        with pytest.raises(ValueError):
            Y.pyin_plan(**{**dict(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, device="cpu"), **bad})


@pytest.mark.needs_reference
@pytest.mark.parametrize("B", [11, 12, 40])
def test_band_table_against_the_reference_matrix(B):
    """The reference's own dense matrix (numba as the identity), its logarithm gathered by column, against the plan's band; and the
    windows rebuilt into a dense matrix equal to it everywhere."""
    from scipy.stats import triang
    from svcmi.pitch.core import pyin as Y
    spec = importlib.util.spec_from_file_location("make_pyin_golden", os.path.join(ROOT, "scripts", "make_pyin_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ref = mod.load_reference("/root/reference")
    ms = 5
    A = ref.compute_transition_matrix(B, triang.pdf(np.arange(-ms, ms + 1), 0.5, scale=2 * ms, loc=-ms))
    assert np.array_equal(_dense_a(B, ms), A)
    logA = np.log(A + np.finfo(0.).tiny)
    band = Y.transition_band(B, ms)
    for i in range(B):
        for d in range(2 * ms + 1):
            j = i - ms + d
            if 0 <= j < B:
                assert band[i, d] == logA[j, i] == logA[j + B, i + B], (i, d)


def test_exports():
    import svcmi.pitch as P
    from svcmi.pitch.core.pyin import pyin, pyin_plan
    from svcmi.svc_inference import F0_METHODS
    assert callable(P.compute_f0_pyin) and callable(P.compute_f0_pyin_begin) and callable(pyin) and callable(pyin_plan)
    assert F0_METHODS == ("crepe", "salience", "pyin")


def test_parsers_take_f0_pyin():
    from svcmi import svc_inference as SI
    from svcmi import svc_inference_batch as SB
    base = ["--config", "c", "--model", "m", "--wave", "w", "--spk", "s"]
    for mod in (SI, SB):
        assert mod.build_parser().parse_args(base).f0 == "crepe"
        assert mod.build_parser().parse_args(base + ["--f0", "pyin"]).f0 == "pyin"
        assert "pyin" in mod.build_parser().format_help()
