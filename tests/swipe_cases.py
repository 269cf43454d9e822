"""Checks of the SWIPE' F0 extractor (csrc/swipe.hip, svcmi.pitch.core.swipe_slim, svcmi.pitch.compute_f0_swipe), shared by the emulator
tests (CPU) and the GPU tests: every function takes ``ops`` and ``device``.

The target is the reference's pitch/core/swipe_slim.py.  Its steps are restated here as a float64 numpy programme on the plan's float64
tables (``strength_ref``: STFT magnitudes, S_N = K_N (W_N Y) / (||W_N Y|| + eps), scipy's linear interpolation in time written out, the
weighted sum in the reference's order of windows; ``finish_ref``: arg-max, the wrap at index 0, the parabola, the frequency axis).
scripts/make_swipe_golden.py and tests/test_swipe_emu.py prove, where the reference exists, that ``strength_ref`` equals the reference's S
to 1e-13 and that ``finish_ref`` on the reference's S returns its f0 and conf bit for bit.

Bars (set by the feature's issue, derived there):
  * S within S_BAR = 1e-5 absolute of the reference (golden columns) resp. of the float64 programme (built clips).  S is a normalised
    correlation in [-1, 1]; an fp32 model of the whole chain moves it by 1.6e-6; the bar is 6x that and under half the smallest gap between
    a winner and its best rival peak in the golden inputs (2.6e-5; the script asserts every gap >= 2e-5);
  * the arg-max equal in every frame;
  * |f0 - f0_ref| <= f0sens + 1e-9 f0_ref, f0sens = the largest |delta f0| over the 8 sign patterns of +-1e-5 on the three S values the
    parabola reads;
  * |conf - conf_ref| <= 1e-5.
  * the finish kernel from a GIVEN fp32 S against ``finish_ref`` on the same S: arg-max and conf equal exactly, f0 within 1e-9 relative
    (the device's exp2 and the host's pow may differ in the last bits).
"""
import ctypes
import functools
import itertools
import os

import numpy as np
import torch

EPS = 2.0 ** -52
S_BAR = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = dict(Fs=16000, H=320, F_min=45.0, F_max=1760.0, R=10)                 # compute_f0_swipe's parameters: 6 windows 64 .. 2048, B = 635
SMALL = dict(Fs=4000, H=80, F_min=100.0, F_max=800.0, R=50)                 # 4 windows 32 .. 256, B = 72, 104 log bins, table widths 17 .. 129
MID = dict(Fs=16000, H=320, F_min=100.0, F_max=200.0, R=100)                # 2 windows 512 and 1024 (the magnitude kernel's LDS and global forms), B = 12
CLIPS = ("035", "010", "glide")
SCOLS = (0, 1, 50, 99)                                                      # the frames whose S columns the golden file keeps
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3


@functools.lru_cache(maxsize=1)
def golden():
    with np.load(os.path.join(GOLDEN, "swipe_f0.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def clip(name):
    """float32 [n] at 16 kHz: the two wav fixtures decoded as int16 / 32768, the glide from the fixture file."""
    if name == "glide":
        return golden()["wave_glide"]
    from scipy.io import wavfile
    rate, x = wavfile.read(os.path.join(GOLDEN, {"035": "035.wav", "010": "vad_010.wav"}[name]))
    assert rate == 16000 and x.dtype == np.int16 and x.ndim == 1
    return x.astype(np.float32) / 32768.0


def plan(device, geometry=None, **over):
    from svcmi.pitch.core import swipe_slim as W
    return W.swipe_plan(device=device, **{**(geometry or P), **over})


def sync(ops):
    if ops.on_gpu:
        torch.cuda.synchronize()


def tone(n, f, fs, seed=0, harmonics=3, noise=1e-3):
    """A harmonic tone of fundamental ``f`` plus a little seeded noise, float32 [n]."""
    t = np.arange(n) / fs
    x = sum(0.5 ** h * np.sin(2 * np.pi * (h + 1) * f * t + 0.3 * h) for h in range(harmonics))
    return (0.3 * x + noise * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


# ================================================================================================ the float64 programme
def stft_mag(x, N, dtype=np.float64):
    """|librosa.stft(np.pad(x, (0, N)), n_fft=N, hop_length=N // 2, window='hann', center=True, pad_mode='constant')|: [N / 2 + 1, frames]."""
    import scipy.fft
    import scipy.signal
    h = N // 2
    xp = np.pad(np.asarray(x, dtype=dtype), (h, N + h))
    frames = 1 + (len(x) + N) // h
    idx = np.arange(N)[None, :] + h * np.arange(frames)[:, None]
    win = scipy.signal.get_window("hann", N, fftbins=True).astype(dtype)
    return np.abs(scipy.fft.rfft(xp[idx] * win, axis=1)).T


def interp_time(T_coef, S_N, t):
    """scipy's ``interp1d(T_coef, S_N, kind='linear', axis=1)(t)`` written out: the segment below the first axis point >= t."""
    hi = np.clip(np.searchsorted(T_coef, t), 1, len(T_coef) - 1)
    lo = hi - 1
    slope = (S_N[:, hi] - S_N[:, lo]) / (T_coef[hi] - T_coef[lo])[None, :]
    return slope * (t - T_coef[lo])[None, :] + S_N[:, lo]


def strength_ref(x, pl, parts=False):
    """S float64 [B, frames] of pitch/core/swipe_slim.py:71-101 from the plan's float64 tables; ``parts``: also every window's (Y, L, S_N)."""
    x = np.asarray(x)
    t = np.arange(0, len(x), pl.H) / pl.Fs
    S = np.zeros((pl.B, len(t)))
    kept = []
    for w in pl.windows:
        N = w["N"]
        Y = stft_mag(x, N)
        L = w["W"] @ Y
        Ln = L / (np.sqrt(np.sum(L ** 2, axis=0)) + EPS)
        S_N = w["K"] @ Ln
        T_coef = np.arange(0, Y.shape[1]) * (N // 2) / pl.Fs
        S[w["cand"], :] += np.multiply(w["mu"].reshape(-1, 1), interp_time(T_coef, S_N, t))
        kept.append((Y, L, S_N))
    return (S, kept) if parts else S


def parabola(y1, y2, y3):
    a = EPS + (y1 + y3 - 2 * y2) / 2
    b = (y3 - y1) / 2
    return -b / (2 * a)


def axis_f0(pl, xq):
    """F_min 2^(interp1d(arange(n_log), F_coef_log, 'linear')(xq)), extrapolating below 0 (where the reference raises ValueError)."""
    hi = np.clip(np.ceil(xq).astype(np.int64), 1, pl.n_log - 1)
    lo = hi - 1
    slope = (pl.F_coef_log[hi] - pl.F_coef_log[lo]) / (hi.astype(np.float64) - lo.astype(np.float64))
    return pl.F_min * 2 ** (slope * (xq - lo) + pl.F_coef_log[lo])


def finish_ref(S, pl, edge="raise", threshold=None):
    """pitch/core/swipe_slim.py:103-118 on S [B, frames] (any float type, widened to float64): (f0, conf, amax, edge frames).  An arg-max
    at 0 reads row -1 = row B - 1; an arg-max at B - 1 raises the reference's IndexError under ``edge="raise"`` and takes shift 0 under
    ``"clamp"``."""
    S = np.asarray(S, dtype=np.float64)
    B, frames = S.shape
    amax = np.argmax(S, axis=0)
    conf = np.max(S, axis=0)
    cols = np.arange(frames)
    last = amax == B - 1
    if last.any() and edge == "raise":
        raise IndexError(f"index {B} is out of bounds for axis 0 with size {B}")
    up = np.where(last, amax, amax + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        shift = np.where(last, 0.0, parabola(S[amax - 1, cols], S[amax, cols], S[up, cols]))
    f0 = axis_f0(pl, amax + shift)
    f0[conf < (pl.threshold if threshold is None else threshold)] = 0
    return f0, conf, amax, last


def f0_sensitivity(S, pl, delta=1e-5):
    """Per frame the largest |f0' - f0| over the 8 sign patterns of +-delta on the three values the parabola reads (0 in edge frames)."""
    S = np.asarray(S, dtype=np.float64)
    B, frames = S.shape
    f0, _, amax, last = finish_ref(S, pl, edge="clamp", threshold=-np.inf)
    cols = np.arange(frames)
    up = np.where(last, amax, amax + 1)
    y = [S[amax - 1, cols], S[amax, cols], S[up, cols]]
    worst = np.zeros(frames)
    for sg in itertools.product((-1.0, 1.0), repeat=3):
        with np.errstate(divide="ignore", invalid="ignore"):
            shift = np.where(last, 0.0, parabola(*(v + s * delta for v, s in zip(y, sg))))
        worst = np.maximum(worst, np.abs(axis_f0(pl, amax + shift) - f0))
    return worst


def rival_gap(S):
    """Per frame: the winner minus the best OTHER local maximum of the column (inf where there is none)."""
    S = np.asarray(S, dtype=np.float64)
    B, frames = S.shape
    padded = np.vstack((np.full((1, frames), -np.inf), S, np.full((1, frames), -np.inf)))
    peak = (padded[1:-1] > padded[:-2]) & (padded[1:-1] > padded[2:])
    amax = np.argmax(S, axis=0)
    peak[amax, np.arange(frames)] = False
    return np.max(S, axis=0) - np.max(np.where(peak, S, -np.inf), axis=0)


# ================================================================================================ device helpers
def stage(ops, device, pl, x):
    """The stage on clip ``x``: (f0, conf, flags, S [frames, B] float32 numpy)."""
    out, S = ops.swipe_f0_fwd(pl.struct, torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device), want_map=True)
    sync(ops)
    host = out.cpu().numpy()
    return host[0], host[1], int(host[2, 0]), S.cpu().numpy()


def finish_dev(ops, device, pl, S, threshold=None):
    """The finish kernel on a given fp32 S [frames, B]: (f0, conf, amax, flags)."""
    out, amax, flags = ops.swipe_finish(torch.from_numpy(np.ascontiguousarray(S, dtype=np.float32)).to(device), pl.n_log, pl.F_min, pl.step,
                                        pl.threshold if threshold is None else threshold)
    sync(ops)
    host = out.cpu().numpy()
    return host[0], host[1], amax.cpu().numpy().astype(np.int64), int(flags.cpu().numpy()[0])


def check_finish(ops, device, pl, S, f0, conf, flags):
    """f0 / conf / flags (of the stage) against ``finish_ref`` and the finish kernel on the SAME fp32 S.  Returns amax."""
    want_f0, want_conf, want_amax, last = finish_ref(S.T, pl, edge="clamp")
    got_f0, got_conf, got_amax, got_flags = finish_dev(ops, device, pl, S)
    assert np.array_equal(got_f0, f0) and np.array_equal(got_conf, conf) and got_flags == flags, "stage and finish kernel disagree"
    assert np.array_equal(got_amax, want_amax) and flags == int(last.sum())
    assert np.array_equal(conf, want_conf) and not np.isnan(f0).any()
    assert bool((np.abs(f0 - want_f0) <= 1e-9 * np.abs(want_f0)).all()), float(np.abs(f0 - want_f0).max())
    return got_amax


# ================================================================================================ 1. the kernels, one by one
def check_kernels(ops, device, geometry=None, n=700, seed=0):
    """Every window: magnitudes, resampling, strength against the float64 programme, pad columns zero; then the accumulation."""
    pl = plan(device, geometry)
    x = tone(n, 2.3 * pl.F_min, pl.Fs, seed=seed)
    S64, parts = strength_ref(x, pl, parts=True)
    xt = torch.from_numpy(x).to(device)
    sn = []
    worst = {}
    for o, (w, (Y64, L64, SN64)) in enumerate(zip(pl.windows, parts)):
        nb = w["N"] // 2 + 1
        Y = ops.swipe_mag(pl.struct, o, xt)
        L = ops.swipe_resample(pl.struct, o, Y)
        SN = ops.swipe_strength(pl.struct, o, L)
        sync(ops)
        Yh, Lh, SNh = Y.cpu().numpy(), L.cpu().numpy(), SN.cpu().numpy()
        assert Yh.shape == (Y64.shape[1], (nb + 7) & ~7) and not Yh[:, nb:].any() and not Lh[:, pl.n_log:].any()
        scale = max(float(np.abs(Y64).max()), 1e-30)
        # magnitudes: N products of an fp32 table entry (2^-24 relative) and a sample, N additions: N 2^-23 of the largest magnitude is generous
        e_y = float(np.abs(Yh[:, :nb].T - Y64).max()) / scale
        assert e_y <= w["N"] * 2.0 ** -23, (w["N"], e_y)
        e_l = float(np.abs(Lh[:, :pl.n_log].T - L64).max()) / max(float(np.abs(L64).max()), 1e-30)
        e_s = float(np.abs(SNh.T - SN64).max())
        assert e_l <= 2e-5 and e_s <= S_BAR, (w["N"], e_l, e_s)
        worst[w["N"]] = (e_y, e_l, e_s)
        sn.append(SN)
    S = ops.swipe_accum(pl.struct, sn, n)
    sync(ops)
    Sh = S.cpu().numpy()
    assert Sh.shape == (-(-n // pl.H), pl.B)
    e = float(np.abs(Sh.T - S64).max())
    assert e <= S_BAR, e
    return worst, e


# ================================================================================================ 2. the stage on built clips
def last_frame_clip_length(pl):
    """A length whose last output frame lies as late as it can between two frames of the largest window: (frames - 1) H = n - 1."""
    return 5 * pl.H + 1 + 2 * max(pl.N_pow2)


def check_stage_shapes(ops, device, geometry=None):
    """n = 1 (one frame, every window mostly padding), H, H + 1, 2 H (the ceil frame count), a clip shorter than the largest window (700 in
    the default geometry, 200 in the small one) and a clip whose last output frame sits on its last sample: ceil(n / H) frames, S within
    S_BAR of the float64 programme, the finish consistent."""
    pl = plan(device, geometry)
    worst = 0.0
    short = 700 if max(pl.N_pow2) > 700 else 200
    assert short < max(pl.N_pow2)
    for k, n in enumerate((1, pl.H, pl.H + 1, 2 * pl.H, short, last_frame_clip_length(pl))):
        x = tone(n, 3.1 * pl.F_min, pl.Fs, seed=k)
        f0, conf, flags, S = stage(ops, device, pl, x)
        frames = -(-n // pl.H)
        assert f0.shape == conf.shape == (frames,) and S.shape == (frames, pl.B), (n, f0.shape, S.shape)
        e = float(np.abs(S.T - strength_ref(x, pl)).max())
        assert e <= S_BAR, (n, e)
        worst = max(worst, e)
        check_finish(ops, device, pl, S, f0, conf, flags)
    return worst


def check_silence(ops, device, geometry=None):
    """Silence: S = 0 everywhere, arg-max 0, the wrap, shift -0.0: F_min (45 Hz in the default geometry) and conf 0 in every frame, no NaN,
    no flag -- at threshold 0 SWIPE' calls silence voiced, like the reference; any threshold above 0 zeroes it."""
    from svcmi.pitch.core.swipe_slim import swipe_slim
    geometry = geometry or P
    pl = plan(device, geometry)
    n = 3 * pl.H + 40
    f0, conf, flags, S = stage(ops, device, pl, np.zeros(n, np.float32))
    assert not S.any() and flags == 0 and np.array_equal(f0, np.full(4, geometry["F_min"])) and np.array_equal(conf, np.zeros(4))
    f0, t, conf = swipe_slim(np.zeros(n, np.float32), device=device, ops=ops, **geometry)
    assert np.array_equal(f0, np.full(4, geometry["F_min"])) and np.array_equal(t, np.arange(4) * pl.H / pl.Fs) and not conf.any()
    f0, _, _ = swipe_slim(np.zeros(n, np.float32), device=device, ops=ops, strength_threshold=0.1, **geometry)
    assert not f0.any()


def check_last_candidate(ops, device):
    """A tone just above the last candidate: arg-max B - 1.  The flag counts those frames, ``edge="raise"`` raises the reference's
    IndexError with its message, ``edge="clamp"`` returns the last candidate's frequency (shift 0) and conf = max S there."""
    from svcmi.pitch.core.swipe_slim import swipe_slim
    pl = plan(device, SMALL)
    x = tone(800, 1.004 * pl.F_coef_log_hz[pl.B - 1], pl.Fs, harmonics=1)
    f0, conf, flags, S = stage(ops, device, pl, x)
    amax = check_finish(ops, device, pl, S, f0, conf, flags)
    hit = amax == pl.B - 1
    assert flags == int(hit.sum()) and flags >= 1, (flags, amax)
    assert np.array_equal(f0[hit], np.full(flags, axis_f0(pl, np.array([pl.B - 1.0]))[0])) and np.array_equal(conf[hit], S[hit].max(axis=1).astype(np.float64))
    try:
        swipe_slim(x, device=device, ops=ops, **SMALL)
    except IndexError as e:
        assert str(e) == f"index {pl.B} is out of bounds for axis 0 with size {pl.B}"
    else:
        raise AssertionError("edge='raise' did not raise IndexError")
    got, _, got_conf = swipe_slim(x, device=device, ops=ops, edge="clamp", **SMALL)
    assert np.array_equal(got, f0) and np.array_equal(got_conf, conf)


def check_wrap(ops, device):
    """An arg-max at candidate 0: the parabola reads S[B - 1] for S[-1] (numpy's wrap).  A tone at F_min does NOT put the arg-max there (the
    reference analyses its lowest candidates with its smallest window), silence does but with three equal values; so the finish kernel
    runs on a handmade S whose row maximum sits at 0 with S[B - 1] != S[1]: once with S[1] the larger (a positive shift) and once with
    S[B - 1] the larger (a negative refined index: the device extrapolates the axis where the reference's interp1d raises ValueError).
    The tone at F_min goes through the stage all the same and must agree with the programme's finish on the same S."""
    pl = plan(device, SMALL)
    x = tone(800, pl.F_min, pl.Fs, harmonics=4)
    f0, conf, flags, S = stage(ops, device, pl, x)
    check_finish(ops, device, pl, S, f0, conf, flags)
    pl, B = plan(device), plan(device).B
    H = (0.25 * np.random.default_rng(11).random((2, B))).astype(np.float32)
    H[:, 0] = 0.75
    H[0, 1], H[0, B - 1] = 0.70, 0.40
    H[1, 1], H[1, B - 1] = 0.40, 0.70
    f0, conf, amax, flags = finish_dev(ops, device, pl, H)
    assert amax.tolist() == [0, 0] and flags == 0 and np.array_equal(conf, np.full(2, 0.75))
    H64 = H.astype(np.float64)
    shift = parabola(H64[:, B - 1], H64[:, 0], H64[:, 1])
    assert shift[0] > 0.1 and shift[1] < -0.1
    want = pl.F_min * 2 ** (shift * pl.step)
    assert bool((np.abs(f0 - want) <= 1e-9 * want).all()) and f0[0] > 45.0 > f0[1]
    unwrapped = pl.F_min * 2 ** (parabola(H64[:, 0], H64[:, 0], H64[:, 1]) * pl.step)       # what a clamp at row 0 would give
    assert bool((np.abs(f0 - unwrapped) > 1e-3).all())


def check_ties(ops, device):
    """The finish kernel on a handmade S: the lowest index wins an exact tie (np.argmax), also across waves and blocks of the reduction."""
    pl = plan(device)
    B = pl.B
    rng = np.random.default_rng(3)
    S = (0.5 * rng.random((6, B))).astype(np.float32)
    S[0, [5, 9]] = 0.75
    S[1, :] = 0.25                                                       # all equal: index 0, neighbours equal, shift -0.0
    S[2, [2, B - 1]] = 0.75                                              # the last candidate ties with an earlier one: no flag
    S[3, [63, 64, 300, 600]] = 0.75                                      # across lanes, waves and strides of the reduction
    S[4, [B - 2, B - 1]] = 0.75
    S[5, B - 1] = 0.75                                                   # the only edge frame
    f0, conf, amax, flags = finish_dev(ops, device, pl, S)
    assert amax.tolist() == [5, 0, 2, 63, B - 2, B - 1] and flags == 1
    want_f0, want_conf, want_amax, _ = finish_ref(S.T, pl, edge="clamp")
    assert np.array_equal(amax, want_amax) and np.array_equal(conf, want_conf)
    assert bool((np.abs(f0 - want_f0) <= 1e-9 * want_f0).all()) and f0[1] == 45.0


def stage_raw(ops, pl, x, ws_base, ws_bytes, stream):
    """svcmi_swipe_f0_fwd called directly on a caller-chosen workspace and stream: (out float64 [2, frames], S, flags) device tensors."""
    frames = -(-x.shape[0] // pl.H)
    out = torch.empty(2, frames, dtype=torch.float64, device=x.device)
    S = torch.empty(frames, pl.B, dtype=torch.float32, device=x.device)
    flags = torch.empty(1, dtype=torch.int32, device=x.device)
    rc = ops.lib.svcmi_swipe_f0_fwd(ctypes.byref(pl.struct), x.data_ptr(), x.shape[0], out[0].data_ptr(), out[1].data_ptr(), S.data_ptr(),
                                    flags.data_ptr(), ws_base, ws_bytes, stream)
    assert rc == 0, rc
    return out, S, flags


def check_repeatable(ops, device):
    """Two launches of the stage, on different streams (GPU) and workspaces of different alignment, give the same bits."""
    pl = plan(device, SMALL)
    x = torch.from_numpy(tone(1234, 2.7 * pl.F_min, pl.Fs, seed=5)).to(device)
    need = ops.lib.svcmi_swipe_workspace_bytes(ctypes.byref(pl.struct), x.shape[0])
    assert need > 0
    ws = [torch.zeros(need + 8192, dtype=torch.uint8, device=device), torch.full((need + 8192,), 255, dtype=torch.uint8, device=device)]
    base = [((ws[0].data_ptr() + 4095) & ~4095), ((ws[1].data_ptr() + 4095) & ~4095) + 256 * 3]
    res = []
    if ops.on_gpu:
        torch.cuda.synchronize()
        streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
        for b, st in zip(base, streams):
            with torch.cuda.stream(st):
                res.append(stage_raw(ops, pl, x, b, need, st.cuda_stream))
        torch.cuda.synchronize()
    else:
        res = [stage_raw(ops, pl, x, b, need, 0) for b in base]
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a.cpu(), b.cpu())
    f0, conf, flags, S = stage(ops, device, pl, x.cpu().numpy())
    assert np.array_equal(res[0][0].cpu().numpy(), np.stack((f0, conf))) and np.array_equal(res[0][1].cpu().numpy(), S)


# ================================================================================================ 3. the golden clips
def check_golden_is_the_programme():
    """No device: the golden file against the float64 programme on the same clips -- S columns to 1e-13, arg-max, f0 and conf bit for
    bit (through ``finish_ref`` with the clamp rule), every rival gap >= 2e-5."""
    g, pl = golden(), plan("cpu")
    for name in CLIPS:
        S = strength_ref(clip(name), pl)
        f0, conf, amax, last = finish_ref(S, pl, edge="clamp")
        assert float(np.abs(S[:, list(SCOLS)].T - g[f"S_{name}"]).max()) <= 1e-13
        assert np.array_equal(amax, g[f"amax_{name}"]) and int(last.sum()) == (10 if name == "010" else 0)
        assert float(np.abs(conf - g[f"conf_{name}"]).max()) <= 1e-13 and bool((np.abs(f0 - g[f"f0_{name}"]) <= 1e-6 * g[f"f0sens_{name}"] + 1e-12 * f0).all())
        assert float(g[f"rival_{name}"].min()) >= 2e-5


def check_end_to_end(ops, device, name):
    """clip -> S columns within S_BAR of the reference's, the arg-max equal in EVERY frame, f0 within f0sens + 1e-9 f0, conf within 1e-5.
    Prints and returns the deviations (S, the worst f0 deviation in units of its tolerance, conf)."""
    g, pl = golden(), plan(device)
    x = clip(name)
    f0, conf, flags, S = stage(ops, device, pl, x)
    want, sens = g[f"f0_{name}"], g[f"f0sens_{name}"]
    assert f0.shape == want.shape == (-(-len(x) // P["H"]),)
    amax = check_finish(ops, device, pl, S, f0, conf, flags)
    e_s = float(np.abs(S[list(SCOLS)].astype(np.float64) - g[f"S_{name}"]).max())
    e_f = float((np.abs(f0 - want) / (sens + 1e-9 * want)).max())
    e_c = float(np.abs(conf - g[f"conf_{name}"]).max())
    print(f"swipe {name}: |S - S_ref| {e_s:.2e}, arg-max differs in {int((amax != g[f'amax_{name}']).sum())} frames, f0 at {e_f:.3f} of its "
          f"tolerance (largest |f0 - f0_ref| {float(np.abs(f0 - want).max()):.2e} Hz), |conf - conf_ref| {e_c:.2e}, {flags} edge frames")
    assert np.array_equal(amax, g[f"amax_{name}"].astype(np.int64)), int((amax != g[f"amax_{name}"]).sum())
    assert e_s <= S_BAR, e_s
    assert e_f <= 1.0, e_f
    assert e_c <= 1e-5, e_c
    assert flags == int((g[f"amax_{name}"] == pl.B - 1).sum())
    return e_s, e_f, e_c


def check_api(ops, device, geometry=None, x=None):
    """``swipe_slim`` returns (f0, t, conf) like the reference: float64, the stage's values, t = arange(0, n, H) / Fs; ``edge`` is checked."""
    from svcmi.pitch.core.swipe_slim import swipe_slim
    geo = geometry or P
    x = clip("glide") if x is None else x
    f0, t, conf = swipe_slim(x, device=device, ops=ops, edge="clamp", **geo)
    want_f0, want_conf, _, _ = stage(ops, device, plan(device, geo), x)
    assert f0.dtype == t.dtype == conf.dtype == np.float64 and np.array_equal(f0, want_f0) and np.array_equal(conf, want_conf)
    assert np.array_equal(t, np.arange(0, len(x), geo["H"]) / geo["Fs"]) and len(t) == len(f0)
    for bad in (dict(edge="wrap"), dict(R=1), dict(F_min=2.0), dict(F_max=9000.0)):     # 6350 candidates; 12 window sizes; F_max above Fs / 2
        try:
            swipe_slim(x[:400], device=device, ops=ops, **{**P, **bad})
        except ValueError:
            pass
        else:
            raise AssertionError(f"{bad} did not raise ValueError")
    try:
        swipe_slim(np.zeros(0, np.float32), device=device, ops=ops, **P)
    except ValueError:
        pass
    else:
        raise AssertionError("an empty clip did not raise ValueError")


def check_compute_f0_swipe(ops, device, name="035"):
    """The recipe: float64 [2 ceil(n / 320)], every frame twice, no moving average, the clamp rule (010 has edge frames and must not raise)."""
    from svcmi.pitch import compute_f0_swipe
    x = clip(name)
    track = compute_f0_swipe(x, device, ops=ops)
    f0, _, _, _ = stage(ops, device, plan(device), x)
    assert track.dtype == np.float64 and track.shape == (2 * (-(-len(x) // 320)),)
    assert np.array_equal(track[0::2], track[1::2]) and np.array_equal(track[0::2], f0) and bool((f0 > 0).all())
    gated = compute_f0_swipe(x, device, strength_threshold=0.3, ops=ops)
    assert np.array_equal(gated == 0, np.repeat(stage(ops, device, plan(device), x)[1] < 0.3, 2)) and 0 < int((gated == 0).sum()) < len(gated)
    return track


# ================================================================================================ 4. the command line
CLI_ARGS = ["--config", "cfg.yaml", "--model", "svc.pth", "--wave", "in.wav", "--spk", "spk.npy", "--whisper", "whisper.pt",
            "--hubert", "hubert.pt", "--crepe", "no_such_dir/full.pth", "--f0", "swipe"]


def prepare_cli_files(tmp_path, monkeypatch, n=None):
    """The files svc_inference.main reads (tests/salience_cases.py makes them; in.wav is 035.wav) in ``tmp_path``; ``n``: in.wav cut to its
    first n samples (the emulator's budget).  Returns the clip the command reads."""
    from scipy.io import wavfile
    from tests import salience_cases as S
    S.prepare_cli_files(tmp_path, monkeypatch)
    rate, pcm = wavfile.read("in.wav")
    assert rate == 16000 and np.array_equal(pcm.astype(np.float32) / 32768.0, clip("035"))
    if n is not None:
        wavfile.write("in.wav", rate, pcm[:n])
    return clip("035")[:n]


def check_csv(path, want, tol=None):
    """svc_tmp.pit.csv against a track: int() of it exactly, or (``tol``) of a value within the tolerance."""
    from svcmi.pitch.inference import load_csv_pitch
    got = np.array(load_csv_pitch(path), dtype=np.float64)
    tol = np.zeros_like(want) if tol is None else tol
    assert got.shape == want.shape and bool(((got >= np.floor(want - tol)) & (got <= np.floor(want + tol))).all())
    return got
