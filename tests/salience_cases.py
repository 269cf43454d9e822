"""Checks of the salience F0 extractor (csrc/salience.hip, svcmi.pitch.core.salience, svcmi.pitch.compute_f0_salience), shared by the emulator
tests (CPU) and the GPU tests: every function takes ``ops`` and ``device``.

Oracles, all written here in numpy float64:
  * the STFT: ``np.fft.rfft`` of the zero-padded, Hann-windowed frames.  Bound per element of re and of im, with u = 2^-24 and
    A[t] = sum_i |w_i x_pad[t hop + i]|:  (n_fft + 2) u A[t] + 4 u |oracle|  (any-order fp32 accumulation of n_fft products plus one
    rounding of the table entry; the form of tests/spectrogram_cases.py);
  * the salience map from a given X: ``map_ref``, the reference's steps restated (pitch/core/salience.py:143-272).  The unit of the bound is
    that case's own ``ref_dev``: max |Z_64 - Z_mixed| / max(Z_64), where Z_mixed is the same restatement run the way the reference runs on
    an fp32 signal (complex64 X: fp32 phases and powers, fp32 smoothing and harmonic sums; frequencies and bin positions in float64 like
    the reference's own float64 ``omega``).  Bound: 8 ref_dev max(Z_64), the margin of tests/vad_cases.py.  Binning is discontinuous: a
    frame holding a cell of power >= 1e-10 of the clip's maximum whose float64 bin position lies within 2e-5 bins of a rounding boundary
    is set aside (at most 5 % of a clip's frames);
  * the trajectory: ``dp_ref``, the float64 dynamic programme with numpy's argmax (lowest index on ties), equal index for index.
"""
import functools
import os

import numpy as np
import torch

U = 2.0 ** -24
EPS32 = float(np.finfo(np.float32).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = dict(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, R=10.0, num_harm=10, freq_smooth_len=11, alpha=0.9, gamma=0.0, tol=5,
         score_low=0.01, score_high=1.0)
CLIPS = ("035", "010", "glide")
LOG_HI = float(np.log(np.float64(1.0) + np.float32(EPS32)))          # float64 + the fp32 eps, as the reference does it
LOG_LO = float(np.log(np.float64(0.01) + np.float32(EPS32)))


@functools.lru_cache(maxsize=1)
def golden():
    with np.load(os.path.join(GOLDEN, "salience_f0.npz")) as z:
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


def plan(device):
    from svcmi.pitch.core import salience as S
    return S.salience_plan(device=device, **P)


def sync(ops):
    if ops.on_gpu:
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1. the STFT
def tone_noise(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / P["Fs"]
    return (0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.25 * np.sin(2 * np.pi * 1333.0 * t + 1.0) + 0.05 * rng.standard_normal(n)).astype(np.float32)


def stft_oracle(x32, k_lo, n_bins):
    """x32 float32 [n] -> (X complex128 [frames, n_bins], A float64 [frames])."""
    N, H = P["N"], P["H"]
    xp = np.pad(np.asarray(x32, dtype=np.float64), N // 2)
    frames = 1 + len(x32) // H
    idx = np.arange(N)[None, :] + H * np.arange(frames)[:, None]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    fr = xp[idx] * w
    return np.fft.rfft(fr, axis=1)[:, k_lo:k_lo + n_bins], np.abs(fr).sum(axis=1)


def stft_ratio(X_dev, x32, pl):
    ref, A = stft_oracle(x32, pl.k_lo, pl.n_bins)
    got = X_dev.cpu().numpy()
    assert got.dtype == np.complex64 and got.shape == ref.shape, (got.shape, ref.shape)
    worst = 0.0
    for part in (np.real, np.imag):
        err = np.abs(part(got).astype(np.float64) - part(ref))
        bound = (P["N"] + 2) * U * A[:, None] + 4 * U * np.abs(part(ref))
        assert np.isfinite(err).all()
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def check_stft_frames(ops, device, T):
    """T frames (n = 320 (T - 1) + 17 samples) against float64 rfft; returns the worst error / bound."""
    pl = plan(device)
    x = tone_noise(P["H"] * (T - 1) + 17, seed=T)
    X = ops.salience_stft(pl.struct, torch.from_numpy(x).to(device))
    sync(ops)
    assert tuple(X.shape) == (T, pl.n_bins)
    r = stft_ratio(X, x, pl)
    assert r <= 1.0, r
    return r


def check_stft_clip(ops, device, name="035"):
    pl = plan(device)
    x = clip(name)
    X = ops.salience_stft(pl.struct, torch.from_numpy(x).to(device))
    sync(ops)
    r = stft_ratio(X, x, pl)
    assert r <= 1.0, r
    return r


def check_stft_bits(ops, device):
    """The bits of a frame depend on its 2048 padded samples alone.  The same 40-frame signal three ways: on its own; embedded between 1280
    real zeros on each side (the first and last frames then lie wholly in zeros and are exactly 0; the inner frames sit four columns
    further on in another tile position, and see real zeros where the first run saw padding); and as an offset view into a wider buffer,
    on another stream on the GPU."""
    pl = plan(device)
    H = P["H"]
    s = tone_noise(H * 40 + 5, seed=11)
    base = ops.salience_stft(pl.struct, torch.from_numpy(s).to(device))
    emb = np.concatenate([np.zeros(4 * H, np.float32), s, np.zeros(4 * H - 5, np.float32)])
    wide = ops.salience_stft(pl.struct, torch.from_numpy(emb).to(device))
    buf = torch.full((s.shape[0] + 64,), 3.0, dtype=torch.float32, device=device)
    buf[3:3 + s.shape[0]] = torch.from_numpy(s).to(device)
    view = buf[3:3 + s.shape[0]]
    assert view.data_ptr() % 16 != 0
    if ops.on_gpu:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            off = ops.salience_stft(pl.struct, view)
        torch.cuda.current_stream().wait_stream(side)
    else:
        off = ops.salience_stft(pl.struct, view)
    sync(ops)
    T = base.shape[0]
    assert T == 41 and wide.shape[0] == T + 8
    assert not bool(wide[0].abs().max() > 0) and not bool(wide[-1].abs().max() > 0)
    assert bool(base.abs().max() > 0)
    assert torch.equal(torch.view_as_real(wide[4:4 + T]), torch.view_as_real(base))
    assert torch.equal(torch.view_as_real(off), torch.view_as_real(base))


# ------------------------------------------------------------------------------------------------ 2. the salience map
def harmonic_vector(B):
    md = 5
    window = np.cos(np.linspace(-1, 1, 2 * md + 1) * np.pi / 2) ** 2
    harmonics = np.round(np.log2(np.arange(1, P["num_harm"] + 1)) * 1200 / P["R"]).astype(int)
    vec = np.zeros(B + md)
    for idx, h in enumerate(harmonics):
        if h + 11 > len(vec):
            break
        vec[h:h + 11] += window * P["alpha"] ** idx
    return vec, -len(vec) // 2 + md


def map_ref(X, k_lo, mixed=False):
    """X complex [frames, n_bins] (bins k_lo ..) -> dict(lf_raw, lf, z_raw, z: float64 [frames, B]; pos: float64 bin positions
    [frames, n_bins] (NaN where masked); power [frames, n_bins]).  ``mixed``: the arithmetic of the reference on a complex64 X."""
    from scipy import ndimage
    N, H, Fs, F_min, F_max, R = P["N"], P["H"], P["Fs"], P["F_min"], P["F_max"], P["R"]
    rt = np.float32 if mixed else np.float64
    Xc = np.asarray(X).astype(np.complex64 if mixed else np.complex128)
    B = int(np.floor((1200 / R) * np.log2(F_max / F_min) + 0.5)) + 1
    k = np.arange(k_lo, k_lo + Xc.shape[1])[None, :]
    omega = 2 * np.pi * k / N
    ang = np.angle(Xc)
    hpi = (ang[1:] - ang[:-1]) - omega * H
    hpi = hpi - 2 * np.pi * (np.around((hpi / (2 * np.pi)) + 1) - 1)
    inst_f = (omega + hpi / H) * Fs / (2 * np.pi)
    inst_f = np.vstack([inst_f[:1], inst_f])
    valid = np.logical_and(inst_f >= F_min, inst_f < F_max)
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = np.where(valid, (1200 / R) * np.log2(np.where(valid, inst_f, F_min) / F_min) + 0.5, np.nan)
    bins = np.where(valid, np.floor(np.nan_to_num(pos)), B).astype(np.int64)
    power = (np.abs(Xc) ** 2).astype(rt)
    Y = np.zeros((Xc.shape[0], B + 1), dtype=rt)
    for t in range(Xc.shape[0]):
        np.add.at(Y[t], bins[t], power[t])
    Y = Y[:, :B]
    lf_raw = ndimage.convolve1d(Y, np.hanning(P["freq_smooth_len"]).astype(rt), axis=1, mode="constant")
    with np.errstate(invalid="ignore", divide="ignore"):
        lf = lf_raw * ((20 * np.log10(lf_raw.astype(np.float64) / np.float64(np.max(lf_raw)) + EPS32)) < P["gamma"])
        vec, origin = harmonic_vector(B)
        z_raw = ndimage.correlate1d(lf.astype(rt), vec.astype(rt), axis=1, mode="constant", cval=0, origin=origin)
        z = z_raw * ((20 * np.log10(z_raw.astype(np.float64) / np.float64(np.max(z_raw)) + EPS32)) < P["gamma"])
    return dict(lf_raw=lf_raw.astype(np.float64), lf=lf.astype(np.float64), z_raw=z_raw.astype(np.float64), z=z.astype(np.float64), pos=pos,
                power=power.astype(np.float64))


def set_aside(ref):
    """Frames holding a cell of power >= 1e-10 of the clip's maximum within 2e-5 bins of a rounding boundary."""
    pos, power = ref["pos"], ref["power"]
    near = np.abs(pos - np.round(pos)) < 2e-5                       # pos = 120 log2(f / F_min) + 0.5: floor() jumps at integers
    return np.any(np.nan_to_num(near, nan=0).astype(bool) & (power >= 1e-10 * power.max()), axis=1)


@functools.lru_cache(maxsize=None)
def clip_map_ref(name):
    """(X complex64 [frames, n_bins], ref64, ref_dev, keep mask) of a clip: computed once, shared, never modified."""
    from svcmi.pitch.core import salience as S
    k_lo, k_hi = S.stft_bin_range(P["Fs"], P["N"], P["H"], P["F_min"], P["F_max"])
    X64, _ = stft_oracle(clip(name), k_lo, k_hi - k_lo + 1)
    X = X64.astype(np.complex64)
    r64, rmx = map_ref(X, k_lo), map_ref(X, k_lo, mixed=True)
    keep = ~set_aside(r64)
    assert (~keep).mean() <= 0.05, f"{name}: {(~keep).mean():.3f} of the frames set aside"
    zmax = r64["z"].max()
    ref_dev = float(np.abs(r64["z"][keep] - rmx["z"][keep]).max() / zmax)
    assert 1e-8 < ref_dev < 1e-5, ref_dev
    return X, r64, ref_dev, keep


def check_map_clip(ops, device, name):
    """The device map from the clip's complex64 X against the float64 restatement; returns (worst error / bound, ref_dev, set-aside share)."""
    X, r64, ref_dev, keep = clip_map_ref(name)
    pl = plan(device)
    lf, z, gmax = ops.salience_map(pl.struct, torch.from_numpy(X).to(device))
    sync(ops)
    lf, z = lf.cpu().numpy().astype(np.float64), z.cpu().numpy().astype(np.float64)
    assert lf.shape == r64["lf"].shape == z.shape and np.isfinite(z).all() and np.isfinite(lf).all()
    zmax = r64["z"].max()
    ratio = float(np.abs(z[keep] - r64["z"][keep]).max() / (8 * ref_dev * zmax))
    lf_ratio = float(np.abs(lf[keep] - r64["lf"][keep]).max() / (8 * ref_dev * r64["lf"].max()))
    print(f"salience map {name}: worst |Z_dev - Z_64| / bound {ratio:.3f} (lf {lf_ratio:.3f}), ref_dev {ref_dev:.2e}, set aside {(~keep).mean():.3f}")
    assert ratio <= 1.0 and lf_ratio <= 1.0, (ratio, lf_ratio)
    # the two quirks: the global-maximum cell of lf_spec and of Z is exactly 0 (and was the maximum: gmax holds its bits)
    g = gmax.cpu().numpy().view(np.float32).astype(np.float64)
    for dev, raw, mx in ((lf, r64["lf_raw"], g[0]), (z, r64["z_raw"], g[1])):
        t, b = np.unravel_index(np.argmax(raw), raw.shape)
        assert keep[t], "the global maximum sits in a frame that was set aside: pick another clip"
        assert dev[t, b] == 0.0 and mx > dev.max() and abs(mx - raw[t, b]) <= 8 * ref_dev * raw[t, b]
        assert int((dev == 0.0).sum()) >= 1 and np.count_nonzero(dev) > dev.size // 4
    return ratio, ref_dev, float((~keep).mean())


def check_map_silence(ops, device):
    """An all-zero X: max = 0 makes the threshold's quotient NaN, which compares false: all-zero maps, no NaN."""
    pl = plan(device)
    lf, z, gmax = ops.salience_map(pl.struct, torch.zeros(5, pl.n_bins, dtype=torch.complex64, device=device))
    sync(ops)
    assert not bool(lf.any()) and not bool(z.any()) and not bool(torch.isnan(z).any()) and not bool(gmax.any())


# ------------------------------------------------------------------------------------------------ 3. the trajectory
def dp_ref(Z, tol=5, log_hi=LOG_HI, log_lo=LOG_LO):
    """Z float [frames, B] -> path int64 [frames]: pitch/core/salience.py:306-349 in float64 (time-major here)."""
    Z = np.asarray(Z, dtype=np.float64)
    T, B = Z.shape
    eps = np.finfo(np.float32).eps
    Z_log = np.log(Z + eps)
    d = np.abs(np.arange(B)[:, None] - np.arange(B)[None, :])
    T_log = np.where(d <= tol, log_hi, log_lo)
    D = Z_log[0].copy()
    E = np.zeros((T, B), dtype=np.int64)
    for n in range(1, T):
        M = T_log + D[None, :]
        E[n] = np.argmax(M, axis=1)
        D = np.max(M, axis=1) + Z_log[n]
    path = np.zeros(T, dtype=np.int64)
    path[T - 1] = int(np.argmax(D))
    for n in range(T - 2, -1, -1):
        path[n] = E[n + 1][path[n + 1]]
    return path


def dp_dev(ops, device, Z, tol=5, log_hi=LOG_HI, log_lo=LOG_LO):
    out = ops.salience_dp(torch.from_numpy(np.ascontiguousarray(Z, dtype=np.float32)).to(device), tol, log_hi, log_lo)
    sync(ops)
    return out.cpu().numpy().astype(np.int64)


def random_z(T, B, seed):
    """A sparse, peaky map like the real one: mostly small values, a few large ones per frame."""
    rng = np.random.default_rng(seed)
    Z = rng.random((T, B)) ** 8
    Z[rng.random((T, B)) < 0.3] = 0.0
    return Z.astype(np.float32)


def check_dp_random(ops, device, T, B=636, tol=5, seed=0):
    Z = random_z(T, B, seed + 31 * T + B)
    want = dp_ref(Z, tol)
    got = dp_dev(ops, device, Z, tol)
    assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[:8], want[:8])
    return got


def check_dp_zero_columns(ops, device):
    """Whole frames of zeros: every state ties exactly, the lowest index wins -- also as the final state."""
    Z = random_z(12, 636, 5)
    Z[3:6] = 0.0
    Z[11] = 0.0
    want = dp_ref(Z)
    assert np.array_equal(dp_dev(ops, device, Z), want)
    allz = np.zeros((4, 636), np.float32)
    assert np.array_equal(dp_dev(ops, device, allz), np.zeros(4, np.int64)) and not dp_ref(allz).any()


@functools.lru_cache(maxsize=1)
def rounding_tie_case():
    """(Z float32 [4, 64], tol, expected path): at frame 2 the states j1 = 10 < j2 = 30 hold D[j1] < D[j2], a rounding apart -- the SAME
    three logarithms added in two orders -- and both are out of band for state 50, where fl(log_lo + D[j1]) == fl(log_lo + D[j2]).
    numpy's argmax over the rounded sums returns j1; a banded programme that takes the out-of-band argmax from D returns j2.
    The three values are searched among seeded candidates whose logarithm lies within 0.1 ulp of a double (checked in extended precision):
    any libm with an error below 0.9 ulp then returns the same double, so the construction does not depend on who computes the log."""
    rng = np.random.default_rng(123)
    v = rng.uniform(0.5, 4.0, 2000).astype(np.float32)
    eps = np.finfo(np.float32).eps
    L = np.log(v.astype(np.float64) + eps)
    assert np.finfo(np.longdouble).nmant >= 63, "extended precision is needed to certify the logarithms"
    Ll = np.log(v.astype(np.longdouble) + np.longdouble(eps))
    safe = np.abs((Ll - L.astype(np.longdouble)).astype(np.float64)) <= 0.1 * np.spacing(np.abs(L))
    v, L = v[safe], L[safe]
    i, j, k = (rng.integers(0, len(v), 200000) for _ in range(3))
    a = (LOG_HI + ((LOG_HI + L[i]) + L[j])) + L[k]      # the values v[i], v[j], v[k] at frames 0, 1, 2
    b = (LOG_HI + ((LOG_HI + L[k]) + L[j])) + L[i]      # ... and v[k], v[j], v[i]
    spread = np.maximum(np.maximum(L[i], L[j]), L[k]) - np.minimum(np.minimum(L[i], L[j]), L[k])
    hit = np.nonzero((a < b) & ((LOG_LO + a) == (LOG_LO + b)) & (spread < 1.0))[0]
    assert len(hit), "no rounding tie among the candidates"
    h = hit[0]
    Z = np.zeros((4, 64), np.float32)
    Z[0, 10], Z[1, 10], Z[2, 10] = v[i[h]], v[j[h]], v[k[h]]          # D[10, 2] = a   (the smaller)
    Z[0, 30], Z[1, 30], Z[2, 30] = v[k[h]], v[j[h]], v[i[h]]          # D[30, 2] = b
    Z[3, 50] = 1.0
    want = dp_ref(Z, 5)
    assert list(want) == [10, 10, 10, 50], want
    return Z, 5, want


def check_dp_rounding_tie(ops, device):
    Z, tol, want = rounding_tie_case()
    got = dp_dev(ops, device, Z, tol)
    assert np.array_equal(got, want), (got, want)


def check_dp_limits(ops, device):
    """B at the kernel's limit (1024), a small B with tol >= B (every transition cheap), and T = 2."""
    for T, B, tol in ((5, 1024, 5), (9, 7, 9), (2, 636, 5), (2, 65, 0)):
        check_dp_random(ops, device, T, B, tol, seed=3)
    z = torch.zeros(4, 1025, dtype=torch.float32, device=device)
    f = ops.lib.svcmi_salience_dp_f64
    ptr = torch.zeros(4 * 1025, dtype=torch.int16, device=device)
    path = torch.full((4,), -7, dtype=torch.int32, device=device)
    assert f(z.data_ptr(), 4, 1025, 5, LOG_HI, LOG_LO, ptr.data_ptr(), path.data_ptr(), ops._stream()) == -2
    assert f(z.data_ptr(), 4, 64, 1025, LOG_HI, LOG_LO, ptr.data_ptr(), path.data_ptr(), ops._stream()) == -2
    assert f(z.data_ptr(), 1, 64, 5, LOG_HI, LOG_LO, ptr.data_ptr(), path.data_ptr(), ops._stream()) == -1
    sync(ops)
    assert bool((path == -7).all())


def check_dp_repeatable(ops, device):
    """The same path on a second run and, on the GPU, on another stream."""
    Z = random_z(33, 636, 17)
    first = dp_dev(ops, device, Z)
    assert np.array_equal(first, dp_dev(ops, device, Z))
    if ops.on_gpu:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            again = ops.salience_dp(torch.from_numpy(Z).to(device), 5, LOG_HI, LOG_LO)
        side.synchronize()
        assert np.array_equal(first, again.cpu().numpy())
    assert np.array_equal(first, dp_ref(Z))


# ------------------------------------------------------------------------------------------------ 4. end to end
def check_end_to_end(ops, device, name):
    """waveform -> path equal to the golden path in every frame; compute_f0_salience equal to the golden track bit for bit; sal inside
    the map's bound (a quotient of two map values: twice the bound over the column maximum)."""
    from svcmi.pitch import compute_f0_salience
    g = golden()
    x = clip(name)
    pl = plan(device)
    want = g[f"path_{name}"].astype(np.int64)
    track = compute_f0_salience(x, device, ops=ops)
    assert track.dtype == np.float64 and track.shape == (2 * len(want),)
    assert np.array_equal(track, g[f"track_{name}"]), int((track != g[f"track_{name}"]).sum())
    path, z = ops.salience_f0_fwd(pl.struct, torch.from_numpy(x).to(device), want_map=True)
    sync(ops)
    assert np.array_equal(path.cpu().numpy().astype(np.int64), want)
    X, r64, ref_dev, keep = clip_map_ref(name)
    zd = z.cpu().numpy().astype(np.float64)
    sal = zd[np.arange(len(want)), want] / zd.max(axis=1)
    bound = 2 * 8 * ref_dev * r64["z"].max() / r64["z"].max(axis=1)
    err = np.abs(sal - g[f"sal_{name}"])
    assert np.isfinite(sal).all() and float((err[keep] / bound[keep]).max()) <= 1.0, float((err[keep] / bound[keep]).max())
    # a few stored columns of the reference's own Z against the device map (the device STFT is not the oracle's X: twice the map's bound)
    rows = [i for i, c in enumerate(g["zcols"]) if keep[int(c)]]
    assert rows and float(np.abs(zd[g["zcols"][rows]] - g[f"zcols_{name}"][rows]).max()) <= 2 * 8 * ref_dev * float(g[f"zmax_{name}"])
    return sal


def check_salience_api(ops, device, name="glide"):
    """``salience`` returns (f0, T_coef, sal) like the reference: float64, f0 from the float64 table at the golden path, sal equal to the
    quotient computed from the device map on the host."""
    from svcmi.pitch.core.salience import salience
    want = golden()[f"path_{name}"].astype(np.int64)
    f0, t_coef, sal = salience(clip(name), Fs=16000, H=320, N=2048, F_min=45.0, F_max=1760.0, device=device, ops=ops)
    assert f0.dtype == np.float64 and np.array_equal(f0, plan(device).F_coef_hertz[want])
    assert np.array_equal(t_coef, np.arange(len(want)) * 320 / 16000)
    assert sal.dtype == np.float64 and np.array_equal(sal, check_end_to_end(ops, device, name))


def check_edges(ops, device):
    """Silence gives 45.0 Hz throughout (every state ties: the lowest bin); 319 samples raise ValueError; 320 give 2 frames."""
    from svcmi.pitch import compute_f0_salience
    from svcmi.pitch.core.salience import salience
    f0, _, _ = salience(np.zeros(3200, np.float32), Fs=16000, H=320, N=2048, F_min=45.0, F_max=1760.0, device=device, ops=ops)
    assert f0.shape == (11,) and bool((f0 == 45.0).all())
    try:
        compute_f0_salience(np.zeros(319, np.float32), device, ops=ops)
    except ValueError:
        pass
    else:
        raise AssertionError("319 samples (one frame) did not raise ValueError")
    two = compute_f0_salience(tone_noise(320, seed=2), device, ops=ops)
    assert two.shape == (4,) and np.isfinite(two).all()
    try:
        salience(np.zeros(3200, np.float32), constraint_region=np.zeros((1, 4)), device=device, ops=ops)
    except ValueError:
        pass
    else:
        raise AssertionError("a constraint region did not raise ValueError")


# ------------------------------------------------------------------------------------------------ 5. the command line
CLI_ARGS = ["--config", "cfg.yaml", "--model", "svc.pth", "--wave", "in.wav", "--spk", "spk.npy", "--whisper", "whisper.pt",
            "--hubert", "hubert.pt", "--crepe", "no_such_dir/full.pth", "--f0", "salience"]


def prepare_cli_files(tmp_path, monkeypatch):
    """The tiny seeded models of workload/ and tests/golden/035.wav as the files svc_inference.main reads, in ``tmp_path`` (made the working
    directory); want.csv = save_csv_pitch of the golden track.  No CREPE checkpoint is written: CLI_ARGS names one that does not exist."""
    import json
    import shutil
    import yaml
    from svcmi.pitch.inference import save_csv_pitch
    from workload import config as K
    from workload import inputs as I
    from workload import weights as W
    monkeypatch.chdir(tmp_path)
    hp = K.tiny_hp()
    shutil.copyfile(os.path.join(GOLDEN, "035.wav"), "in.wav")
    torch.save({"model_g": W.make_vits_state(hp, seed=1234)}, "svc.pth")
    torch.save(W.make_whisper_state({**K.WHISPER_TINY_TEST, "n_audio_state": hp.vits.ppg_dim, "n_audio_head": 4}), "whisper.pt")
    torch.save(W.make_hubert_state(dict(K.HUBERT_TINY_TEST, proj=hp.vits.vec_dim)), "hubert.pt")
    np.save("spk.npy", I.synth_spk(hp.vits.spk_dim, seed=7).numpy())
    with open("cfg.yaml", "w") as f:
        yaml.safe_dump(json.loads(json.dumps(hp)), f)
    save_csv_pitch(golden()["track_035"], "want.csv")
