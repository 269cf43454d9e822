"""Checks of the pYIN F0 extractor (csrc/pyin.hip, svcmi.pitch.core.pyin, svcmi.pitch.compute_f0_pyin), shared by the emulator tests (CPU)
and the GPU tests: every function takes ``ops`` and ``device``.

The target is the reference's pitch/core/pyin.py AS IT EXECUTES under numpy with ``numba.njit`` as the identity.  Its steps are restated here
as a float64 numpy programme (``observe_frame``, ``normalise``, ``viterbi_dense``, ``finish_ref``, composed in ``pyin_ref``);
tests/test_pyin_emu.py and scripts/make_pyin_golden.py prove the programme equal to the reference bit for bit where the reference exists.

Oracles and bounds:
  * CMNDF and RMS: an ``np.longdouble`` oracle, compared per element with a RELATIVE bound.  With u = 2^-53 and N the frame length:
      - a difference x[j] - x[j + tau] of two fp32 values rounds once in fp64 (1 u), its square once more (3 u in all);
      - a sum of at most N non-negative terms in ANY order adds at most (N - 1) u: d(tau) carries at most (N + 2) u;
      - the running mean m = m (tau - 1) / tau + d / tau is a sum of non-negative parts, each step adds 3 u to what is already there
        and 2 u to the new term: after p_max <= N steps at most (3 N + N + 2) u;
      - the quotient d / (m + eps) adds 2 u and the errors of d and m: (N + 2) + (4 N + 2) + 2 <= 5 (N + 2) u.
    So |c_dev - c| <= CMNDF_C (N + 2) u |c| with CMNDF_C = 5 (first order; the oracle's own error is 2^-11 of that).  The RMS -- exact
    squares, N - 1 additions, a division, a square root -- stays below (N + 2) u.  DELTA = 5 (2048 + 2) u = 1.14e-12 is the perturbation
    under which scripts/make_pyin_golden.py asserts the reference's own decisions unchanged.
  * the observation kernel from given CMNDF rows: equal to ``observe_frame`` + ``normalise`` bit for bit, NaN positions included;
  * Viterbi from a given logO: equal to ``viterbi_dense`` index for index;
  * end to end on the golden clips: path, voicing and conf equal, |f0 - f0_golden| <= 8 f0sens + 4 u f0_golden per frame (f0sens: how far
    the reference's own f0 moves under DELTA, through the refinement only).
"""
import functools
import os

import numpy as np
import torch

U = 2.0 ** -53
EPS = 2.0 ** -52
TINY = float(np.finfo(0.).tiny)
CMNDF_C = 5.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = dict(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0)            # compute_f0_pyin's parameters
SMALL = dict(Fs=16000, N=64, H=1, F_min=250.0, F_max=4000.0)            # the smallest geometry: p_max = N, hop 1
DELTA = CMNDF_C * (P["N"] + 2) * U
CLIPS = ("035", "010", "glide")
ROWS = (0, 1, 50, 100)                                                   # the frames whose CMNDF rows / O columns the golden file keeps


@functools.lru_cache(maxsize=1)
def golden():
    with np.load(os.path.join(GOLDEN, "pyin_f0.npz")) as z:
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


def plan(device, **over):
    from svcmi.pitch.core import pyin as Y
    return Y.pyin_plan(device=device, **{**P, **over})


def sync(ops):
    if ops.on_gpu:
        torch.cuda.synchronize()


def same_bits(a, b):
    """Equal bit for bit, any NaN equal to any NaN at the same place."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


# ================================================================================================ the float64 programme
def frames_of(x, N, H):
    """float64 [frames, N]: the centred frames of the zero-padded clip."""
    xp = np.concatenate((np.zeros(N // 2), np.asarray(x, dtype=np.float64), np.zeros(N // 2)))
    M = (len(xp) - N) // H + 1
    return xp[np.arange(N)[None, :] + H * np.arange(M)[:, None]]


def cmndf_f64(frame, p_max):
    """The CMNDF in float64 with numpy's own summation order (what the reference computes)."""
    c = np.zeros(p_max + 1)
    c[0] = 1
    mean = 0
    for tau in range(1, p_max + 1):
        d = np.sum((frame[0:-tau] - frame[tau:]) ** 2)
        mean = mean * (tau - 1) / tau + d / tau
        c[tau] = d / (mean + EPS)
    return c


def observe_frame(c, thresholds, beta, p_min, p_max, amp, F_axis, Fs):
    """Steps 1-6 for one CMNDF row -> (O_m float64 [B] (the voiced half, before normalisation), lag_thr, val_thr, info)."""
    c = np.array(c, dtype=np.float64)
    B, nt = len(F_axis), len(thresholds)
    c[:p_min] = np.inf
    c[p_max] = np.inf
    inner = np.arange(1, p_max)
    M = inner[(c[1:-1] < c[:-2]) & (c[1:-1] < c[2:])]
    info = dict(L=len(M), quirk=False, nan_lag=False, nan_val=False, border_lo=False, border_hi=False, fallback=0)
    O = np.zeros(B)
    if len(M) == 0:
        return O, np.full(nt, float(p_min)), np.ones(nt), info
    L = len(M)
    info["border_lo"], info["border_hi"] = bool(M[0] == p_min), bool(M[-1] == p_max - 1)
    quirk = bool(M[-1] == p_max - 1 and (L - 1) in M)                  # the "deletion" that drops the first minimum
    info["quirk"] = quirk
    I = M[1:] if quirk else M
    y1, y2, y3 = c[I - 1], c[I], c[I + 1]
    with np.errstate(invalid="ignore"):
        a = EPS + (y1 + y3 - 2 * y2) / 2
        b = (y3 - y1) / 2
        corr = -b / (2 * a)
        c[I] = y2 - (b * b) / (4 * a)
    corr0 = 0.0 if M[0] == p_min else float(corr[0])
    nan_at = np.flatnonzero(np.isnan(c))
    if len(nan_at):
        g_idx, g_val = int(nan_at[0]), np.nan
    else:
        g_idx = int(np.argmin(c))
        g_val = c[g_idx]
    cm = c[M]
    lag_thr, val_thr = np.zeros(nt), np.zeros(nt)
    for i in range(nt):
        below = np.flatnonzero(cm < thresholds[i])                      # NaN is never below a threshold
        if len(below):
            m = M[below[0]]
            lag, val, w = m + corr0, c[m], beta[i]
        else:
            lag, val, w = float(g_idx), g_val, amp * beta[i]
            info["fallback"] += 1
        if lag < p_min:
            lag = float(p_min)
        elif lag >= p_max:
            lag = float(p_max - 1)
        lag_thr[i], val_thr[i] = lag, val
        if np.isnan(lag):
            idx, info["nan_lag"] = 0, True
        else:
            idx = int(np.argmin(np.abs(1200 * np.log2(F_axis / (Fs / lag)))))
        info["nan_val"] |= bool(np.isnan(val))
        O[idx] += w
    return O, lag_thr, val_thr, info


def normalise(Ov, voicing_prob):
    """Step 7: Ov float64 [B, frames] -> O [2B, frames]."""
    B = Ov.shape[0]
    O = np.zeros((2 * B, Ov.shape[1]))
    O[0:B, :] = Ov
    O[0:B, :] *= voicing_prob
    O[B:2 * B, :] = (1 - voicing_prob) * (1 - np.sum(O[0:B, :], axis=0)) / B
    return O


def observe_rows(rows, pl, amp=0.01, voicing_prob=0.5):
    """rows float64 [frames >= 2, p_max + 1] -> (O [2B, frames], lag_thr [n_thr, frames], val_thr, infos)."""
    assert len(rows) >= 2, "np.sum(axis=0) of a single column may take another summation order"
    out = [observe_frame(r, pl.thresholds_np, pl.beta_np, pl.p_min, pl.p_max, amp, pl.F_axis, pl.Fs) for r in rows]
    O = normalise(np.stack([o[0] for o in out], axis=1), voicing_prob)
    return O, np.stack([o[1] for o in out], axis=1), np.stack([o[2] for o in out], axis=1), [o[3] for o in out]


def dense_log_a(band, log_tiny, log_cross):
    """The full [2B, 2B] log transition matrix from the band table (rows = predecessors j, columns = states i)."""
    B, W = band.shape
    ms = W // 2
    A = np.full((2 * B, 2 * B), log_tiny)
    i = np.arange(B)
    for d in range(W):
        j = i - ms + d
        ok = (j >= 0) & (j < B)
        A[j[ok], i[ok]] = band[ok, d]
        A[B + j[ok], B + i[ok]] = band[ok, d]
    A[i, i + B] = log_cross
    A[i + B, i] = log_cross
    return A


def viterbi_dense(logA, log_c, logO):
    """logO float64 [frames, 2B] -> path int64 [frames]: every predecessor evaluated, np.argmax (lowest index among equal rounded sums).
    Also returns the back pointers [frames, 2B]."""
    T, S = logO.shape
    D = log_c + logO[0]
    E = np.zeros((T, S), dtype=np.int64)
    for n in range(1, T):
        sums = logA + D[:, None]
        E[n] = np.argmax(sums, axis=0)
        D = np.max(sums, axis=0) + logO[n]
    path = np.zeros(T, dtype=np.int64)
    path[T - 1] = int(np.argmax(D))
    for n in range(T - 2, -1, -1):
        path[n] = E[n + 1][path[n + 1]]
    return path, E


def finish_ref(path, O, rms, lag_thr, val_thr, F_axis, Fs, R):
    """Step 9: (f0, conf) from the decoded path; O [2B, frames], lag_thr / val_thr [n_thr, frames]."""
    B, T = len(F_axis), len(path)
    f0 = np.concatenate((F_axis, np.zeros(B)))[path]
    f0[0] = 0
    f0[rms < 0.01] = 0
    conf = O[path, np.arange(T)] / np.max(O, axis=0)
    out = np.zeros(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        f_orig = Fs / lag_thr
        for m in np.flatnonzero(f0 > 0):
            near = np.flatnonzero(np.abs(1200 * np.log2(f_orig[:, m] / f0[m])) < R)
            if len(near) == 0:
                out[m] = f0[m]
                continue
            v = val_thr[near, m]
            nan_at = np.flatnonzero(np.isnan(v))
            out[m] = f_orig[near[nan_at[0] if len(nan_at) else int(np.argmin(v))], m]
    return out, conf


def pyin_ref(x, pl, R=10, amp=0.01, voicing_prob=0.5, cmndf_scale=None, o_scale=None):
    """The whole programme on a clip -> dict(path, f0, conf, rms, cmndf [frames, p_max + 1], O [2B, frames], lag_thr, val_thr).
    ``cmndf_scale`` [frames, p_max + 1] / ``o_scale`` [2B, frames] multiply the CMNDF / O elementwise (the golden script's perturbations)."""
    fr = frames_of(x, pl.N, pl.H)
    cm = np.stack([cmndf_f64(f, pl.p_max) for f in fr])
    if cmndf_scale is not None:
        cm = cm * cmndf_scale
    rms = np.sqrt(np.mean(fr ** 2, axis=1))
    O, lag_thr, val_thr, _ = observe_rows(cm, pl, amp, voicing_prob)
    if o_scale is not None:
        O = O * o_scale
    logA = dense_log_a(pl.band_np, pl.log_tiny, pl.log_cross)
    path, _ = viterbi_dense(logA, pl.log_c, np.ascontiguousarray(np.log(O + TINY).T))
    f0, conf = finish_ref(path, O, rms, lag_thr, val_thr, pl.F_axis, pl.Fs, R)
    return dict(path=path, f0=f0, conf=conf, rms=rms, cmndf=cm, O=O, lag_thr=lag_thr, val_thr=val_thr)


# ================================================================================================ 1. CMNDF and RMS
def tone_noise(n, seed=0, fs=16000):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (0.4 * np.sin(2 * np.pi * 196.0 * t) + 0.2 * np.sin(2 * np.pi * 392.0 * t + 0.7) + 0.03 * rng.standard_normal(n)).astype(np.float32)


def cmndf_oracle(x32, N, H, p_max):
    """np.longdouble: (cmndf [frames, p_max + 1], rms [frames])."""
    assert np.finfo(np.longdouble).nmant >= 63, "extended precision is needed for the oracle"
    fr = frames_of(x32, N, H).astype(np.longdouble)
    T = fr.shape[0]
    c = np.zeros((T, p_max + 1), dtype=np.longdouble)
    c[:, 0] = 1
    mean = np.zeros(T, dtype=np.longdouble)
    eps = np.longdouble(EPS)
    for tau in range(1, p_max + 1):
        d = ((fr[:, :N - tau] - fr[:, tau:]) ** 2).sum(axis=1)
        mean = mean * (tau - 1) / tau + d / tau
        c[:, tau] = d / (mean + eps)
    return c, np.sqrt((fr ** 2).mean(axis=1))


def cmndf_ratio(cm_dev, rms_dev, x32, N, H, p_max):
    want, rms = cmndf_oracle(x32, N, H, p_max)
    got, got_rms = cm_dev.cpu().numpy(), rms_dev.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape and got_rms.shape == rms.shape, (got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(got_rms).all() and bool((got[:, 0] == 1.0).all())
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    bound = CMNDF_C * (N + 2) * U * np.abs(want).astype(np.float64)
    assert bool((err[bound == 0] == 0).all())                           # an exact zero (a silent frame) must come out as one
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    rerr = np.abs(got_rms.astype(np.longdouble) - rms).astype(np.float64)
    rb = (N + 2) * U * rms.astype(np.float64)
    assert bool((rerr[rb == 0] == 0).all())
    rr = float((rerr[rb > 0] / rb[rb > 0]).max()) if (rb > 0).any() else 0.0
    return r, rr


def check_cmndf_frames(ops, device, T, small=False):
    """T frames against the longdouble oracle; returns (worst CMNDF error / bound, worst RMS error / bound)."""
    par = SMALL if small else P
    pl = plan(device, **par)
    x = tone_noise(par["H"] * (T - 1) + (0 if small else 17), seed=T)
    cm, rms = ops.pyin_cmndf(pl.struct, torch.from_numpy(x).to(device))
    sync(ops)
    assert tuple(cm.shape) == (T, pl.p_max + 1) and (not small or pl.p_max == par["N"])
    r, rr = cmndf_ratio(cm, rms, x, par["N"], par["H"], pl.p_max)
    print(f"pyin CMNDF {'N=64 ' if small else ''}{T} frames: worst error / bound {r:.3f}, rms {rr:.3f}")
    assert r <= 1.0 and rr <= 1.0, (r, rr)
    return r, rr


def check_cmndf_silence(ops, device):
    pl = plan(device)
    cm, rms = ops.pyin_cmndf(pl.struct, torch.zeros(5 * P["H"], dtype=torch.float32, device=device))
    sync(ops)
    assert bool((cm[:, 0] == 1).all()) and not bool(cm[:, 1:].any()) and not bool(torch.isnan(cm).any()) and not bool(rms.any())


def check_cmndf_bits(ops, device):
    """The bits of a frame depend on its N padded samples alone.  The same signal three ways: on its own; embedded between real zeros (the
    inner frames sit four blocks further on and see real zeros where the first run saw padding; the outermost frames lie wholly in zeros);
    and as an offset view into a wider buffer, on another stream on the GPU."""
    pl = plan(device)
    H = P["H"]
    s = tone_noise(H * 8 + 5, seed=11)
    base, base_rms = ops.pyin_cmndf(pl.struct, torch.from_numpy(s).to(device))
    emb = np.concatenate([np.zeros(4 * H, np.float32), s, np.zeros(4 * H - 5, np.float32)])
    wide, wide_rms = ops.pyin_cmndf(pl.struct, torch.from_numpy(emb).to(device))
    buf = torch.full((s.shape[0] + 64,), 3.0, dtype=torch.float32, device=device)
    buf[3:3 + s.shape[0]] = torch.from_numpy(s).to(device)
    view = buf[3:3 + s.shape[0]]
    assert view.data_ptr() % 16 != 0
    if ops.on_gpu:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            off, off_rms = ops.pyin_cmndf(pl.struct, view)
        torch.cuda.current_stream().wait_stream(side)
    else:
        off, off_rms = ops.pyin_cmndf(pl.struct, view)
    sync(ops)
    T = base.shape[0]
    assert T == 9 and wide.shape[0] == T + 8
    assert not bool(wide[0, 1:].any()) and not bool(wide[-1, 1:].any()) and bool(base[:, 1:].abs().max() > 0)
    assert torch.equal(wide[4:4 + T], base) and torch.equal(wide_rms[4:4 + T], base_rms)
    assert torch.equal(off, base) and torch.equal(off_rms, base_rms)


# ================================================================================================ 2. the observation kernel
def built_rows(pl, seed=0):
    """Seeded CMNDF rows [p_max + 1] built to hit each branch of the thresholding; returns (rows, the properties each must show)."""
    rng = np.random.default_rng(seed)
    n, p_min, p_max = pl.p_max + 1, pl.p_min, pl.p_max
    ramp = 1.5 + 0.002 * np.arange(n)
    rows, want = [], []

    def dips(base, count, lo):
        """``count`` strict interior minima at seeded, non-adjacent lags in lo .. p_max - 3."""
        pos = np.sort(rng.choice(np.arange(lo, p_max - 3, 3), size=count, replace=False))
        base[pos] = rng.uniform(0.02, 0.9, size=count)
        return base

    rows.append(np.full(n, 0.7)); want.append(dict(L=0))                                     # no minimum: a plateau
    rows.append(np.zeros(n)); want.append(dict(L=0))                                         # silence
    rows.append(ramp.copy()); want.append(dict(L=1, border_lo=True, border_hi=False))        # only the p_min minimum
    rows.append(ramp[::-1].copy()); want.append(dict(L=1, border_lo=False, border_hi=True, nan_val=True))      # only p_max - 1: c there is NaN
    peak = np.minimum(ramp, ramp[::-1]).copy()
    rows.append(peak); want.append(dict(L=2, border_lo=True, border_hi=True))                # both borders, nothing between
    # the deletion quirk with a minimum at p_min: L - 1 == p_min, so L = p_min + 1 minima, the last at p_max - 1
    q = dips(ramp.copy(), p_min + 1 - 2, p_min + 3)
    q[p_max - 1] = 0.3
    rows.append(q); want.append(dict(L=p_min + 1, quirk=True, border_lo=True, border_hi=True))
    # ... and without one: the first minimum at p_min + 1 == L - 1, its correction replaced by the SECOND minimum's
    q = dips(ramp.copy(), p_min + 2 - 2, p_min + 4)
    q[p_min] = 9.0
    q[p_max - 1] = 0.3
    rows.append(q); want.append(dict(L=p_min + 2, quirk=True, border_lo=False, border_hi=True))
    # ordinary rows: interior minima only, some thresholds fall back to the global minimum
    for k in range(3):
        q = dips(ramp.copy(), 6 + 5 * k, p_min + 3)
        q[p_min] = 9.0
        q[p_min + 1] = 8.0
        q[p_max - 1] = 7.0
        q[p_max - 2] = 6.0
        rows.append(q); want.append(dict(border_hi=False))
    return np.stack(rows), want


def observe_dev(ops, device, pl, rows):
    O, lag, val = ops.pyin_observe(pl.struct, torch.from_numpy(np.ascontiguousarray(rows)).to(device))
    sync(ops)
    return O.cpu().numpy().T, lag.cpu().numpy().T, val.cpu().numpy().T


def check_observe_rows(ops, device, rows, pl, want=None):
    Ow, lw, vw, infos = observe_rows(rows, pl)
    for k, w in enumerate(want or ()):
        for key, v in w.items():
            assert infos[k][key] == v, (k, key, infos[k])
    Od, ld, vd = observe_dev(ops, device, pl, rows)
    assert same_bits(ld, lw), np.argwhere(~((ld == lw) | (np.isnan(ld) & np.isnan(lw))))[:4]
    assert same_bits(vd, vw), np.argwhere(~((vd == vw) | (np.isnan(vd) & np.isnan(vw))))[:4]
    assert same_bits(Od, Ow), np.argwhere(Od != Ow)[:4]
    return infos


def check_observe_built(ops, device):
    """The built rows with 99 thresholds and with one; no input reaches a NaN lag (the code path exists in the reference, but a
    correction is NaN only at a border minimum whose CMNDF value is NaN too, and NaN is never below a threshold)."""
    pl = plan(device)
    rows, want = built_rows(pl)
    infos = check_observe_rows(ops, device, rows, pl, want)
    assert any(i["nan_val"] for i in infos) and any(i["fallback"] for i in infos) and not any(i["nan_lag"] for i in infos)
    one = plan(device, thresholds=np.array([0.1]))
    assert one.struct.n_thr == 1
    check_observe_rows(ops, device, rows, one)


def check_observe_golden(ops, device):
    """The stored CMNDF rows of the reference's own runs: O columns, lag_thr, val_thr equal to the stored ones bit for bit."""
    g, pl = golden(), plan(device)
    rows = np.concatenate([g[f"cmndf_{n}"] for n in CLIPS])
    infos = check_observe_rows(ops, device, rows, pl)
    Od, ld, vd = observe_dev(ops, device, pl, rows)
    assert same_bits(Od.T, np.concatenate([g[f"O_{n}"] for n in CLIPS]))
    assert same_bits(ld.T, np.concatenate([g[f"lag_thr_{n}"] for n in CLIPS])) and same_bits(vd.T, np.concatenate([g[f"val_thr_{n}"] for n in CLIPS]))
    return infos


# ================================================================================================ 3. Viterbi
@functools.lru_cache(maxsize=None)
def band_for(B, max_step=5):
    from svcmi.pitch.core import pyin as Y
    band = Y.transition_band(B, max_step)
    log_tiny, log_cross, log_c = float(np.log(TINY)), float(np.log(np.float64(1 - 0.99) + TINY)), float(np.log(np.float64(1.0) / (2 * B) + TINY))
    return band, log_tiny, log_cross, log_c, dense_log_a(band, log_tiny, log_cross)


def random_log_o(T, B, seed):
    """Columns like the real ones: a few voiced bins hold weight, the rest are exact zeros; the unvoiced half is one constant per frame."""
    rng = np.random.default_rng(seed)
    Ov = np.zeros((B, T))
    for t in range(T):
        k = rng.integers(0, 5)
        Ov[rng.integers(0, B, size=k), t] = rng.random(k) * 0.3
    return np.ascontiguousarray(np.log(normalise(Ov, 0.5) + TINY).T)


def viterbi_dev(ops, device, logO, B, max_step=5):
    band, log_tiny, log_cross, log_c, _ = band_for(B, max_step)
    out = ops.pyin_viterbi(torch.from_numpy(np.ascontiguousarray(logO)).to(device), torch.from_numpy(band).to(device), log_tiny, log_cross, log_c)
    sync(ops)
    return out.cpu().numpy().astype(np.int64)


def check_viterbi(ops, device, logO, B, max_step=5):
    _, _, _, log_c, logA = band_for(B, max_step)
    want, _ = viterbi_dense(logA, log_c, logO)
    got = viterbi_dev(ops, device, logO, B, max_step)
    assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[:8], want[:8])
    return got


def check_viterbi_random(ops, device, T, B=634):
    return check_viterbi(ops, device, random_log_o(T, B, 31 * T + B), B)


def check_viterbi_sizes(ops, device):
    """B = 11 (max_step 5: both edge regimes of the transition matrix overlap), the kernel's limit B = 1024, and the refusals."""
    for T, B in ((7, 11), (2, 11), (3, 1024)):
        check_viterbi_random(ops, device, T, B)
    band, log_tiny, log_cross, log_c, _ = band_for(11)
    z = torch.zeros(4 * 2 * 1025, dtype=torch.float64, device=device)
    ptr = torch.zeros(4 * 2 * 1025, dtype=torch.int16, device=device)
    path = torch.full((4,), -7, dtype=torch.int32, device=device)
    bd = torch.from_numpy(band).to(device)
    f = ops.lib.svcmi_pyin_viterbi_f64
    assert f(z.data_ptr(), 4, 1025, 5, bd.data_ptr(), log_tiny, log_cross, log_c, ptr.data_ptr(), path.data_ptr(), ops._stream()) == -2
    assert f(z.data_ptr(), 4, 64, 17, bd.data_ptr(), log_tiny, log_cross, log_c, ptr.data_ptr(), path.data_ptr(), ops._stream()) == -2
    assert f(z.data_ptr(), 1, 64, 5, bd.data_ptr(), log_tiny, log_cross, log_c, ptr.data_ptr(), path.data_ptr(), ops._stream()) == -1
    sync(ops)
    assert bool((path == -7).all())


def check_viterbi_ties(ops, device, B=634):
    """All-equal columns: every sum ties exactly, the lowest index wins at every step and at the end -- alone, and between random columns."""
    flat = np.full((5, 2 * B), np.log(TINY))
    assert not check_viterbi(ops, device, flat, B).any()
    mixed = random_log_o(12, B, 5)
    mixed[3:6] = -3.0
    mixed[11] = -1.0
    check_viterbi(ops, device, mixed, B)


def check_viterbi_rounding_tie(ops, device, B=634):
    """Two predecessors j1 < j2 with D[j1] < D[j2], a few ulps apart, collide after log_tiny (ulp 1.1e-13) is added: numpy's argmax over the
    ROUNDED sums takes j1 for every state that reaches both over an "impossible" transition; an arg-max of D itself would take j2."""
    _, log_tiny, _, log_c, logA = band_for(B)
    j1, j2, far = 10, 30, 500
    logO = np.full((3, 2 * B), -40.0)
    logO[0] = -5000.0                                                  # nothing but j1 and j2 is worth leaving at frame 0
    logO[0, j1] = -3.0
    logO[0, j2] = -3.0 + 8 * np.spacing(3.0)                           # two ulps of D (about -10.1) above j1
    logO[1:] = -5000.0                                                 # ... and only `far`, out of both bands, is worth reaching
    logO[1, far] = -1.0
    logO[2, far] = -1.0
    D0 = log_c + logO[0]
    assert D0[j1] < D0[j2] and log_tiny + D0[j1] == log_tiny + D0[j2]
    want, E = viterbi_dense(logA, log_c, logO)
    assert E[1][far] == j1 and list(want) == [j1, far, far], (E[1][far], want)
    assert np.array_equal(viterbi_dev(ops, device, logO, B), want)


def check_viterbi_impossible(ops, device, B=634):
    """Frames whose only weight sits far outside the band of the previous frame's: the path has to take a -708 transition."""
    log_tiny = float(np.log(TINY))
    logO = np.full((6, 2 * B), log_tiny)
    for t, s in enumerate((100, 300, 300, B + 20, 600, 5)):
        logO[t, s] = -0.5
    got = check_viterbi(ops, device, logO, B)
    assert list(got) == [100, 300, 300, B + 20, 600, 5], got


def check_viterbi_repeatable(ops, device, B=634):
    logO = random_log_o(33, B, 17)
    first = viterbi_dev(ops, device, logO, B)
    assert np.array_equal(first, viterbi_dev(ops, device, logO, B))
    if ops.on_gpu:
        band, log_tiny, log_cross, log_c, _ = band_for(B)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            again = ops.pyin_viterbi(torch.from_numpy(logO).to(device), torch.from_numpy(band).to(device), log_tiny, log_cross, log_c)
        side.synchronize()
        assert np.array_equal(first, again.cpu().numpy())


# ================================================================================================ 4. end to end
def check_end_to_end(ops, device, name):
    """clip -> path, voicing and conf equal to the golden ones in every frame, f0 within 8 f0sens + 4 u f0; rms inside its bound (twice:
    the golden rms is numpy's float64, not the oracle).  Returns (f0, conf)."""
    g, pl = golden(), plan(device)
    x = clip(name)
    out, path, parts = ops.pyin_f0_fwd(pl.struct, torch.from_numpy(x).to(device), want_parts=True)
    sync(ops)
    f0, conf = out.cpu().numpy()
    want_path, want_f0 = g[f"path_{name}"].astype(np.int64), g[f"f0_{name}"]
    assert f0.dtype == np.float64 and f0.shape == want_f0.shape == (1 + len(x) // P["H"],)
    assert np.array_equal(path.cpu().numpy().astype(np.int64), want_path)
    assert np.array_equal(f0 > 0, want_f0 > 0)
    assert same_bits(conf, g[f"conf_{name}"]), int((conf != g[f"conf_{name}"]).sum())
    tol = 8 * g[f"f0sens_{name}"] + 4 * U * want_f0
    assert bool((np.abs(f0 - want_f0) <= tol).all()), float((np.abs(f0 - want_f0) - tol).max())
    rms = parts["rms"].cpu().numpy()
    assert bool((np.abs(rms - g[f"rms_{name}"]) <= (P["N"] + 2) * U * 2 * g[f"rms_{name}"]).all())
    assert parts["O"].shape == (len(f0), 2 * pl.B) and parts["lag_thr"].shape == (len(f0), 99)
    return f0, conf


def check_pyin_api(ops, device, name="glide"):
    """``pyin`` returns (f0, t, conf) like the reference: float64, the stage's own values; and its two exceptions."""
    from svcmi.pitch.core.pyin import pyin
    f0, t, conf = pyin(clip(name), device=device, ops=ops, **P)
    want_f0, want_conf = check_end_to_end(ops, device, name)
    assert f0.dtype == conf.dtype == np.float64 and np.array_equal(f0, want_f0) and same_bits(conf, want_conf)
    assert np.array_equal(t, np.arange(len(f0)) * 320 / 16000)
    for bad in (dict(F_min=2000.0), dict(F_min=5.0)):
        try:
            pyin(clip(name), device=device, ops=ops, **{**P, **bad})
        except ValueError:
            raise AssertionError("the reference raises a plain Exception here")
        except Exception as e:          # noqa: BLE001
            assert "F_min" in str(e)
        else:
            raise AssertionError(f"{bad} did not raise")


def check_compute_f0_pyin(ops, device, name="035"):
    """The recipe: float64 [2 (1 + n // 320)], every frame twice, zeros where the golden track is unvoiced, no moving average."""
    from svcmi.pitch import compute_f0_pyin
    x = clip(name)
    track = compute_f0_pyin(x, device, ops=ops)
    want = golden()[f"f0_{name}"]
    assert track.dtype == np.float64 and track.shape == (2 * (1 + len(x) // 320),)
    assert np.array_equal(track[0::2], track[1::2]) and np.array_equal(track[0::2] == 0, want == 0) and 0 < int((want == 0).sum()) < len(want)
    assert bool((np.abs(track[0::2] - want) <= 8 * golden()[f"f0sens_{name}"] + 4 * U * want).all())
    return track


def check_edges(ops, device):
    """Silence is unvoiced throughout; 319 samples (one frame) raise ValueError; 320 give 2 frames; limits raise ValueError."""
    from svcmi.pitch import compute_f0_pyin
    from svcmi.pitch.core.pyin import pyin
    f0, _, conf = pyin(np.zeros(3200, np.float32), device=device, ops=ops, **P)
    assert f0.shape == (11,) and not f0.any() and np.isfinite(conf).all()
    try:
        compute_f0_pyin(np.zeros(319, np.float32), device, ops=ops)
    except ValueError:
        pass
    else:
        raise AssertionError("319 samples (one frame) did not raise ValueError")
    two = compute_f0_pyin(tone_noise(320, seed=2), device, ops=ops)
    assert two.shape == (4,) and np.isfinite(two).all()
    for bad in (dict(R=1), dict(thresholds=np.arange(0.001, 1, 0.005)), dict(N=8192), dict(N=2047), dict(R=60)):
        try:
            pyin(np.zeros(3200, np.float32), device=device, ops=ops, **{**P, **bad})
        except ValueError:
            pass
        else:
            raise AssertionError(f"{bad} did not raise ValueError")


# ================================================================================================ 5. the command line
CLI_ARGS = ["--config", "cfg.yaml", "--model", "svc.pth", "--wave", "in.wav", "--spk", "spk.npy", "--whisper", "whisper.pt",
            "--hubert", "hubert.pt", "--crepe", "no_such_dir/full.pth", "--f0", "pyin"]


def prepare_cli_files(tmp_path, monkeypatch):
    """The files svc_inference.main reads (tests/salience_cases.py makes them) in ``tmp_path``.  Returns the golden 035 track repeated
    twice: the command's svc_tmp.pit.csv is compared with it line by line, a voiced frame within the f0 tolerance of its integer part."""
    from tests import salience_cases as S
    S.prepare_cli_files(tmp_path, monkeypatch)
    return np.repeat(golden()["f0_035"], 2), np.repeat(8 * golden()["f0sens_035"] + 4 * U * golden()["f0_035"], 2)


def check_csv(path, want, tol):
    """svc_tmp.pit.csv against the golden track: int() of a value within the tolerance of the golden one; zeros exactly."""
    from svcmi.pitch.inference import load_csv_pitch
    got = np.array(load_csv_pitch(path), dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(got == 0, want == 0)
    assert bool(((got >= np.floor(want - tol)) & (got <= np.floor(want + tol))).all())
    return got
