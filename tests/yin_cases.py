"""Checks of the YIN F0 extractor (csrc/yin.hip, svcmi.pitch.core.yin, svcmi.pitch.compute_f0_yin), shared by the emulator tests (CPU) and
the GPU tests: every function takes ``ops`` and ``device``.

The target is the reference's pitch/core/yin.py AS IT EXECUTES under numpy with ``numba.njit`` as the identity.  Its steps are restated here
as a float64 numpy programme (``threshold_row``, ``pick_row``, ``aperiodicity_f64``, composed in ``yin_ref``); tests/test_yin_emu.py and
scripts/make_yin_golden.py prove the programme equal to the reference bit for bit where the reference exists.

Oracles and bounds (u = 2^-53, N the frame length):
  * CMNDF: the rows hold the bits of ``pyin_cmndf`` at p_max = lag_max (it is the same kernel).  A single frame, which pYIN's entry point
    refuses, is compared with the float64 programme inside pYIN's relative bound 5 (N + 2) u (tests/pyin_cases.py derives it).
  * the two thresholdings from given rows: equal to ``pick_row`` bit for bit -- both lags, the kind bits.
  * aperiodicity from a given lag: an ``np.longdouble`` oracle with a first-order bound (``ap_oracle``).  The samples are fp32, so f^2 and, for
    a lag without fractional part, s^2 are exact in fp64; f - s rounds once (u), its square once more (3 u in all).  A sum of N
    non-negative terms in any order adds (N - 1) u, the division by N one more: mean f^2 carries N u, mean (f - s)^2 carries (N + 3) u.  With a
    fractional lag s = fl(fl(1 - frac) a) + fl(frac b) is off by at most 3 u M, M = (1 - frac) |a| + frac |b| (the two products carry 2 u and
    u, the sum u of |s| <= M) -- an ABSOLUTE error, a and b may cancel --, which adds 6 u mean(|s| M) + u mean s^2 to mean s^2 and
    6 u mean(|f - s| M) to mean (f - s)^2.  pwr + eps takes two more roundings, the quotient one:
        |ap_dev - ap| <= (d_res + ap d_pwr) / (pwr + eps) + u ap,
        d_res = ((N + 3) u R + 6 u mean(|f - s| M)) / 2,   d_pwr = (N u S1 + (N + 1) u S2 + 6 u mean(|s| M)) / 2 + 2 u (pwr + eps).
    Nothing in it is fitted to the device.  All three sums zero (silence) must give exactly 0.
  * end to end on the golden clips: the integer parts of both lags and the kind bits equal in every frame, |f0 - f0_golden| <= 8 f0sens +
    4 u f0_golden, |ap - ap_golden| <= 8 apsens + the bound above (f0sens, apsens: how far the reference's own f0 and ap move when its
    CMNDF is perturbed by the CMNDF kernel's bound DELTA; scripts/make_yin_golden.py).
"""
import functools
import os

import numpy as np
import torch

from tests import pyin_cases as PC

U = PC.U
EPS = PC.EPS
DELTA = PC.DELTA
GOLDEN = PC.GOLDEN
P = dict(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, threshold=0.15)      # compute_f0_yin's parameters
SMALL = dict(Fs=16000, N=64, H=16, F_min=250.0, F_max=4000.0, threshold=0.15)      # lag_max = N
AP_THRESHOLD = 0.2                                                                  # the voicing threshold the recipe tests use
CLIPS = PC.CLIPS
ROWS = (0, 1, 50, 100)                                                              # the frames whose CMNDF rows the golden file keeps
R_UP, R_DOWN = 2 ** (25 / 1200), 2 ** (-25 / 1200)
clip = PC.clip
same_bits = PC.same_bits
sync = PC.sync
tone_noise = PC.tone_noise
frames_of = PC.frames_of


@functools.lru_cache(maxsize=1)
def golden():
    with np.load(os.path.join(GOLDEN, "yin_f0.npz")) as z:
        return {k: z[k] for k in z.files}


def plan(**over):
    from svcmi.pitch.core import yin as Y
    return Y.yin_plan(**{**P, **over})


def is_int(v):
    return isinstance(v, (int, np.integer))


# ================================================================================================ the float64 programme
def threshold_row(c, thr, lo, hi):
    """One ``absolute_thresholding`` over [lo, hi) on the row ``c`` (modified in place) -> (lag, how): how = "short" (lo == hi: lo, an
    int), "min" (the first strict local minimum below thr, interpolated: a float; c[lag] takes the parabola's value) or "arg" (np.argmin
    of c[lo:hi] + lo, an int)."""
    if lo == hi:
        return lo, "short"
    i = np.arange(lo, hi)
    hits = i[(c[i] < c[i - 1]) & (c[i] < c[i + 1]) & (c[i] < thr)]
    if not len(hits):
        return int(np.argmin(c[lo:hi])) + lo, "arg"
    lag = int(hits[0])
    y1, y2, y3 = c[lag - 1], c[lag], c[lag + 1]
    a = EPS + (y1 + y3 - 2 * y2) / 2
    b = (y3 - y1) / 2
    c[lag] = y2 - (b * b) / (4 * a)
    return lag + -b / (2 * a), "min"


def pick_row(c, threshold, lag_min, lag_max, Fs):
    """Steps 3 and 4 for one CMNDF row -> (lag_new, lag_first, kind); the lags keep their types (int or float)."""
    c = np.array(c, dtype=np.float64)
    first, how1 = threshold_row(c, threshold, lag_min, lag_max)
    lo = max(int(np.round(Fs / ((Fs / first) * R_UP))), lag_min)
    hi = min(int(np.round(Fs / ((Fs / first) * R_DOWN))), lag_max)
    new, how2 = threshold_row(c, np.inf, lo, hi)
    return new, first, (1 if how1 == "arg" else 0) | (2 if how2 == "short" else 0) | (4 if how2 == "arg" else 0)


def aperiodicity_f64(frame, lag):
    """Step 6 in float64 with numpy's own summation order (what the reference computes)."""
    n = len(frame)
    li = int(np.floor(lag))
    frac = lag - li
    g = np.concatenate((frame, frame[::-1]))
    s = g[li:li + n] if frac == 0 else (1 - frac) * g[li:li + n] + frac * g[li + 1:li + 1 + n]
    pwr = (np.mean(frame ** 2) + np.mean(s ** 2)) / 2
    res = np.mean((frame - s) ** 2) / 2
    return res / (pwr + EPS)


def yin_ref(x, par=None, cmndf=None, cmndf_scale=None):
    """The whole programme on a clip -> dict(f0, ap, lag, lag_first float64 [frames], kind, lag_int, first_int (whether each lag came out
    as an integer) and cmndf [frames, lag_max + 1]).  ``cmndf``: rows computed earlier; ``cmndf_scale`` multiplies them elementwise."""
    par = par or P
    Fs, N, H = par["Fs"], par["N"], par["H"]
    lag_min, lag_max = max(int(np.ceil(Fs / par["F_max"])), 1), int(np.ceil(Fs / par["F_min"]))
    fr = frames_of(x, N, H)
    cm = np.stack([PC.cmndf_f64(f, lag_max) for f in fr]) if cmndf is None else cmndf
    rows = cm if cmndf_scale is None else cm * cmndf_scale
    T = len(fr)
    out = dict(f0=np.zeros(T), ap=np.zeros(T), lag=np.zeros(T), lag_first=np.zeros(T), kind=np.zeros(T, np.int32), lag_int=np.zeros(T, bool),
               first_int=np.zeros(T, bool), cmndf=cm)
    for m in range(T):
        new, first, kind = pick_row(rows[m], par["threshold"], lag_min, lag_max, Fs)
        out["lag"][m], out["lag_first"][m], out["kind"][m], out["lag_int"][m], out["first_int"][m] = new, first, kind, is_int(new), is_int(first)
        out["f0"][m] = Fs / new
        out["ap"][m] = aperiodicity_f64(fr[m], new)
    return out


# ================================================================================================ 1. CMNDF
def check_cmndf_equals_pyin(ops, device, T, small=False):
    """T frames: the rows of ``yin_cmndf`` hold the bits of ``pyin_cmndf`` for the same clip, n_fft, hop and p_max = lag_max."""
    par = SMALL if small else P
    pl = plan(**par)
    ppl = PC.plan(device, **{k: v for k, v in par.items() if k != "threshold"})
    assert (ppl.p_min, ppl.p_max) == (pl.lag_min, pl.lag_max) and (not small or pl.lag_max == par["N"])
    x = torch.from_numpy(tone_noise(par["H"] * (T - 1) + (5 if small else 17), seed=40 + T)).to(device)
    mine = ops.yin_cmndf(pl.struct, x)
    theirs, _ = ops.pyin_cmndf(ppl.struct, x)
    sync(ops)
    assert tuple(mine.shape) == (T, pl.lag_max + 1) and mine.dtype == torch.float64
    assert torch.equal(mine.view(torch.int64), theirs.view(torch.int64)) and bool(mine[:, 1:].abs().max() > 0)


def check_cmndf_one_frame(ops, device):
    """n = 1 and n = hop - 1: one frame, which pYIN's entry point refuses, against the float64 programme inside pYIN's bound."""
    pl = plan()
    for n in (1, P["H"] - 1):
        x = tone_noise(n, seed=n) + np.float32(0.25)
        cm = ops.yin_cmndf(pl.struct, torch.from_numpy(x).to(device))
        sync(ops)
        want = PC.cmndf_f64(frames_of(x, P["N"], P["H"])[0], pl.lag_max)
        got = cm.cpu().numpy()
        assert got.shape == (1, pl.lag_max + 1) and got[0, 0] == 1.0 and bool(want[1:].max() > 0)
        err, bound = np.abs(got[0] - want), PC.CMNDF_C * (P["N"] + 2) * U * np.abs(want)
        print(f"yin CMNDF one frame, n = {n}: worst error / bound {float((err[bound > 0] / bound[bound > 0]).max()):.2e}")
        assert bool((err <= bound).all()), float((err - bound).max())


# ================================================================================================ 2. the two thresholdings
def built_rows(pl):
    """CMNDF rows [lag_max + 1] built to hit each rule of the thresholding; returns (rows, per row the (floor(lag_first), floor(lag), kind)
    the programme must show, None where the row is only compared)."""
    n, lo, hi, thr = pl.lag_max + 1, pl.lag_min, pl.lag_max, pl.threshold
    assert (lo, hi, thr) == (10, 356, 0.15)
    base = np.ones(n)                                         # flat: every minimum below is put there by hand
    rows, want = [], []

    def row(**at):
        c = base.copy()
        for k, v in at.items():
            c[int(k[1:])] = v
        return c
    # no minimum below the threshold; the arg-min ties exactly between 50 and 200: the lowest index wins
    rows.append(row(i50=0.5, i200=0.5)); want.append((50, 50, 1))
    # no strict minimum at all (a flat row): np.argmin of equal values is the first index, then a collapsed window
    rows.append(base.copy()); want.append((10, 10, 1 | 2))
    # the first qualifying minimum is not the deepest; asymmetric neighbours: the write-back changes the second interpolation
    rows.append(row(i79=0.7, i80=0.1, i81=0.6, i160=0.01)); want.append((80, 80, 0))
    # a plateau is no strict minimum: 60 and 61 are skipped
    rows.append(row(i60=0.05, i61=0.05, i119=0.9, i120=0.1, i121=0.8)); want.append((120, 120, 0))
    # a value exactly equal to the threshold does not qualify
    rows.append(row(i70=thr, i139=0.9, i140=np.nextafter(thr, 0), i141=0.7)); want.append((140, 140, 0))
    # ... and is what the arg-min branch returns when nothing else is lower
    rows.append(row(i70=thr)); want.append((70, 70, 1))
    # a minimum at lag_min: the refinement window collapses (round(10 / 1.0145) = round(10 x 1.0145) = 10), an integer result
    rows.append(row(i10=0.05, i11=0.4)); want.append((10, 10, 2))
    # a small lag a little further on: still collapsed
    rows.append(row(i20=0.3, i21=0.05, i22=0.5)); want.append((20, 21, 2))
    # a minimum at lag_max - 1: the window is clipped to lag_max
    rows.append(row(i354=0.5, i355=0.05, i356=0.9)); want.append((354, 354, 0))
    # the refinement window [296, 304) holds an earlier (shallow, above the threshold) minimum than the first search's 300
    rows.append(row(i297=0.9, i299=0.3, i300=0.05, i301=0.4)); want.append((299, 297, 0))
    # both searches take the arg-min branch: the lowest value is a plateau, which the window [99, 101) holds without a strict minimum
    rows.append(row(i100=0.5, i101=0.5)); want.append((100, 100, 1 | 4))
    # the parabola moves the first minimum from 30 to 29.51: the window [29, 30) no longer holds it -> arg-min, the integer 29
    rows.append(row(i29=0.06, i30=0.05)); want.append((29, 29, 4))
    rng = np.random.default_rng(5)
    for k in range(24):                                       # seeded rows like real ones: a smooth curve with a few dips, some below the threshold
        t = np.arange(n)
        c = 1.0 + 0.5 * np.cos(2 * np.pi * t / rng.uniform(20, 180) + rng.uniform(0, 6)) * rng.uniform(0.2, 1.9) + 0.05 * rng.standard_normal(n)
        c = np.abs(c) * (1.0 if k % 3 else 0.3)
        c[0] = 1.0
        rows.append(c); want.append(None)
    return np.stack(rows), want


def pick_dev(ops, device, pl, rows):
    keep = torch.from_numpy(np.ascontiguousarray(rows)).to(device)
    before = keep.clone()
    out, first, kind = ops.yin_pick(pl.struct, keep, want_parts=True)
    sync(ops)
    assert torch.equal(keep, before), "the rows must not be modified"
    out = out.cpu().numpy()
    return out[0], out[1], first.cpu().numpy(), kind.cpu().numpy()


def check_pick_rows(ops, device, rows, pl, want=None):
    """The device against ``pick_row``: lag, lag_first and f0 bit for bit, kind equal.  Returns the programme's results."""
    ref = [pick_row(r, pl.threshold, pl.lag_min, pl.lag_max, pl.Fs) for r in rows]
    for k, w in enumerate(want or ()):
        if w is not None:
            assert (int(np.floor(ref[k][1])), int(np.floor(ref[k][0])), ref[k][2]) == w, (k, ref[k], w)
    for new, first, kind in ref:                             # the types follow the kind bits
        assert is_int(first) == bool(kind & 1) or pl.lag_min == pl.lag_max
        assert is_int(new) == bool(kind & 6)
    lag, f0, first, kind = pick_dev(ops, device, pl, rows)
    wl, wf, wk = (np.array([float(r[i]) for r in ref]) for i in range(3))
    assert same_bits(lag, wl), (np.flatnonzero(lag != wl)[:4], lag[lag != wl][:4], wl[lag != wl][:4])
    assert same_bits(first, wf), np.flatnonzero(first != wf)[:4]
    assert np.array_equal(kind, wk.astype(np.int32)), np.flatnonzero(kind != wk)[:4]
    assert same_bits(f0, pl.Fs / wl)
    return ref


def check_pick_built(ops, device):
    pl = plan()
    rows, want = built_rows(pl)
    ref = check_pick_rows(ops, device, rows, pl, want)
    kinds = {r[2] for r in ref}
    assert {0, 1, 2, 3}.issubset(kinds) and any(k & 4 for k in kinds), kinds
    # the write-back changes the second interpolation: with the same minimum chosen twice the two offsets differ
    new, first, kind = ref[2]
    assert kind == 0 and int(first) == int(new) == 80 and new != first
    # an earlier minimum inside the window
    assert int(ref[9][0]) < int(ref[9][1])
    # another threshold: +inf takes every first minimum, 0 takes none
    check_pick_rows(ops, device, rows, plan(threshold=float("inf")))
    assert all(r[2] & 1 for r in check_pick_rows(ops, device, rows, plan(threshold=0.0)))


def check_pick_single_lag(ops, device):
    """lag_min == lag_max: both searches return at once, integers."""
    pl = plan(F_min=100.0, F_max=100.0)
    assert pl.lag_min == pl.lag_max == 160
    rng = np.random.default_rng(3)
    rows = np.abs(rng.standard_normal((3, 161))) + 0.01
    ref = check_pick_rows(ops, device, rows, pl)
    assert all(r == (160, 160, 2) for r in ref)


def check_pick_golden(ops, device):
    """The stored CMNDF rows of the reference's own runs: both lags and the kind bits equal to the stored ones."""
    g, pl = golden(), plan()
    rows = np.concatenate([g[f"cmndf_{n}"] for n in CLIPS])
    idx = np.array(ROWS)
    check_pick_rows(ops, device, rows, pl)
    lag, f0, first, kind = pick_dev(ops, device, pl, rows)
    assert same_bits(lag, np.concatenate([g[f"lag_{n}"][idx] for n in CLIPS])) and same_bits(first, np.concatenate([g[f"lag_first_{n}"][idx] for n in CLIPS]))
    assert np.array_equal(kind, np.concatenate([g[f"kind_{n}"][idx] for n in CLIPS])) and same_bits(f0, np.concatenate([g[f"f0_{n}"][idx] for n in CLIPS]))


# ================================================================================================ 3. aperiodicity
def ap_oracle(frame, lag):
    """np.longdouble: (ap, the first-order bound of the module docstring) for one float64 frame of fp32 values and one float64 lag."""
    assert np.finfo(np.longdouble).nmant >= 63, "extended precision is needed for the oracle"
    n = len(frame)
    f = frame.astype(np.longdouble)
    li = int(np.floor(lag))
    frac = np.longdouble(lag) - li
    g = np.concatenate((f, f[::-1]))
    if frac == 0:
        s, M = g[li:li + n], np.zeros(n, np.longdouble)
    else:
        a, b = g[li:li + n], g[li + 1:li + 1 + n]
        s, M = (1 - frac) * a + frac * b, (1 - frac) * np.abs(a) + frac * np.abs(b)
    d = f - s
    S1, S2, R = (f * f).mean(), (s * s).mean(), (d * d).mean()
    pwr = (S1 + S2) / 2 + np.longdouble(EPS)
    ap = (R / 2) / pwr
    d_res = ((n + 3) * U * R + 6 * U * (np.abs(d) * M).mean()) / 2
    d_pwr = (n * U * S1 + (n + 1) * U * S2 + 6 * U * (np.abs(s) * M).mean()) / 2 + 2 * U * pwr
    return float(ap), float((d_res + ap * d_pwr) / pwr + U * ap)


def ap_ratio(got, x32, lags, N, H):
    """Worst |device - oracle| / bound over the frames; an exact zero must come out as one."""
    fr = frames_of(x32, N, H)
    assert got.shape == (len(fr),) == lags.shape and got.dtype == np.float64 and np.isfinite(got).all()
    worst = 0.0
    for m in range(len(fr)):
        want, bound = ap_oracle(fr[m], lags[m])
        err = abs(got[m] - want)
        if bound == 0:
            assert err == 0 and got[m] == 0, (m, got[m])
        else:
            worst = max(worst, err / bound)
    return worst


def check_ap_lags(ops, device, small=False):
    """Integer lags (the path without a product), fractional lags, the smallest and the largest lag -- at lag_max = N the shifted frame is the
    mirror image alone."""
    par = SMALL if small else P
    pl = plan(**par)
    N, H, hi = par["N"], par["H"], pl.lag_max
    lags = np.array([float(pl.lag_min), float(hi), hi - 0.5, hi - 1 + 2.0 ** -20, 37.0, 37.25, 36.999999999, float(hi // 2), hi / 3.0, 1.0, 0.5, 0.0,
                     np.nextafter(float(hi), 0)])
    x = tone_noise(H * (len(lags) - 1) + 3, seed=77)
    ap = ops.yin_aperiodicity(pl.struct, torch.from_numpy(x).to(device), torch.from_numpy(lags).to(device))
    sync(ops)
    r = ap_ratio(ap.cpu().numpy(), x, lags, N, H)
    print(f"yin aperiodicity {'N=64 ' if small else ''}{len(lags)} lags: worst error / bound {r:.2e}")
    assert r <= 1.0, r
    assert ap[11].item() == 0.0                              # lag 0: the frame against itself
    return r


def check_ap_silence(ops, device):
    pl = plan()
    lags = np.array([82.0, 81.37, 356.0, 10.5, 200.0, 0.25])
    ap = ops.yin_aperiodicity(pl.struct, torch.zeros(5 * P["H"], dtype=torch.float32, device=device), torch.from_numpy(lags).to(device))
    sync(ops)
    got = ap.cpu().numpy()
    assert got.shape == (6,) and not got.any() and not np.signbit(got).any()


def check_ap_short_clips(ops, device):
    """n = 1, H - 1, H, H + 1: one or two frames, most of every frame is padding."""
    pl = plan()
    H = P["H"]
    worst = 0.0
    for n in (1, H - 1, H, H + 1):
        x = tone_noise(n, seed=n) + np.float32(0.125)
        lags = np.array([100.0, 57.3])[:1 + n // H]
        ap = ops.yin_aperiodicity(pl.struct, torch.from_numpy(x).to(device), torch.from_numpy(lags).to(device))
        sync(ops)
        worst = max(worst, ap_ratio(ap.cpu().numpy(), x, lags, P["N"], H))
    print(f"yin aperiodicity short clips: worst error / bound {worst:.2e}")
    assert worst <= 1.0, worst


def check_ap_bits(ops, device):
    """The bits of a frame's ap depend on its N padded samples and its lag alone: the same signal on its own, embedded between real zeros
    (more frames in the launch, the frames four blocks further on), and as an offset view on another stream on the GPU."""
    pl = plan()
    H = P["H"]
    s = tone_noise(H * 8 + 5, seed=11)
    lags = np.array([82.0, 81.37, 40.0, 300.5, 356.0, 10.0, 123.456, 99.0, 250.75])
    lt = torch.from_numpy(lags).to(device)
    base = ops.yin_aperiodicity(pl.struct, torch.from_numpy(s).to(device), lt)
    emb = np.concatenate([np.zeros(4 * H, np.float32), s, np.zeros(4 * H - 5, np.float32)])
    wl = torch.from_numpy(np.concatenate([np.full(4, 50.0), lags, np.full(4, 50.5)])).to(device)
    wide = ops.yin_aperiodicity(pl.struct, torch.from_numpy(emb).to(device), wl)
    buf = torch.full((s.shape[0] + 64,), 3.0, dtype=torch.float32, device=device)
    buf[3:3 + s.shape[0]] = torch.from_numpy(s).to(device)
    view = buf[3:3 + s.shape[0]]
    assert view.data_ptr() % 16 != 0
    if ops.on_gpu:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            off = ops.yin_aperiodicity(pl.struct, view, lt)
        torch.cuda.current_stream().wait_stream(side)
    else:
        off = ops.yin_aperiodicity(pl.struct, view, lt)
    sync(ops)
    assert base.shape[0] == 9 and wide.shape[0] == 17 and bool((base > 0).all())
    assert wide[0].item() == 0.0 and wide[-1].item() == 0.0
    assert torch.equal(wide[4:13], base) and torch.equal(off, base)


# ================================================================================================ 4. the stage and the drop-ins
def ap_bounds(x32, lags, N, H):
    fr = frames_of(x32, N, H)
    return np.array([ap_oracle(fr[m], lags[m])[1] for m in range(len(fr))])


def check_end_to_end(ops, device, name):
    """clip -> the integer parts of both lags and the kind bits equal to the golden ones in every frame, f0 within 8 f0sens + 4 u f0, ap
    within 8 apsens + the kernel's bound.  Returns (f0, ap)."""
    g, pl = golden(), plan()
    x = clip(name)
    out, parts = ops.yin_f0_fwd(pl.struct, torch.from_numpy(x).to(device), want_parts=True)
    sync(ops)
    f0, ap = out.cpu().numpy()
    lag, first, kind = parts["lag"].cpu().numpy(), parts["lag_first"].cpu().numpy(), parts["kind"].cpu().numpy()
    want_f0, want_ap, want_lag = g[f"f0_{name}"], g[f"ap_{name}"], g[f"lag_{name}"]
    assert f0.dtype == ap.dtype == np.float64 and f0.shape == ap.shape == want_f0.shape == (1 + len(x) // P["H"],)
    assert np.array_equal(np.floor(lag), np.floor(want_lag)) and np.array_equal(np.floor(first), np.floor(g[f"lag_first_{name}"]))
    assert np.array_equal(kind, g[f"kind_{name}"]) and same_bits(f0, P["Fs"] / lag)
    tol = 8 * g[f"f0sens_{name}"] + 4 * U * want_f0
    assert bool((np.abs(f0 - want_f0) <= tol).all()), float((np.abs(f0 - want_f0) - tol).max())
    atol = 8 * g[f"apsens_{name}"] + ap_bounds(x, want_lag, P["N"], P["H"])
    print(f"yin {name}: worst |f0 - golden| / tolerance {float((np.abs(f0 - want_f0) / tol).max()):.3f}, "
          f"ap {float((np.abs(ap - want_ap)[atol > 0] / atol[atol > 0]).max()):.3f}")
    assert bool((np.abs(ap - want_ap) <= atol).all()), float((np.abs(ap - want_ap) - atol).max())
    return f0, ap


def check_yin_api(ops, device, name="glide"):
    """``yin`` returns (f0, t, ap) like the reference: float64, the stage's own values, the reference's time axis; and its two exceptions
    with its texts."""
    from svcmi.pitch.core.yin import yin
    f0, t, ap = yin(clip(name), device=device, ops=ops, **P)
    want_f0, want_ap = check_end_to_end(ops, device, name)
    assert f0.dtype == ap.dtype == t.dtype == np.float64 and np.array_equal(f0, want_f0) and np.array_equal(ap, want_ap)
    assert f0.shape == t.shape == ap.shape and np.array_equal(t, np.arange(len(f0)) * 320 / 16000)
    texts = {"F_min must be smaller than F_max!": dict(F_min=2000.0),
             "The condition (F_min >= Fs/N) was not met. With Fs = 16000, N = 2048 and F_min = 5.0 you have the following options: \n"
             "1) Set F_min >= 8.0 Hz. \n2) Set N >= 3200. \n3) Set Fs <= 10240.0 Hz.": dict(F_min=5.0)}
    for text, bad in texts.items():
        try:
            yin(clip(name), device=device, ops=ops, **{**P, **bad})
        except ValueError:
            raise AssertionError("the reference raises a plain Exception here")
        except Exception as e:          # noqa: BLE001
            assert str(e) == text, str(e)
        else:
            raise AssertionError(f"{bad} did not raise")


def check_compute_f0_yin(ops, device, name="035"):
    """The recipe: float64 [2 (1 + n // 320)], every frame twice, no moving average; with ap_threshold = 0.2 zeros exactly where the golden
    ap is above it, with None no zero at all."""
    from svcmi.pitch import compute_f0_yin
    g, x = golden(), clip(name)
    want, tol = g[f"f0_{name}"], 8 * g[f"f0sens_{name}"] + 4 * U * g[f"f0_{name}"]
    unvoiced = g[f"ap_{name}"] > AP_THRESHOLD
    assert np.abs(g[f"ap_{name}"] - AP_THRESHOLD).min() > 1e-6 and 0 < int(unvoiced.sum()) < len(want)
    track = compute_f0_yin(x, device, ops=ops)
    assert track.dtype == np.float64 and track.shape == (2 * (1 + len(x) // 320),)
    assert np.array_equal(track[0::2], track[1::2]) and bool((track > 0).all()) and bool((np.abs(track[0::2] - want) <= tol).all())
    gated = compute_f0_yin(x, device, ap_threshold=AP_THRESHOLD, ops=ops)
    assert gated.shape == track.shape and np.array_equal(gated[0::2], gated[1::2]) and np.array_equal(gated[0::2] == 0, unvoiced)
    assert np.array_equal(gated[0::2][~unvoiced], track[0::2][~unvoiced])
    return track, gated


def check_edges(ops, device):
    """Silence has an f0 in every frame and ap = 0; one sample gives one frame; an empty signal and parameters beyond the kernels' limits
    raise ValueError."""
    from svcmi.pitch import compute_f0_yin
    from svcmi.pitch.core.yin import yin
    f0, _, ap = yin(np.zeros(3200, np.float32), device=device, ops=ops, **P)
    assert f0.shape == (11,) and bool((f0 == 16000 / 10).all()) and not ap.any()      # a flat row of zeros: np.argmin gives lag_min
    one = compute_f0_yin(tone_noise(1, seed=2) + np.float32(0.5), device, ops=ops)
    assert one.shape == (2,) and np.isfinite(one).all() and one[0] == one[1] > 0
    two = compute_f0_yin(tone_noise(320, seed=2), device, ops=ops)
    assert two.shape == (4,) and np.isfinite(two).all()
    for bad in (dict(N=8192), dict(N=2047), dict(H=0)):
        try:
            yin(np.zeros(3200, np.float32), device=device, ops=ops, **{**P, **bad})
        except ValueError:
            pass
        else:
            raise AssertionError(f"{bad} did not raise ValueError")
    try:
        yin(np.zeros(0, np.float32), device=device, ops=ops, **P)
    except ValueError:
        pass
    else:
        raise AssertionError("an empty signal did not raise ValueError")
