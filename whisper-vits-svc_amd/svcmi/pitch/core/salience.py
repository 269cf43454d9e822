"""Drop-in for the reference's pitch/core/salience.py ``salience`` (libf0's Melodia-style F0 estimator): a salience map from
instantaneous frequencies and harmonic summation, then ONE dynamic-programming trajectory over the clip -- on the kernels of
csrc/salience.hip.

    f0, t, sal = salience(audio, Fs=16000, H=320, N=2048, F_min=45.0, F_max=1760.0)      # float64 [1 + n // H] each

The host makes the plan once per parameter set and device (``salience_plan``): the windowed DFT table in float64 restricted to the STFT bins
whose instantaneous frequency can fall into [F_min, F_max), the smoothing taps, the harmonic weights as a sparse list, the transition
constants.  Everything per clip runs on the device (``salience_begin``: enqueued, nothing waits); the host tail is a table lookup.

Differences from the reference, on purpose: ``constraint_region`` other than None raises ValueError (not implemented), and fewer than two
frames raise ValueError where the reference fails with IndexError.  ``gamma`` other than 0 thresholds at 10^(gamma / 20) of the maximum.
"""
import threading

import numpy as np
import torch

from ..._lib import SALIENCE_MAX_BINS, SaliencePlan
from ...ops import Ops

EPS32 = float(np.finfo(np.float32).eps)
HARMONIC_WIN_LEN = 11
_PLANS = {}
_OPS = None
_LOCK = threading.Lock()


def _default_ops():
    global _OPS
    with _LOCK:
        if _OPS is None:
            _OPS = Ops()
        return _OPS


def frequency_to_bin_index(F, R, F_ref):
    """pitch/core/salience.py:418-441."""
    return np.floor((1200 / R) * np.log2(F / F_ref) + 0.5).astype(np.int64)


def stft_bin_range(Fs, N, H, F_min, F_max):
    """(k_lo, k_hi) inclusive: the STFT bins that can contribute.  The wrapped phase increment is at most half a turn, so the instantaneous
    frequency of bin k lies within Fs / (2 H) of its centre k Fs / N; one more bin on each side covers the rounding of a half-turn."""
    reach = Fs / (2.0 * H)
    k_lo = int(np.ceil((F_min - reach) * N / Fs)) - 1
    k_hi = int(np.floor((F_max + reach) * N / Fs)) + 1
    return max(k_lo, 0), min(k_hi, N // 2)


def harmonic_weights(B, R, num_harm, alpha, harmonic_win_len=HARMONIC_WIN_LEN):
    """The weighting vector of pitch/core/salience.py:250-266 as (offsets, weights): z[b] = sum_m weights[m] lf[b + offsets[m]], m
    ascending -- scipy's correlate1d with that vector and origin, zeros skipped."""
    max_diff = harmonic_win_len // 2
    window = np.cos(np.linspace(-1, 1, 2 * max_diff + 1) * np.pi / 2) ** 2
    harmonics = np.round(np.log2(np.arange(1, num_harm + 1)) * 1200 / R).astype(int)
    vec = np.zeros(B + max_diff)
    for idx, h in enumerate(harmonics):
        if h + harmonic_win_len > len(vec):
            break
        vec[h:h + harmonic_win_len] += window * alpha ** idx
    origin = -len(vec) // 2 + max_diff
    shift = -(len(vec) // 2) - origin
    nz = np.nonzero(vec)[0]
    return (nz + shift).astype(np.int32), vec[nz]


class Plan:
    """One parameter set on one device: the filled ``struct`` (svcmi_salience_plan), the tensors it points to, the float64 frequency axis."""

    def __init__(self, Fs, N, H, F_min, F_max, R, num_harm, freq_smooth_len, alpha, gamma, tol, score_low, score_high, device):
        if N < 2 or N % 2 or H < 1 or not (0 < F_min < F_max) or R <= 0 or num_harm < 1 or alpha <= 0 or tol < 0:
            raise ValueError(f"salience: unsupported parameters N={N} H={H} F_min={F_min} F_max={F_max} R={R} num_harm={num_harm} alpha={alpha} tol={tol}")
        if freq_smooth_len < 1 or freq_smooth_len % 2 == 0 or freq_smooth_len > 65:
            raise ValueError(f"salience: freq_smooth_len {freq_smooth_len} must be odd and at most 65")
        B = int(frequency_to_bin_index(np.float64(F_max), R, F_min)) + 1
        k_lo, k_hi = stft_bin_range(Fs, N, H, F_min, F_max)
        n_bins = k_hi - k_lo + 1
        if n_bins < 1 or B < 1 or max(n_bins, B, tol) > SALIENCE_MAX_BINS:
            raise ValueError(f"salience: {n_bins} STFT bins / {B} pitch bins / tol {tol}: each must be in 1..{SALIENCE_MAX_BINS}")
        self.B, self.k_lo, self.n_bins, self.H, self.Fs = B, k_lo, n_bins, int(H), Fs
        self.F_coef_hertz = F_min * np.power(2, (np.arange(0, B) * R / 1200))
        i = np.arange(N, dtype=np.int64)
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * i.astype(np.float64) / N)                      # periodic Hann of N
        ang = 2.0 * np.pi * ((i[:, None] * np.arange(k_lo, k_hi + 1, dtype=np.int64)[None, :]) % N) / N
        table = np.empty((N, 2 * n_bins), dtype=np.float64)
        table[:, 0::2] = w[:, None] * np.cos(ang)
        table[:, 1::2] = -w[:, None] * np.sin(ang)
        off, hw = harmonic_weights(B, R, num_harm, alpha)
        if len(off) < 1 or len(off) > SALIENCE_MAX_BINS:
            raise ValueError(f"salience: {len(off)} harmonic taps, must be in 1..{SALIENCE_MAX_BINS}")
        self.basis = torch.from_numpy(table.astype(np.float32)).to(device)
        self.smooth = torch.from_numpy(np.hanning(freq_smooth_len).astype(np.float32)).to(device)
        self.harm_off = torch.from_numpy(off).to(device)
        self.harm_w = torch.from_numpy(hw.astype(np.float32)).to(device)
        self.log_hi = float(np.log(np.float64(score_high) + np.float32(EPS32)))
        self.log_lo = float(np.log(np.float64(score_low) + np.float32(EPS32)))
        s = self.struct = SaliencePlan()
        s.basis, s.smooth, s.harm_off, s.harm_w = self.basis.data_ptr(), self.smooth.data_ptr(), self.harm_off.data_ptr(), self.harm_w.data_ptr()
        s.n_fft, s.hop, s.k_lo, s.n_bins = int(N), int(H), k_lo, n_bins
        s.n_pitch, s.smooth_len, s.n_harm, s.tol = B, int(freq_smooth_len), len(off), int(tol)
        s.fs, s.f_min, s.f_max, s.bins_per_octave = float(Fs), float(F_min), float(F_max), 1200.0 / float(R)
        s.thresh, s.log_hi, s.log_lo = 10.0 ** (float(gamma) / 20.0), self.log_hi, self.log_lo


def salience_plan(Fs=22050, N=2048, H=256, F_min=55.0, F_max=1760.0, R=10.0, num_harm=10, freq_smooth_len=11, alpha=0.9, gamma=0.0,
                  tol=5, score_low=0.01, score_high=1.0, device="cuda"):
    """The cached ``Plan`` of one parameter set on one device."""
    key = (float(Fs), int(N), int(H), float(F_min), float(F_max), float(R), int(num_harm), int(freq_smooth_len), float(alpha), float(gamma),
           int(tol), float(score_low), float(score_high), str(torch.device(device)))
    with _LOCK:
        plan = _PLANS.get(key)
    if plan is None:
        plan = Plan(Fs, N, H, F_min, F_max, R, num_harm, freq_smooth_len, alpha, gamma, tol, score_low, score_high, device)
        with _LOCK:
            plan = _PLANS.setdefault(key, plan)
    return plan


@torch.no_grad()
def salience_begin(x, plan, ops, want_sal=False):
    """The device half: ``x`` float32 [n] on the plan's device -> everything ENQUEUED on the current stream, nothing waits.  Returns
    ``finish() -> (index int64 [frames], sal float64 [frames] or None)`` which does ONE device -> host copy."""
    if x.dim() != 1:
        raise ValueError(f"salience: expected a mono signal [n], got {tuple(x.shape)}")
    if 1 + x.shape[0] // plan.H < 2:
        raise ValueError(f"salience: {x.shape[0]} samples at hop {plan.H} give one frame; the phase increment needs at least 2")
    if x.shape[0] > 1 and x.stride(0) != 1:
        x = x.contiguous()
    if want_sal:
        path, z = ops.salience_f0_fwd(plan.struct, x, want_map=True)
        # Z_norm[index, n] = Z / column maximum (salience.py:84-86; 0 / 0 = NaN on a silent column, like the reference)
        picked = z.gather(1, path.to(torch.int64)[:, None])[:, 0].double() / z.max(dim=1).values.double()
        both = torch.stack([path.double(), picked])                           # indices < 1024 are exact in float64
    else:
        both = ops.salience_f0_fwd(plan.struct, x)

    def finish():
        host = both.cpu()
        if want_sal:
            return host[0].to(torch.int64).numpy(), host[1].numpy()
        return host.to(torch.int64).numpy(), None
    return finish


def salience(x, Fs=22050, N=2048, H=256, F_min=55.0, F_max=1760.0, R=10.0, num_harm=10, freq_smooth_len=11,
             alpha=0.9, gamma=0.0, constraint_region=None, tol=5, score_low=0.01, score_high=1.0, device=None, ops=None):
    """pitch/core/salience.py:13-89.  ``x``: mono signal [n] (numpy, or a tensor on any device).  Returns (f0 [frames] Hz, always voiced;
    T_coef [frames] seconds; sal [frames], the salience of the chosen bin over its column's maximum), float64 like the reference."""
    if constraint_region is not None:
        raise ValueError("salience: constraint regions are not implemented (compute_f0_salience never passes one)")
    ops = ops if ops is not None else _default_ops()
    x = torch.as_tensor(x)
    if device is None:
        device = x.device if (x.is_cuda or not ops.on_gpu) else "cuda"
    plan = salience_plan(Fs, N, H, F_min, F_max, R, num_harm, freq_smooth_len, alpha, gamma, tol, score_low, score_high, device)
    index, sal = salience_begin(x.to(device, torch.float32), plan, ops, want_sal=True)()
    traj = plan.F_coef_hertz[index]
    T_coef = (np.arange(index.shape[0]) * H) / Fs
    return traj, T_coef, sal
