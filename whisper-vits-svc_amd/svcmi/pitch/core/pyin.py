"""Drop-in for the reference's pitch/core/pyin.py ``pyin`` (libf0's pYIN: YIN's difference function per frame, a sweep of thresholds
weighted by a beta distribution, a voiced / unvoiced HMM decoded with Viterbi) -- on the kernels of csrc/pyin.hip.

    f0, t, conf = pyin(audio, Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0)      # float64 [1 + n // H] each; f0 = 0 where unvoiced

The device reproduces the reference as it executes under numpy (``numba.njit`` as the identity), defects included: DESIGN.md 4.10.  The host
makes the plan once per parameter set and device (``pyin_plan``): the beta weights, the frequency axis, the transition matrix as a band
gathered by column, the constants.  Everything per clip runs on the device (``pyin_begin``: enqueued, nothing waits).

Differences from the reference, on purpose: ``N`` must be even, fewer than two frames raise ValueError, and parameters beyond the
kernels' limits (B <= 1024 pitch bins, 128 thresholds, N <= 4096, a transition band of at most 33) raise ValueError.
"""
import threading

import numpy as np
import torch

from ..._lib import PYIN_MAX_BAND, PYIN_MAX_BINS, PYIN_MAX_NFFT, PYIN_MAX_THRESHOLDS, PyinPlan
from ...ops import Ops

TINY = float(np.finfo(0.).tiny)
MAX_STEP_CENTS = 50          # pitch/core/pyin.py:80
PROB_SELF = 0.99             # compute_transition_matrix
_PLANS = {}
_OPS = None
_LOCK = threading.Lock()


def _default_ops():
    global _OPS
    with _LOCK:
        if _OPS is None:
            _OPS = Ops()
        return _OPS


def beta_weights(thresholds, beta_params):
    """pitch/core/pyin.py:67-70: the beta-binomial weight of every threshold."""
    from scipy.special import beta, comb
    n = len(thresholds)
    idx = np.arange(n)
    return comb(n, idx) * beta(idx + beta_params[0], n - idx + beta_params[1]) / beta(beta_params[0], beta_params[1])


def transition_rows(B, max_step):
    """The voiced block of ``compute_transition_matrix`` as windows: rows[i, d] = A[i, i - max_step + d] (0 outside the matrix), with the
    reference's three row regimes applied in its order -- the edge rows renormalised, the rows i < max_step one column short
    (A[i, 0 : i + max_step], not : i + max_step + 1).  The unvoiced block A[B + i, B + j] holds the same values."""
    from scipy.stats import triang
    ms = int(max_step)
    t = triang.pdf(np.arange(-ms, ms + 1), 0.5, scale=2 * ms, loc=-ms)
    rows = np.zeros((B, 2 * ms + 1))
    for i in range(B):
        col0 = i - ms                                                    # the window's first column
        if i < ms:
            v = PROB_SELF * t[ms - i:-1] / np.sum(t[ms - i:-1])          # columns 0 .. i + ms - 1
            rows[i, 0 - col0:0 - col0 + len(v)] = v
        if ms <= i < B - ms:
            rows[i, :] = PROB_SELF * t
        if i >= B - ms:
            v = PROB_SELF * t[0:ms - (i - B)] / np.sum(t[0:ms - (i - B)])  # columns i - ms .. B - 1
            rows[i, 0:len(v)] = v
    return rows


def transition_band(B, max_step):
    """band[i, d] = log(A[i - max_step + d, i] + tiny): the rows above gathered by COLUMN (what state i's predecessors cost).  Zeros
    inside the window carry log(tiny), the constant of every transition outside it; entries whose row is outside the matrix hold log(tiny)
    too and are never read."""
    ms = int(max_step)
    rows = transition_rows(B, ms)
    band = np.zeros((B, 2 * ms + 1))
    for d in range(2 * ms + 1):
        j = np.arange(B) - ms + d                                        # the predecessor of state i
        ok = (j >= 0) & (j < B)
        band[ok, d] = rows[j[ok], 2 * ms - d]                            # column i in row j's window: i - (j - ms)
    return np.log(band + TINY)


class Plan:
    """One parameter set on one device: the filled ``struct`` (svcmi_pyin_plan), the tensors it points to, the float64 tables."""

    def __init__(self, Fs, N, H, F_min, F_max, R, thresholds, beta_params, absolute_min_prob, voicing_prob, device):
        thresholds = np.asarray(thresholds, dtype=np.float64)
        if N < 2 or N % 2 or H < 1 or not (0 < F_min <= F_max) or R <= 0 or thresholds.ndim != 1 or len(thresholds) < 1:
            raise ValueError(f"pyin: unsupported parameters N={N} H={H} F_min={F_min} F_max={F_max} R={R} thresholds={thresholds.shape}")
        if not (0.0 <= voicing_prob <= 1.0):
            raise ValueError(f"pyin: voicing_prob {voicing_prob} must lie in 0 .. 1")
        B = int(np.log2(F_max / F_min) * (1200 / R))
        max_step = int(MAX_STEP_CENTS / R)
        p_min = max(int(np.ceil(Fs / F_max)), 1)
        p_max = int(np.ceil(Fs / F_min))
        if max_step < 1 or B < 2 * max_step + 1:
            raise ValueError(f"pyin: R={R} gives max_step {max_step} and {B} pitch bins; needs max_step >= 1 and at least 2 max_step + 1 bins")
        if B > PYIN_MAX_BINS or len(thresholds) > PYIN_MAX_THRESHOLDS or N > PYIN_MAX_NFFT or 2 * max_step + 1 > PYIN_MAX_BAND or p_max > N:
            raise ValueError(f"pyin: {B} pitch bins / {len(thresholds)} thresholds / N {N} / band {2 * max_step + 1} / p_max {p_max}: the limits "
                             f"are {PYIN_MAX_BINS} / {PYIN_MAX_THRESHOLDS} / {PYIN_MAX_NFFT} / {PYIN_MAX_BAND} / N")
        self.B, self.H, self.N, self.Fs, self.max_step, self.p_min, self.p_max = B, int(H), int(N), Fs, max_step, p_min, p_max
        self.thresholds_np = thresholds
        self.beta_np = np.asarray(beta_weights(thresholds, beta_params), dtype=np.float64)
        self.F_axis = F_min * np.power(2, np.arange(B) * R / 1200)
        self.band_np = transition_band(B, max_step)
        self.log_tiny = float(np.log(np.float64(0.0) + TINY))
        self.log_cross = float(np.log(np.float64(1 - PROB_SELF) + TINY))
        self.log_c = float(np.log(np.float64(1.0) / (2 * B) + TINY))
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        self.thresholds, self.beta, self.f_axis, self.band = to(thresholds), to(self.beta_np), to(self.F_axis), to(self.band_np)
        s = self.struct = PyinPlan()
        s.thresholds, s.beta, s.f_axis, s.band = self.thresholds.data_ptr(), self.beta.data_ptr(), self.f_axis.data_ptr(), self.band.data_ptr()
        s.n_fft, s.hop, s.p_min, s.p_max = int(N), int(H), p_min, p_max
        s.n_pitch, s.n_thr, s.max_step, s.reserved = B, len(thresholds), max_step, 0
        s.fs, s.tol_cents, s.absolute_min_prob, s.voicing_prob = float(Fs), float(R), float(absolute_min_prob), float(voicing_prob)
        s.log_tiny, s.log_cross, s.log_c, s.tiny = self.log_tiny, self.log_cross, self.log_c, TINY


def pyin_plan(Fs=22050, N=2048, H=256, F_min=55.0, F_max=1760.0, R=10, thresholds=np.arange(0.01, 1, 0.01), beta_params=(1, 18),
              absolute_min_prob=0.01, voicing_prob=0.5, device="cuda"):
    """The cached ``Plan`` of one parameter set on one device."""
    thr = np.asarray(thresholds, dtype=np.float64)
    key = (float(Fs), int(N), int(H), float(F_min), float(F_max), float(R), thr.tobytes(), float(beta_params[0]), float(beta_params[1]),
           float(absolute_min_prob), float(voicing_prob), str(torch.device(device)))
    with _LOCK:
        plan = _PLANS.get(key)
    if plan is None:
        plan = Plan(Fs, N, H, F_min, F_max, R, thr, beta_params, absolute_min_prob, voicing_prob, device)
        with _LOCK:
            plan = _PLANS.setdefault(key, plan)
    return plan


@torch.no_grad()
def pyin_begin(x, plan, ops):
    """The device half: ``x`` float32 [n] on the plan's device -> everything ENQUEUED on the current stream, nothing waits.  Returns
    ``finish() -> (f0 float64 [frames], conf float64 [frames])`` which does ONE device -> host copy."""
    if x.dim() != 1:
        raise ValueError(f"pyin: expected a mono signal [n], got {tuple(x.shape)}")
    if 1 + x.shape[0] // plan.H < 2:
        raise ValueError(f"pyin: {x.shape[0]} samples at hop {plan.H} give one frame; the trajectory needs at least 2")
    if x.shape[0] > 1 and x.stride(0) != 1:
        x = x.contiguous()
    out, _ = ops.pyin_f0_fwd(plan.struct, x)

    def finish():
        host = out.cpu().numpy()
        return host[0], host[1]
    return finish


def pyin(x, Fs=22050, N=2048, H=256, F_min=55.0, F_max=1760.0, R=10, thresholds=np.arange(0.01, 1, 0.01), beta_params=[1, 18],
         absolute_min_prob=0.01, voicing_prob=0.5, device=None, ops=None):
    """pitch/core/pyin.py:15-108.  ``x``: mono signal [n] (numpy, or a tensor on any device).  Returns (f0 [frames] Hz, 0 where unvoiced;
    t [frames] seconds; conf [frames], the observation of the decoded state over its column's maximum), float64 like the reference.  The
    two exceptions of the reference are raised with its messages."""
    if F_min > F_max:
        raise Exception("F_min must be smaller than F_max!")
    if F_min < Fs / N:
        raise Exception(f"The condition (F_min >= Fs/N) was not met. With Fs = {Fs}, N = {N} and F_min = {F_min} you have the following options: \n"
                        f"1) Set F_min >= {np.ceil(Fs/N)} Hz. \n2) Set N >= {np.ceil(Fs/F_min).astype(int)}. \n3) Set Fs <= {np.floor(F_min * N)} Hz.")
    ops = ops if ops is not None else _default_ops()
    x = torch.as_tensor(x)
    if device is None:
        device = x.device if (x.is_cuda or not ops.on_gpu) else "cuda"
    plan = pyin_plan(Fs, N, H, F_min, F_max, R, thresholds, beta_params, absolute_min_prob, voicing_prob, device)
    f0, conf = pyin_begin(x.to(device, torch.float32), plan, ops)()
    t = np.arange(f0.shape[0]) * H / Fs
    return f0, t, conf
