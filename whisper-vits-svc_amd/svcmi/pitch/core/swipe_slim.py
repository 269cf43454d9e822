"""Drop-in for the reference's pitch/core/swipe_slim.py ``swipe_slim`` (libf0's SWIPE' on a log-frequency spectrogram: the spectrum is
correlated with prime-harmonic sawtooth kernels at one power-of-two window size per octave of candidates) -- on the kernels of
csrc/swipe.hip.

    f0, t, conf = swipe_slim(audio, Fs=16000, H=320, F_min=45.0, F_max=1760.0)      # float64 [ceil(n / H)] each; conf = pitch strength

The host makes the plan once per parameter set and device (``swipe_plan``): the axes, the kernel matrix (``compute_kernel`` and
``prime_and_one`` restated), per window size the DFT basis, the candidates with their weights, and W_N -- the reference's
``interp1d(kind='cubic')`` from the linear to the log-frequency axis is a fixed linear map, tabulated in float64 by sending the identity
through scipy's ``interp1d`` and cast to fp32.  Everything per clip runs on the device (``swipe_begin``: enqueued, nothing waits).

The reference's two edge defects: an arg-max at candidate 0 reads row -1, which numpy wraps to the last candidate --
reproduced; an arg-max at the last candidate reads one row past the end and the reference raises IndexError for the whole clip --
``edge="raise"`` raises it with the reference's message, ``edge="clamp"`` gives such frames shift 0 (the last candidate's frequency).

Differences from the reference, on purpose: an empty clip and parameters beyond the kernels' limits (8 window sizes, N <= 4096, 1024
log-frequency bins, 1024 candidates) raise ValueError; a negative refined index at candidate 0 extrapolates the frequency axis where the
reference's ``interp1d`` raises ValueError.
"""
import threading

import numpy as np
import torch

from ..._lib import SWIPE_MAX_CANDIDATES, SWIPE_MAX_LOGBINS, SWIPE_MAX_NFFT, SWIPE_MAX_WINDOWS, SwipePlan
from ...ops import Ops

_PLANS = {}
_OPS = None
_LOCK = threading.Lock()


def _default_ops():
    global _OPS
    with _LOCK:
        if _OPS is None:
            _OPS = Ops()
        return _OPS


def prime_and_one(upto=1000000):
    """pitch/core/swipe_slim.py:162-180: 1, 2 and the odd primes up to ``upto``."""
    primes = np.arange(3, upto + 1, 2)
    isprime = np.ones((upto - 1) // 2, dtype=np.bool_)
    for factor in primes[:int(np.sqrt(upto)) // 2]:
        if isprime[(factor - 2) // 2]:
            isprime[(factor * 3 - 2) // 2::factor] = 0
    return np.concatenate((np.array([1, 2]), primes[isprime]))


def compute_kernel(f, F_coef_log_hz):
    """pitch/core/swipe_slim.py:121-159: the SWIPE' kernel of candidate ``f`` on the log-frequency axis, in the reference's operation order
    (a main peak OVERWRITES, a valley adds half a cosine), decayed by 1 / sqrt(frequency) and normalised by its positive part."""
    k = np.zeros(len(F_coef_log_hz))
    n_harmonics = np.floor(F_coef_log_hz[-1] / f).astype(np.int32)
    ratio = F_coef_log_hz / f
    for p in prime_and_one(100)[:n_harmonics]:
        a = np.abs(ratio - p)
        main = a < 0.25
        k[main] = np.cos(np.dot(np.array(2 * np.pi).reshape(-1, 1), ratio[main].reshape(1, -1))).flatten()
        valley = np.logical_and(0.25 < a, a < 0.75)
        k[valley] += np.cos(np.dot(np.array(2 * np.pi).reshape(-1, 1), ratio[valley].reshape(1, -1))).flatten() / 2
    k = np.multiply(k, np.sqrt(1.0 / F_coef_log_hz))
    return k / np.linalg.norm(k[k > 0])


def resample_matrix(N, Fs, F_coef_log_hz):
    """W_N float64 [n_log, N / 2 + 1]: ``interp1d(F_coef_lin_hz, Y, kind='cubic', axis=0)(F_coef_log_hz)`` is linear in Y (a not-a-knot
    spline on a uniform grid), so the identity sent through it is its matrix."""
    from scipy.interpolate import interp1d
    lin = np.arange(N // 2 + 1) * Fs / N
    return interp1d(lin, np.eye(N // 2 + 1), kind="cubic", axis=0)(F_coef_log_hz)


def dft_basis(N):
    """float64 [N, 2 (N / 2 + 1)]: hann[i] cos(2 pi i k / N) at column 2k, -hann[i] sin(2 pi i k / N) at 2k + 1 (the periodic Hann window of
    librosa.stft; the angle from (i k) mod N, so it is exact for every N)."""
    i, k = np.arange(N)[:, None], np.arange(N // 2 + 1)[None, :]
    ang = 2.0 * np.pi * ((i * k) % N) / N
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    out = np.empty((N, 2 * (N // 2 + 1)))
    out[:, 0::2] = win[:, None] * np.cos(ang)
    out[:, 1::2] = -win[:, None] * np.sin(ang)
    return out


def _pad8(a):
    """Rows zero-padded to a multiple of 8 columns."""
    out = np.zeros((a.shape[0], (a.shape[1] + 7) & ~7), dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


class Plan:
    """One parameter set on one device: the filled ``struct`` (svcmi_swipe_plan), the tensors it points to, the float64 tables."""

    def __init__(self, Fs, H, F_min, F_max, R, strength_threshold, device):
        if not (Fs > 0 and H >= 1 and int(H) == H and 0 < F_min < F_max <= Fs / 2 and R > 0) or strength_threshold != strength_threshold:
            raise ValueError(f"swipe_slim: unsupported parameters Fs={Fs} H={H} F_min={F_min} F_max={F_max} R={R} threshold={strength_threshold}")
        # pitch/core/swipe_slim.py:51-69
        self.F_coef_log = np.arange(0, np.log2(Fs / 2 / F_min), R / 1200)
        self.F_coef_log_hz = F_min * 2 ** self.F_coef_log
        F_min_idx = int(np.argmin(np.abs(self.F_coef_log_hz - F_min)))
        F_max_idx = int(np.argmin(np.abs(self.F_coef_log_hz - F_max)))
        B, n_log = F_max_idx - F_min_idx, len(self.F_coef_log_hz)
        L_opt = np.log2(Fs * 8 / np.array([F_min, F_max]))
        L_rnd = np.arange(np.round(L_opt[1]), np.round(L_opt[0]) + 1).astype(np.int32)
        self.N_pow2 = [int(v) for v in 2 ** L_rnd.astype(np.int64)]
        if (B < 1 or B > SWIPE_MAX_CANDIDATES or n_log < 2 or n_log > SWIPE_MAX_LOGBINS or not 1 <= len(self.N_pow2) <= SWIPE_MAX_WINDOWS
                or min(self.N_pow2) < 8 or max(self.N_pow2) > SWIPE_MAX_NFFT):
            raise ValueError(f"swipe_slim: {B} candidates / {n_log} log-frequency bins / window sizes {self.N_pow2}: the limits are 1 .. "
                             f"{SWIPE_MAX_CANDIDATES} / 2 .. {SWIPE_MAX_LOGBINS} / at most {SWIPE_MAX_WINDOWS} sizes in 8 .. {SWIPE_MAX_NFFT}")
        cands = self.F_coef_log_hz[F_min_idx:F_max_idx]
        self.kernels = np.zeros((B, n_log))
        for i, f in enumerate(cands):
            self.kernels[i, :] = compute_kernel(f, self.F_coef_log_hz)
        self.err = np.abs(np.log2(8 * Fs / cands) - np.log2(np.max(self.N_pow2)))
        self.B, self.n_log, self.H, self.Fs, self.F_min, self.R = B, n_log, int(H), Fs, float(F_min), R
        self.step, self.threshold = R / 1200, float(strength_threshold)
        self.windows, self._keep = [], []
        s = self.struct = SwipePlan()
        for octave, N in enumerate(self.N_pow2):
            mask = (self.err > octave - 1) & (self.err < octave + 1)
            cand = np.nonzero(mask)[0].astype(np.int32)
            if len(cand) < 1:
                raise ValueError(f"swipe_slim: window size {N} serves no candidate")
            mu = 1 - np.abs(self.err[mask] - octave)
            W = resample_matrix(N, Fs, self.F_coef_log_hz)
            self.windows.append(dict(N=N, cand=cand, mu=mu, W=W, K=self.kernels[cand]))
            to = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
            t = [to(dft_basis(N)), to(_pad8(W)), to(_pad8(self.kernels[cand])), to(cand, np.int32), to(mu)]
            self._keep.append(t)
            w = s.win[octave]
            w.basis, w.resample, w.kernels, w.cand, w.mu = (v.data_ptr() for v in t)
            w.n_fft, w.n_cand = N, len(cand)
        s.n_win, s.hop, s.n_log, s.n_pitch = len(self.N_pow2), int(H), n_log, B
        s.f_min, s.step, s.threshold = float(F_min), self.step, self.threshold


def swipe_plan(Fs=22050, H=256, F_min=55.0, F_max=1760.0, R=10, strength_threshold=0, device="cuda"):
    """The cached ``Plan`` of one parameter set on one device."""
    key = (float(Fs), int(H), float(F_min), float(F_max), float(R), float(strength_threshold), str(torch.device(device)))
    with _LOCK:
        plan = _PLANS.get(key)
    if plan is None:
        plan = Plan(Fs, H, F_min, F_max, R, strength_threshold, device)
        with _LOCK:
            plan = _PLANS.setdefault(key, plan)
    return plan


@torch.no_grad()
def swipe_begin(x, plan, ops, edge="raise"):
    """The device half: ``x`` float32 [n] on the plan's device -> everything ENQUEUED on the current stream, nothing waits.  Returns
    ``finish() -> (f0 float64 [frames], conf float64 [frames])`` which does ONE device -> host copy and applies ``edge``."""
    if edge not in ("raise", "clamp"):
        raise ValueError(f"swipe_slim: edge must be 'raise' or 'clamp', got {edge!r}")
    if x.dim() != 1 or x.shape[0] < 1:
        raise ValueError(f"swipe_slim: expected a mono signal [n] with n >= 1, got {tuple(x.shape)}")
    if x.shape[0] > 1 and x.stride(0) != 1:
        x = x.contiguous()
    out = ops.swipe_f0_fwd(plan.struct, x)

    def finish():
        host = out.cpu().numpy()
        if edge == "raise" and host[2, 0] != 0:
            raise IndexError(f"index {plan.B} is out of bounds for axis 0 with size {plan.B}")
        return host[0], host[1]
    return finish


def swipe_slim(x, Fs=22050, H=256, F_min=55.0, F_max=1760.0, R=10, strength_threshold=0, device=None, ops=None, edge="raise"):
    """pitch/core/swipe_slim.py:13-118.  ``x``: mono signal [n] (numpy, or a tensor on any device).  Returns (f0 [ceil(n / H)] Hz, 0 where
    conf < strength_threshold; t [frames] seconds; conf [frames], the pitch strength), float64 like the reference."""
    ops = ops if ops is not None else _default_ops()
    x = torch.as_tensor(x)
    if device is None:
        device = x.device if (x.is_cuda or not ops.on_gpu) else "cuda"
    plan = swipe_plan(Fs, H, F_min, F_max, R, strength_threshold, device)
    f0, conf = swipe_begin(x.to(device, torch.float32), plan, ops, edge=edge)()
    t = np.arange(0, x.shape[0], H) / Fs
    return f0, t, conf
