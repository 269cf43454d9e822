"""Drop-in for the reference's pitch/core/yin.py ``yin`` (libf0's YIN: the cumulative mean normalised difference function per frame, the
first minimum below an absolute threshold, a refinement inside +/- 25 cents, the aperiodicity of the frame at the lag found) -- on the
kernels of csrc/yin.hip.

    f0, t, ap = yin(audio, Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0)      # float64 [1 + n // H] each; every frame has an f0

The device reproduces the reference as it executes under numpy (``numba.njit`` as the identity): DESIGN.md 4.12.  YIN decides no voicing:
``ap`` (0 = perfectly periodic) is the continuous measure a caller thresholds.  The plan (``yin_plan``) is plain numbers made once per
parameter set; everything per clip runs on the device (``yin_begin``: enqueued, nothing waits).

Differences from the reference, on purpose: ``N`` must be even and at most 4096, and an empty signal raises ValueError.
"""
import threading

import numpy as np
import torch

from ..._lib import YIN_MAX_NFFT, YinPlan
from ...ops import Ops

TOL_CENTS = 25               # pitch/core/yin.py:76
_PLANS = {}
_OPS = None
_LOCK = threading.Lock()


def _default_ops():
    global _OPS
    with _LOCK:
        if _OPS is None:
            _OPS = Ops()
        return _OPS


class Plan:
    """One parameter set: the filled ``struct`` (svcmi_yin_plan).  It holds no device memory, so one plan serves every device."""

    def __init__(self, Fs, N, H, F_min, F_max, threshold):
        if N < 2 or N % 2 or H < 1 or not (0 < F_min <= F_max) or not Fs > 0 or np.isnan(threshold):
            raise ValueError(f"yin: unsupported parameters Fs={Fs} N={N} H={H} F_min={F_min} F_max={F_max} threshold={threshold}")
        lag_min = max(int(np.ceil(Fs / F_max)), 1)
        lag_max = int(np.ceil(Fs / F_min))
        if N > YIN_MAX_NFFT or lag_max > N:
            raise ValueError(f"yin: N {N} / lag_max {lag_max}: the limits are {YIN_MAX_NFFT} / N")
        self.N, self.H, self.Fs, self.lag_min, self.lag_max, self.threshold = int(N), int(H), Fs, lag_min, lag_max, float(threshold)
        # the refinement window's factors as the reference's expression evaluates them (Python floats)
        self.ratio_up, self.ratio_down = 2 ** (TOL_CENTS / 1200), 2 ** (-TOL_CENTS / 1200)
        s = self.struct = YinPlan()
        s.n_fft, s.hop, s.lag_min, s.lag_max = int(N), int(H), lag_min, lag_max
        s.fs, s.threshold, s.ratio_up, s.ratio_down = float(Fs), float(threshold), self.ratio_up, self.ratio_down


def yin_plan(Fs=22050, N=2048, H=256, F_min=55.0, F_max=1760.0, threshold=0.15, device=None):
    """The cached ``Plan`` of one parameter set.  ``device`` is accepted like ``pyin_plan``'s and not used: the plan is the same everywhere."""
    key = (float(Fs), int(N), int(H), float(F_min), float(F_max), float(threshold))
    with _LOCK:
        plan = _PLANS.get(key)
    if plan is None:
        plan = Plan(Fs, N, H, F_min, F_max, threshold)
        with _LOCK:
            plan = _PLANS.setdefault(key, plan)
    return plan


@torch.no_grad()
def yin_begin(x, plan, ops):
    """The device half: ``x`` float32 [n >= 1] on the device of ``ops`` -> everything ENQUEUED on the current stream, nothing waits.
    Returns ``finish() -> (f0 float64 [frames], ap float64 [frames])`` which does ONE device -> host copy."""
    if x.dim() != 1:
        raise ValueError(f"yin: expected a mono signal [n], got {tuple(x.shape)}")
    if x.shape[0] < 1:
        raise ValueError("yin: the signal is empty")
    if x.shape[0] > 1 and x.stride(0) != 1:
        x = x.contiguous()
    out = ops.yin_f0_fwd(plan.struct, x)

    def finish():
        host = out.cpu().numpy()
        return host[0], host[1]
    return finish


def yin(x, Fs=22050, N=2048, H=256, F_min=55.0, F_max=1760.0, threshold=0.15, verbose=False, device=None, ops=None):
    """pitch/core/yin.py:11-92.  ``x``: mono signal [n] (numpy, or a tensor on any device).  Returns (f0 [frames] Hz; t [frames] seconds;
    ap [frames], the aperiodicity: the lower, the more reliable the estimate), float64 like the reference.  The two exceptions of the
    reference are raised with its messages.  ``verbose`` is accepted and ignored: there is no per-frame loop to report on."""
    if F_min > F_max:
        raise Exception("F_min must be smaller than F_max!")
    if F_min < Fs / N:
        raise Exception(f"The condition (F_min >= Fs/N) was not met. With Fs = {Fs}, N = {N} and F_min = {F_min} you have the following options: \n"
                        f"1) Set F_min >= {np.ceil(Fs/N)} Hz. \n2) Set N >= {np.ceil(Fs/F_min).astype(int)}. \n3) Set Fs <= {np.floor(F_min * N)} Hz.")
    ops = ops if ops is not None else _default_ops()
    x = torch.as_tensor(x)
    if device is None:
        device = x.device if (x.is_cuda or not ops.on_gpu) else "cuda"
    plan = yin_plan(Fs, N, H, F_min, F_max, threshold)
    f0, ap = yin_begin(x.to(device, torch.float32), plan, ops)()
    t = np.arange(f0.shape[0]) * H / Fs
    return f0, t, ap
