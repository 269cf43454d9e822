"""Checks of the fused linear spectrogram (csrc/spectrogram.hip: reflect padding + windowed DFT on the fp32 matrix cores + magnitude in
one launch), shared by the emulator tests (CPU) and the GPU tests like tests/resample_cases.py: every function takes ``ops`` and ``device``.

Oracle: the reference recipe (vits/spectrogram.py:55-75) restated with CPU ``torch.stft`` in float64: reflect pad by
``int((n_fft - hop) / 2)``, periodic Hann window of ``win``, ``center=False``, ``sqrt(re^2 + im^2 + 1e-6)``.
Tolerance, derived and not tuned, per element: with u = 2^-24 and A[t] = sum_i |w_i x_pad[t hop + i]|,

    |out - oracle|  <=  sqrt(2) (n_fft + 2) u A[t]  +  4 u oracle

The first term is any-order fp32 accumulation of n_fft products plus one rounding of the table entry, for re and for im; the second the
squares, the sum, eps and the square root.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-6
SR = 32000
# (n_fft, hop, win, n)
SHAPES = [(1024, 320, 1024, 2560),              # 8 frames
          (1024, 320, 1024, 353),               # 1 frame, n = pad + 1: nearly all reflected
          (1024, 320, 1024, 320 * 67 + 17),     # 67 frames: three frame tiles, the last with 3 frames; unused tail
          (64, 20, 64, 203),
          (64, 16, 48, 200),                    # win < n_fft
          (2048, 240, 1200, 4000),              # long K
          (1024, 512, 1024, 3000),              # 31 hop + n_fft samples do not fit the block's LDS span: samples read from global memory
          (64, 7, 64, 300)]                     # odd hop: the LDS span without its skew
FULL = (1024, 320, 1024, 320000)                # GPU only: 10 s at 32 kHz -> [513, 1000]


def pad_of(n_fft, hop):
    return int((n_fft - hop) / 2)


def frames_of(n_fft, hop, n):
    return 1 + (n + 2 * pad_of(n_fft, hop) - n_fft) // hop


def tone_noise(n, seed=0):
    """0.5-amplitude 220 Hz tone + 0.05 white noise, first quarter exactly zero (silent frames: the eps floor, oracle = 1e-3)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = 0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.05 * rng.standard_normal(n)
    x[:n // 4] = 0.0
    return x.astype(np.float32)


def bin_tone_dc(n, n_fft):
    """A tone exactly on bin n_fft / 8 with a DC offset, full scale: the extremes are exactly +-1."""
    i = np.arange(n)
    x = 0.25 + 0.75 * np.cos(2 * np.pi * (n_fft // 8) * i / n_fft)
    x[0], x[min(n - 1, 4)] = 1.0, -1.0
    return x.astype(np.float32)


def inputs(n_fft, n):
    return [tone_noise(n, seed=n % 1009), bin_tone_dc(n, n_fft)]


def oracle(x32, n_fft, hop, win):
    """x32 [B, n] float32 (numpy) -> (float64 reference [B, bins, frames], per-element bound)."""
    x = torch.from_numpy(np.asarray(x32, dtype=np.float64))
    pad = pad_of(n_fft, hop)
    xp = torch.nn.functional.pad(x.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    w = torch.hann_window(win, dtype=torch.float64)
    spec = torch.stft(xp, n_fft, hop_length=hop, win_length=win, window=w, center=False, normalized=False, onesided=True, return_complex=True)
    ref = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + EPS)
    wp = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win) // 2
    wp[left:left + win] = w
    a = (xp.abs().unfold(1, n_fft, hop) * wp).sum(-1)                          # [B, frames]
    bound = math.sqrt(2.0) * (n_fft + 2) * U * a[:, None, :] + 4 * U * ref
    return ref.numpy(), bound.numpy()


def run(ops, device, x, n_fft, hop, win):
    """x: numpy [B, n] or a tensor on ``device`` (any batch stride) -> [B, bins, frames] through the public entry point."""
    from svcmi.vits.spectrogram import spectrogram_torch
    y = torch.from_numpy(x).to(device) if isinstance(x, np.ndarray) else x
    return spectrogram_torch(y, n_fft, SR, hop, win, center=False, ops=ops)


def worst_ratio(out, x32, n_fft, hop, win):
    ref, bound = oracle(x32, n_fft, hop, win)
    assert out.dtype == torch.float32 and tuple(out.shape) == ref.shape == (x32.shape[0], n_fft // 2 + 1, frames_of(n_fft, hop, x32.shape[1])), \
        (out.shape, ref.shape)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    assert np.isfinite(err).all()
    return float((err / bound).max())


def check_shape(ops, device, n_fft, hop, win, n):
    """Both inputs at one shape, every element against the float64 oracle; returns the largest error / bound."""
    worst = 0.0
    for x in inputs(n_fft, n):
        out = run(ops, device, x[None], n_fft, hop, win)
        assert out.is_contiguous() and str(out.device).startswith(str(device))
        worst = max(worst, worst_ratio(out, x[None], n_fft, hop, win))
    return worst


def strided_batch(device, n_fft, n):
    """batch = 3 with a non-contiguous batch stride: rows of a wider buffer.  Returns (view on ``device``, the same values as numpy)."""
    rows = np.stack([tone_noise(n, seed=5), bin_tone_dc(n, n_fft), tone_noise(n, seed=6)[::-1].copy()])
    buf = torch.full((3, n + 37), 7.0, dtype=torch.float32, device=device)
    buf[:, :n] = torch.from_numpy(rows).to(device)
    view = buf[:, :n]
    assert view.stride(0) == n + 37 and not view.is_contiguous()
    return view, rows


def check_batch(ops, device, n_fft=64, hop=20, win=64, n=203):
    """batch = 3, strided: inside the bound, and every item bit-equal to its solo run.  Returns the largest error / bound."""
    view, rows = strided_batch(device, n_fft, n)
    out = run(ops, device, view, n_fft, hop, win)
    worst = worst_ratio(out, rows, n_fft, hop, win)
    for b in range(3):
        solo = run(ops, device, rows[b:b + 1], n_fft, hop, win)
        assert torch.equal(out[b], solo[0]), b
    return worst


def check_crop(ops, device, n_fft=1024, hop=320, win=1024, n=320 * 45 + 17, first=5, count=36):
    """Interior frames of a clip against the same frames computed from a hop-aligned crop: other tiles, other lanes, another frame
    count -- the same bits.  Interior = the frame's n_fft samples touch no reflected sample in either signal."""
    x = tone_noise(n, seed=9) + bin_tone_dc(n, n_fft) * np.float32(0.25)
    x[: n // 4] += tone_noise(n, seed=10)[-(n // 4):]                       # no exactly silent part: every frame differs
    crop = x[first * hop: (first + count) * hop]
    full = run(ops, device, x[None], n_fft, hop, win)[0]
    part = run(ops, device, crop[None], n_fft, hop, win)[0]
    pad = pad_of(n_fft, hop)
    inner = [t for t in range(part.shape[1]) if t * hop - pad >= 0 and t * hop - pad + n_fft <= crop.shape[0]]
    assert len(inner) >= 30 and inner[0] >= 1
    idx = torch.tensor(inner, device=full.device)
    a, b = part.index_select(1, idx), full.index_select(1, idx + first)
    assert torch.equal(a, b), float((a - b).abs().max())
    assert not torch.equal(part[:, 0], full[:, first])                      # the reflected frames do differ: the check compares something


@functools.lru_cache(maxsize=None)
def _valid_call():
    """(n_fft, hop, pad, n, frames) of a call that launches: the error cases below change one argument each."""
    n_fft, hop, n = 64, 20, 203
    return n_fft, hop, pad_of(n_fft, hop), n, frames_of(n_fft, hop, n)


def check_argument_validation(ops, device):
    """Each error case returns SVCMI_EINVAL and leaves the output buffer untouched; the unchanged call launches and fills it."""
    from svcmi.vits.spectrogram import spectrogram_basis
    n_fft, hop, pad, n, frames = _valid_call()
    bins = n_fft // 2 + 1
    x = torch.from_numpy(tone_noise(n, seed=1)).to(device).view(1, n)
    basis = spectrogram_basis(n_fft, n_fft, device)
    out = torch.full((1, bins, frames), -5.0, dtype=torch.float32, device=device)
    f = ops.lib.svcmi_linear_spectrogram_f32
    stream = ops._stream()
    xp, bp, op = x.data_ptr(), basis.data_ptr(), out.data_ptr()
    cases = {
        "n <= pad": (xp, n, 1, pad, bp, n_fft, hop, pad, EPS, op, 1, stream),
        "n == pad - 1": (xp, n, 1, pad - 1, bp, n_fft, hop, pad, EPS, op, 1, stream),
        "frames < 1": (xp, n, 1, 30, bp, n_fft, hop, 10, EPS, op, 0, stream),                  # 30 + 20 < 64
        "hop < 1": (xp, n, 1, n, bp, n_fft, 0, pad, EPS, op, frames, stream),
        "hop negative": (xp, n, 1, n, bp, n_fft, -20, pad, EPS, op, frames, stream),
        "n_fft odd": (xp, n, 1, n, bp, n_fft - 1, hop, pad, EPS, op, 1 + (n + 2 * pad - (n_fft - 1)) // hop, stream),
        "null x": (None, n, 1, n, bp, n_fft, hop, pad, EPS, op, frames, stream),
        "null basis": (xp, n, 1, n, None, n_fft, hop, pad, EPS, op, frames, stream),
        "null out": (xp, n, 1, n, bp, n_fft, hop, pad, EPS, None, frames, stream),
        "another frame count": (xp, n, 1, n, bp, n_fft, hop, pad, EPS, op, frames + 1, stream),
    }
    for name, args in cases.items():
        assert f(*args) == -1, name
    if ops.on_gpu:
        torch.cuda.synchronize()
    assert bool((out == -5.0).all()), "an error case wrote to the output"
    assert f(xp, n, 1, n, bp, n_fft, hop, pad, EPS, op, frames, stream) == 0
    if ops.on_gpu:
        torch.cuda.synchronize()
    assert bool((out > 0).all())
    assert torch.equal(out, run(ops, device, x, n_fft, hop, n_fft))
