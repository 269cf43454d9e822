"""Drop-in for the reference's vits/spectrogram.py ``spectrogram_torch`` and prepare/preprocess_spec.py ``compute_spec``: the linear
spectrogram every training item's posterior encoder reads, as ONE launch of csrc/spectrogram.hip (reflect padding, windowed DFT on the
fp32 matrix cores, magnitude).

    spec = spectrogram_torch(y[B, n], 1024, 32000, 320, 1024)        # [B, 513, n // 320] on the GPU
    compute_spec(hps.data, "waves-32k/s/f.wav", "specs/s/f.pt")       # torch.save of the CPU float32 [513, frames]
"""
import threading

import numpy as np
import torch

from ..ops import Ops

_BASIS = {}
_OPS = None
_LOCK = threading.Lock()


def _default_ops():
    global _OPS
    with _LOCK:
        if _OPS is None:
            _OPS = Ops()
        return _OPS


def spectrogram_basis(n_fft, win_size, device):
    """The kernel's DFT table, float32 [n_fft, n_fft + 2], cached per (n_fft, win_size, device):
    ``basis[i, 2k] = w[i] cos(2 pi ((k i) mod n_fft) / n_fft)``, the odd column with sin, for k < n_fft // 2 + 1; ``w`` is the periodic Hann
    window of ``win_size`` (torch.hann_window), centred and zero padded to ``n_fft`` as torch.stft does.  Built in float64 (the
    argument reduced exactly in integers first) and rounded once."""
    key = (int(n_fft), int(win_size), str(torch.device(device)))
    with _LOCK:
        basis = _BASIS.get(key)
    if basis is None:
        if n_fft < 2 or n_fft % 2 or not 1 <= win_size <= n_fft:
            raise ValueError(f"spectrogram_basis: n_fft {n_fft} must be even and win_size {win_size} in 1..n_fft")
        bins = n_fft // 2 + 1
        w = np.zeros(n_fft, dtype=np.float64)
        left = (n_fft - win_size) // 2
        w[left:left + win_size] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_size, dtype=np.float64) / win_size)
        ang = 2.0 * np.pi * ((np.arange(n_fft, dtype=np.int64)[:, None] * np.arange(bins, dtype=np.int64)[None, :]) % n_fft) / n_fft
        table = np.empty((n_fft, 2 * bins), dtype=np.float64)
        table[:, 0::2] = w[:, None] * np.cos(ang)
        table[:, 1::2] = w[:, None] * np.sin(ang)
        basis = torch.from_numpy(table.astype(np.float32)).to(device)
        with _LOCK:
            basis = _BASIS.setdefault(key, basis)
    return basis


@torch.no_grad()
def spectrogram_torch(y, n_fft, sampling_rate, hop_size, win_size, center=False, ops=None, device=None):
    """vits/spectrogram.py:41-76: ``y`` [B, n] float on any device -> sqrt(|STFT|^2 + 1e-6), float32 [B, n_fft // 2 + 1, frames] on the
    GPU (``device``: where a host tensor goes, default the current GPU; with an emulator ``ops`` the CPU).  Same prints as the reference."""
    if center:
        raise NotImplementedError("spectrogram_torch: center=True is not implemented (the reference never passes it)")
    ops = ops if ops is not None else _default_ops()
    if device is None:
        device = y.device if (y.is_cuda or not ops.on_gpu) else "cuda"
    y = y.to(device, torch.float32)
    if y.dim() != 2:
        raise ValueError(f"spectrogram_torch: expected [B, n], got {tuple(y.shape)}")
    lo, hi = torch.aminmax(y)
    if lo < -1.0:
        print("min value is ", lo)
    if hi > 1.0:
        print("max value is ", hi)
    if y.stride(1) != 1:
        y = y.contiguous()
    pad = int((n_fft - hop_size) / 2)
    if y.shape[1] <= pad:      # torch's reflect pad: "Padding size should be less than the corresponding input dimension"
        raise RuntimeError(f"spectrogram_torch: reflect padding {pad} needs more than {y.shape[1]} samples")
    return ops.linear_spectrogram(y, spectrogram_basis(n_fft, win_size, y.device), n_fft, hop_size, pad, 1e-6)


def compute_spec(hps, filename, specname, ops=None):
    """prepare/preprocess_spec.py:13-25: the int16 wav at ``hps.sampling_rate`` divided by ``hps.max_wav_value`` -> torch.save of the CPU
    float32 [bins, frames]."""
    from scipy.io import wavfile
    sampling_rate, data = wavfile.read(filename)
    assert sampling_rate == hps.sampling_rate, f"{sampling_rate} is not {hps.sampling_rate}"
    audio_norm = torch.from_numpy(data.astype(np.float32)) / hps.max_wav_value
    spec = spectrogram_torch(audio_norm.unsqueeze(0), hps.filter_length, hps.sampling_rate, hps.hop_length, hps.win_length, center=False, ops=ops)
    torch.save(torch.squeeze(spec, 0).cpu(), specname)
