"""Drop-in for the reference's vits_extend/stft.py ``TacotronSTFT``: the linear and the log-mel spectrogram by which its validation step
compares a converted item with the recording (vits_extend/validation.py:28-31).

    stft = TacotronSTFT(1024, 320, 1024, 100, 32000, 50.0, 16000.0, device="cuda")
    mel = stft.mel_spectrogram(y)                    # y [B, n] in [-1, 1] -> float32 [B, 100, n // 320]

Two launches: csrc/spectrogram.hip (reflect pad ``int((n_fft - hop) / 2)``, ``center=False``, ``sqrt(re^2 + im^2 + 1e-9)``) and
svcmi_log_mel_f32 (the projection on the matrix cores and ``log(clamp(., 1e-5))``).  The filterbank is the project's numpy restatement of
librosa.filters.mel's defaults (Slaney scale, Slaney norm: ``svcmi.whisper.audio.slaney_mel_filterbank``); librosa is not a dependency.
Left out on purpose: the reference's ``assert min(y) >= -1`` / ``max(y) <= 1`` -- each is a host synchronisation in front of the launches.
``linear_spectrogram`` is ``torch.norm`` of the STFT, without an epsilon (stft.py:57-69).
"""
import threading

import numpy as np
import torch

from ..ops import Ops
from ..vits.spectrogram import spectrogram_basis
from ..whisper.audio import slaney_mel_filterbank

_TABLES = {}
_OPS = None
_LOCK = threading.Lock()


def _default_ops():
    global _OPS
    with _LOCK:
        if _OPS is None:
            _OPS = Ops()
        return _OPS


def mel_table(sampling_rate, n_fft, n_mels, fmin, fmax, device):
    """The operand of ``Ops.log_mel``: the filterbank TRANSPOSED, float32 [bins, ldm] with ldm = n_mels rounded up to 32 and zero columns
    past n_mels (the 32 lanes of a half-wave read 32 consecutive floats of one row).  Cached per argument tuple."""
    key = (int(sampling_rate), int(n_fft), int(n_mels), float(fmin), None if fmax is None else float(fmax), str(torch.device(device)))
    with _LOCK:
        table = _TABLES.get(key)
    if table is None:
        mel = slaney_mel_filterbank(sampling_rate, n_fft, n_mels, fmin, fmax)               # [n_mels, bins]
        padded = np.zeros((mel.shape[1], (n_mels + 31) // 32 * 32), dtype=np.float32)
        padded[:, :n_mels] = mel.T
        table = torch.from_numpy(padded).to(device)
        with _LOCK:
            table = _TABLES.setdefault(key, table)
    return table


class TacotronSTFT(torch.nn.Module):
    def __init__(self, filter_length=512, hop_length=160, win_length=512, n_mel_channels=80, sampling_rate=16000, mel_fmin=0.0, mel_fmax=None,
                 center=False, device="cpu", ops=None):
        super().__init__()
        if center:
            raise NotImplementedError("TacotronSTFT: center=True is not implemented (the reference never passes it)")
        self.n_mel_channels = n_mel_channels
        self.sampling_rate = sampling_rate
        self.n_fft = filter_length
        self.hop_size = hop_length
        self.win_size = win_length
        self.fmin = mel_fmin
        self.fmax = mel_fmax
        self.center = center
        self.ops = ops
        mel = slaney_mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)
        self.register_buffer("mel_basis", torch.from_numpy(mel).float().to(device))
        self.register_buffer("hann_window", torch.hann_window(win_length).to(device))

    def _magnitude(self, y, eps):
        ops = self.ops if self.ops is not None else _default_ops()
        if not y.is_cuda and ops.on_gpu:
            y = y.to(self.mel_basis.device if self.mel_basis.is_cuda else "cuda")
        y = y.to(torch.float32)
        if y.dim() != 2:
            raise ValueError(f"TacotronSTFT: expected [B, n], got {tuple(y.shape)}")
        if y.stride(1) != 1:
            y = y.contiguous()
        pad = int((self.n_fft - self.hop_size) / 2)
        if y.shape[1] <= pad:
            raise RuntimeError(f"TacotronSTFT: reflect padding {pad} needs more than {y.shape[1]} samples")
        return ops, ops.linear_spectrogram(y, spectrogram_basis(self.n_fft, self.win_size, y.device), self.n_fft, self.hop_size, pad, eps)

    @torch.no_grad()
    def linear_spectrogram(self, y):
        """stft.py:57-69: |STFT| [B, n_fft // 2 + 1, frames]."""
        return self._magnitude(y, 0.0)[1]

    @torch.no_grad()
    def mel_spectrogram(self, y):
        """stft.py:71-97: y [B, n] in [-1, 1] -> log(clamp(mel @ sqrt(|STFT|^2 + 1e-9), 1e-5)), float32 [B, n_mel_channels, frames]."""
        ops, spec = self._magnitude(y, 1e-9)
        table = mel_table(self.sampling_rate, self.n_fft, self.n_mel_channels, self.fmin, self.fmax, spec.device)
        return ops.log_mel(spec, table, self.n_mel_channels, 1e-5)
