"""Drop-in for the inference subset of the reference's speaker/utils/audio.py ``AudioProcessor``: what speaker/infer.py calls
(``load_wav``, ``trim_silence``, ``sound_norm``, ``melspectrogram``) for the configuration of speaker_pretrain/config.json.

    mel = normalise(20 log10(max(1e-5, mel_basis |STFT(preemphasis(y))|)))         speaker/utils/audio.py:354-391, 480-489, 561-571

On the GPU: pre-emphasis + reflect padding in one kernel, the windowed DFT (n_fft = win = 1024, hop 256, periodic Hann, centred) and the
mel projection as two launches of the implicit GEMM, magnitude and the dB / range normalisation / clip tail as two small kernels
(csrc/lstm.hip).  The mel filterbank is ``svcmi.whisper.audio.slaney_mel_filterbank`` (librosa.filters.mel's published algorithm).

``trim_silence`` and ``sound_norm`` decide a length and one scale factor from the whole clip: they run on the host in numpy.
"""
import math
from functools import lru_cache

import numpy as np
import torch

from ..._lib import SvcmiError
from ...whisper.audio import load_audio, load_audio_device, slaney_mel_filterbank


@lru_cache(maxsize=None)
def _operands(device, sr, n_fft, n_mels):
    """Packed GEMM operands: the DFT basis [2 * half, n_fft] (rows hann * cos | -hann * sin, zero rows as padding; half = the bin
    count rounded up to a multiple of 4) and the filterbank [n_mels, half]."""
    nbins = n_fft // 2 + 1
    half = (nbins + 3) // 4 * 4
    k = np.arange(n_fft, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / n_fft)                        # scipy.signal.get_window("hann", n, fftbins=True)
    ang = 2.0 * np.pi * np.outer(np.arange(nbins, dtype=np.float64), k) / n_fft
    basis = np.zeros((2 * half, n_fft), dtype=np.float32)
    basis[:nbins] = (win * np.cos(ang)).astype(np.float32)
    basis[half:half + nbins] = (-win * np.sin(ang)).astype(np.float32)
    fb = np.zeros((n_mels, half), dtype=np.float32)
    fb[:, :nbins] = slaney_mel_filterbank(sr, n_fft, n_mels)
    return torch.from_numpy(basis).to(device), torch.from_numpy(fb).to(device), nbins, half


class AudioProcessor:
    """``AudioProcessor(**config["audio"])`` with the reference's keyword names.  Settings the kernels do not implement raise."""

    def __init__(self, sample_rate=None, resample=False, num_mels=None, min_level_db=None, hop_length=None, win_length=None,
                 ref_level_db=None, fft_size=1024, preemphasis=0.0, signal_norm=None, symmetric_norm=None, max_norm=None,
                 mel_fmin=None, mel_fmax=None, spec_gain=20, stft_pad_mode="reflect", clip_norm=True, do_trim_silence=False,
                 trim_db=60, do_sound_norm=False, do_amp_to_db_mel=True, stats_path=None, frame_shift_ms=None, frame_length_ms=None,
                 ops=None, device=None, loader="host", **_):
        self.sample_rate, self.resample, self.num_mels = sample_rate, resample, num_mels
        self.min_level_db, self.ref_level_db, self.max_norm = min_level_db or 0, ref_level_db, 4.0 if max_norm is None else float(max_norm)
        self.fft_size, self.hop_length, self.win_length = fft_size, hop_length, win_length
        self.preemphasis, self.spec_gain = preemphasis, float(spec_gain)
        self.signal_norm, self.symmetric_norm, self.clip_norm = signal_norm, symmetric_norm, clip_norm
        self.mel_fmin, self.mel_fmax = mel_fmin or 0, mel_fmax
        self.do_trim_silence, self.trim_db, self.do_sound_norm = do_trim_silence, trim_db, do_sound_norm
        self.loader = loader
        bad = []
        if not sample_rate or not num_mels or not hop_length or not win_length:
            bad.append("sample_rate / num_mels / hop_length / win_length must be given")
        if frame_shift_ms or frame_length_ms:
            bad.append("frame_shift_ms / frame_length_ms")
        if win_length != fft_size:
            bad.append(f"win_length {win_length} != fft_size {fft_size}")
        if not (signal_norm and symmetric_norm and clip_norm) or stats_path:
            bad.append("only signal_norm + symmetric_norm + clip_norm without a stats file")
        if not do_amp_to_db_mel or float(spec_gain) != 20.0 or stft_pad_mode != "reflect":
            bad.append("do_amp_to_db_mel / spec_gain / stft_pad_mode")
        if not self.min_level_db < 0 or ref_level_db is None:
            bad.append("min_level_db must be negative, ref_level_db given")
        if self.mel_fmin != 0 or (mel_fmax is not None and sample_rate and float(mel_fmax) != sample_rate / 2.0):
            bad.append(f"mel_fmin {mel_fmin} / mel_fmax {mel_fmax}: only the full band 0 .. sample_rate / 2")
        if not preemphasis:
            bad.append("preemphasis 0")
        if bad:
            raise SvcmiError("AudioProcessor: configuration outside what svcmi implements (speaker_pretrain/config.json's form): " + "; ".join(bad))
        self._ops, self._device = ops, device

    @property
    def ops(self):
        if self._ops is None:
            from ...ops import Ops
            self._ops = Ops()
        return self._ops

    @property
    def device(self):
        return torch.device(self._device if self._device is not None else ("cuda" if self.ops.on_gpu else "cpu"))

    # ------------------------------------------------------------------ host side: load, trim, level
    def trim_silence(self, wav):
        """speaker/utils/audio.py:714-720: drop a 10 ms margin at both ends, then ``librosa.effects.trim(top_db=trim_db,
        frame_length=win_length, hop_length=hop_length)``.  librosa is not installed here: its published algorithm is RESTATED (parity
        unpinned) -- frame RMS over centred, zero-padded frames (``librosa.feature.rms``), in dB relative to the loudest frame with
        amin = 1e-5 (``amplitude_to_db(ref=np.max, top_db=None)``), frames above -top_db are sound, and the clip is cut to
        [first sound frame * hop, min(n, (last sound frame + 1) * hop))."""
        wav = np.asarray(wav)
        margin = int(self.sample_rate * 0.01)
        wav = wav[margin:-margin]
        start, end = self.trim_bounds(wav)
        return wav[start:end]

    def trim_bounds(self, wav):
        n, fl, hop = wav.shape[0], self.win_length, self.hop_length
        if n == 0:
            raise ValueError("trim_silence: nothing left after the 10 ms margins")
        y = np.pad(wav.astype(np.float64), fl // 2)
        frames = 1 + (y.shape[0] - fl) // hop
        csum = np.concatenate([[0.0], np.cumsum(y * y)])
        idx = np.arange(frames) * hop
        rms = np.sqrt(np.maximum(csum[idx + fl] - csum[idx], 0.0) / fl)
        amin = 1e-5
        db = 10.0 * np.log10(np.maximum(amin * amin, rms * rms)) - 10.0 * np.log10(max(amin * amin, float(rms.max()) ** 2))
        sound = np.flatnonzero(db > -float(self.trim_db))
        if sound.size == 0:
            return 0, 0
        return int(sound[0]) * hop, min(n, (int(sound[-1]) + 1) * hop)

    @staticmethod
    def sound_norm(x):
        """speaker/utils/audio.py:722-732."""
        return x / abs(x).max() * 0.95

    def load_wav(self, filename, sr=None):
        """speaker/utils/audio.py:735-759: mono float32 at ``sr`` (default: the processor's rate) through the project's loaders
        (``loader="gpu"``: decode + resampling in one kernel launch), then the optional trim and level normalisation."""
        sr = sr or self.sample_rate
        if self.loader == "gpu":
            x = load_audio_device(filename, sr=sr, device=self.device, ops=self.ops).cpu().numpy()
        else:
            x = load_audio(filename, sr=sr)
        if self.do_trim_silence:
            try:
                x = self.trim_silence(x)
            except ValueError:
                print(f" [!] File cannot be trimmed for silence - {filename}")
        if self.do_sound_norm:
            x = self.sound_norm(x)
        return x

    # ------------------------------------------------------------------ GPU: waveform -> normalised mel
    @torch.no_grad()
    def melspectrogram_device(self, y):
        """y: numpy / tensor [n] -> [frames, num_mels] float32 on the device (time-major: what the encoder reads), frames = 1 + n // hop."""
        ops = self.ops
        if not torch.is_tensor(y):
            y = torch.from_numpy(np.ascontiguousarray(np.asarray(y, dtype=np.float32)))
        x = y.to(self.device, torch.float32).reshape(1, -1).contiguous()
        n, pad = x.shape[1], self.fft_size // 2
        if n <= pad:
            raise ValueError(f"melspectrogram: {n} samples cannot be reflect-padded by {pad} (needs more than {pad})")
        basis, fb, nbins, half = _operands(str(self.device), self.sample_rate, self.fft_size, self.num_mels)
        frames = 1 + n // self.hop_length
        xp = ops.preemph_pad(x, pad, self.preemphasis)                                                   # [1, n + n_fft]
        ri = ops.conv(xp, basis, None, ksize=self.fft_size, stride=self.hop_length, pad=0, c_in=1, ldx=1, t_in=xp.shape[1],
                      t_out=frames, x_bstride=xp.stride(0))                                              # [1, frames, 2 * half]
        mag = ops.magnitude_spectrum(ri, nbins, half)                                                    # [1, frames, half]
        mel = ops.conv(mag, fb, None)                                                                    # [1, frames, num_mels]
        return ops.speaker_mel_finish(mel, self.ref_level_db, self.min_level_db, self.max_norm)[0]

    def melspectrogram(self, y):
        """speaker/utils/audio.py:561-571: float32 numpy [num_mels, frames], as the reference returns it."""
        return np.ascontiguousarray(self.melspectrogram_device(y).cpu().numpy().T)
