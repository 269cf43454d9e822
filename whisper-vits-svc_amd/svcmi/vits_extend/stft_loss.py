"""Drop-in for the reference's vits_extend/stft_loss.py ``MultiResolutionSTFTLoss`` as a MEASURE (no autograd): spectral convergence and
log-STFT-magnitude distance of a predicted and a recorded batch, averaged over the resolutions of ``hp.mrd.resolutions``.

    loss = MultiResolutionSTFTLoss("cuda", [(1024, 120, 600), (2048, 240, 1200), (4096, 480, 2400), (512, 50, 240)])
    sc, mag = loss(fake[B, n], real[B, n])           # two float32 scalars on the device

One launch of svcmi_stft_distance_f32 per resolution: both signals through one read of the DFT table, ``sqrt(clamp(re^2 + im^2, 1e-7))``
(stft_loss.py:28), and three sums per item in fp64 -- no spectrogram is written.  From them, in fp64:
    sc  = sqrt(sum (my - mx)^2) / sqrt(sum my^2)     over the whole batch tensor, as torch.norm(., "fro") does (stft_loss.py:46)
    mag = sum |log my - log mx| / (B bins frames)    (F.l1_loss, stft_loss.py:64)
``window`` other than "hann_window" is not implemented: the table builder knows the periodic Hann window only.
"""
import torch

from ..vits.spectrogram import spectrogram_basis
from . import stft as _stft

FLOOR = 1e-7


def resolution_sums(ops, x, y, fft_size, shift_size, win_length):
    """float64 [B, 3] of one resolution (torch.stft's defaults: center=True, reflect): see ``Ops.stft_distance``."""
    return ops.stft_distance(x, y, spectrogram_basis(fft_size, win_length, x.device), fft_size, shift_size, fft_size // 2, FLOOR)


def sc_mag_from_sums(sums, fft_size, shift_size, n):
    """sums float64 [B, 3] -> (sc, mag) float64 scalars of that batch at one resolution."""
    total = sums.sum(0)
    count = sums.shape[0] * (fft_size // 2 + 1) * (1 + n // shift_size)
    return torch.sqrt(total[0]) / torch.sqrt(total[1]), total[2] / count


class STFTLoss(torch.nn.Module):
    def __init__(self, device, fft_size=1024, shift_size=120, win_length=600, window="hann_window", ops=None):
        super().__init__()
        if window != "hann_window":
            raise NotImplementedError(f"STFTLoss: window {window!r} is not implemented (hann_window only)")
        self.fft_size, self.shift_size, self.win_length, self.device, self.ops = fft_size, shift_size, win_length, device, ops

    @torch.no_grad()
    def forward(self, x, y):
        """x predicted, y recorded, [B, n] -> (sc, mag) float32 scalars (stft_loss.py:80-94)."""
        ops = self.ops if self.ops is not None else _stft._default_ops()
        x, y = _prepare(ops, x, self.device), _prepare(ops, y, self.device)
        sc, mag = sc_mag_from_sums(resolution_sums(ops, x, y, self.fft_size, self.shift_size, self.win_length), self.fft_size, self.shift_size,
                                   x.shape[1])
        return sc.float(), mag.float()


class MultiResolutionSTFTLoss(torch.nn.Module):
    def __init__(self, device, resolutions, window="hann_window", ops=None):
        super().__init__()
        self.device, self.ops = device, ops
        self.stft_losses = torch.nn.ModuleList([STFTLoss(device, fs, ss, wl, window, ops=ops) for fs, ss, wl in resolutions])

    @torch.no_grad()
    def forward(self, x, y):
        """stft_loss.py:114-133: the means over the resolutions, accumulated in fp64, returned as float32 scalars."""
        ops = self.ops if self.ops is not None else _stft._default_ops()
        x, y = _prepare(ops, x, self.device), _prepare(ops, y, self.device)
        sc_loss = torch.zeros((), dtype=torch.float64, device=x.device)
        mag_loss = torch.zeros((), dtype=torch.float64, device=x.device)
        for f in self.stft_losses:
            sc, mag = sc_mag_from_sums(resolution_sums(ops, x, y, f.fft_size, f.shift_size, f.win_length), f.fft_size, f.shift_size, x.shape[1])
            sc_loss += sc
            mag_loss += mag
        return (sc_loss / len(self.stft_losses)).float(), (mag_loss / len(self.stft_losses)).float()


def _prepare(ops, t, device):
    if t.dim() != 2:
        raise ValueError(f"STFTLoss: expected [B, n], got {tuple(t.shape)}")
    if not t.is_cuda and ops.on_gpu:
        t = t.to(device if torch.device(device).type == "cuda" else "cuda")
    t = t.to(torch.float32)
    return t if t.stride(1) == 1 else t.contiguous()
