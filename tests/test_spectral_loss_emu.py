"""The checkpoint-scoring kernels (csrc/spectral_loss.hip) executed on the CPU by the SIMT emulator: tests/spectral_loss_cases.py at
every shape against float64 oracles, the determinism contract, the argument checks, the filterbank restatement against an independent
implementation, and -- where the reference tree is present -- the reference's own MultiResolutionSTFTLoss and TacotronSTFT."""
import sys
import types

import numpy as np
import pytest
import torch

from tests import spectral_loss_cases as L
from tests import spectrogram_cases as S
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("n_fft,hop,win,n", L.SHAPES)
def test_distance_sums_against_float64(ops, n_fft, hop, win, n):
    worst = L.check_shape(ops, "cpu", n_fft, hop, win, n)
    print(f"({n_fft}, {hop}, {win}, {n}): worst relative error of the three sums = {worst:.3e}")
    assert worst <= L.TOL


def test_distance_of_a_signal_to_itself_is_exactly_zero(ops):
    L.check_self_distance(ops, "cpu")


def test_strided_batch_equals_solo_runs_and_swaps_with_its_items(ops):
    worst = L.check_batch(ops, "cpu")
    print(f"batch 3, strided: worst relative error = {worst:.3e}")
    assert worst <= L.TOL


@pytest.mark.parametrize("shape", L.ABS_COUNTS)
def test_abs_diff_sum_against_float64(ops, shape):
    worst = L.check_abs_diff(ops, "cpu", shape)
    print(f"{shape}: worst relative error = {worst:.3e}")
    assert worst <= L.TOL


@pytest.mark.parametrize("n_fft,hop,win,n_mel,fmin,fmax,n", L.MEL_SHAPES)
def test_log_mel_within_derived_bound(ops, n_fft, hop, win, n_mel, fmin, fmax, n):
    worst = L.check_mel(ops, "cpu", n_fft, hop, win, n_mel, fmin, fmax, n)
    print(f"mel ({n_fft}, {hop}, {win}) x {n_mel}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_results_do_not_depend_on_the_thread_order(ops, monkeypatch):
    """SVCMI_EMU_ORDER=reverse runs the fibers of every scheduling round backwards: a missing barrier after the span staging or around
    the block reduction would show.  Each kernel once more, equal bits."""
    x, y = L.pair(1500)
    xg, yg = L.pair(1000)
    a = L.run_distance(ops, "cpu", x[None], y[None], 512, 50, 240)                      # spans in LDS
    b = L.run_distance(ops, "cpu", xg[None], yg[None], *L.GLOBAL_SMALL[:3])                 # spans from global memory
    tone = S.tone_noise(320 * 35 + 5, seed=3)[None]
    m = L.run_mel(ops, "cpu", tone, 1024, 320, 1024, 100, 50.0, 16000.0)
    p, q = torch.from_numpy(np.array(x[:1400]).reshape(1, 14, 100)), torch.from_numpy(np.array(y[:1400]).reshape(1, 14, 100))
    d = ops.abs_diff_sum(p, q)
    monkeypatch.setenv("SVCMI_EMU_ORDER", "reverse")
    assert np.array_equal(L.run_distance(ops, "cpu", x[None], y[None], 512, 50, 240), a)
    assert np.array_equal(L.run_distance(ops, "cpu", xg[None], yg[None], *L.GLOBAL_SMALL[:3]), b)
    assert torch.equal(L.run_mel(ops, "cpu", tone, 1024, 320, 1024, 100, 50.0, 16000.0), m)
    assert torch.equal(ops.abs_diff_sum(p, q), d)


def test_argument_validation(ops):
    L.check_argument_validation(ops, "cpu")


def test_ops_layer_validates_its_tensors(ops):
    from svcmi import SvcmiError
    from svcmi.vits.spectrogram import spectrogram_basis
    basis = spectrogram_basis(64, 64, "cpu")
    x = torch.zeros(1, 200)
    with pytest.raises(SvcmiError):
        ops.stft_distance(x, torch.zeros(1, 201), basis, 64, 16)                       # shapes differ
    with pytest.raises(SvcmiError):
        ops.stft_distance(x.double(), x.double(), basis, 64, 16)
    with pytest.raises(SvcmiError):
        ops.stft_distance(x, x, basis[:, :-2], 64, 16)
    with pytest.raises(SvcmiError):
        ops.stft_distance(x[:, :32], x[:, :32], basis, 64, 16)                         # n <= pad: no reflect padding
    with pytest.raises(SvcmiError):
        ops.stft_distance(x, x, basis, 64, 16, workspace=torch.zeros(2))
    with pytest.raises(SvcmiError):
        ops.log_mel(torch.zeros(1, 33, 12), torch.zeros(33, 10), 10)                   # the table is not padded to 32 columns
    with pytest.raises(SvcmiError):
        ops.abs_diff_sum(torch.zeros(2, 5), torch.zeros(2, 6))


def test_filterbank_restatement_against_transformers():
    """The numpy restatement of librosa.filters.mel's defaults (Slaney scale, Slaney norm) against an independent implementation of the
    same published algorithm, at configs/base.yaml's parameters."""
    from transformers.audio_utils import mel_filter_bank
    from svcmi.whisper.audio import slaney_mel_filterbank
    sr, n_fft, n_mel, fmin, fmax = 32000, 1024, 100, 50, 16000
    want = mel_filter_bank(num_frequency_bins=n_fft // 2 + 1, num_mel_filters=n_mel, min_frequency=fmin, max_frequency=fmax, sampling_rate=sr,
                           norm="slaney", mel_scale="slaney").T
    got = slaney_mel_filterbank(sr, n_fft, n_mel, fmin, fmax)
    assert got.dtype == np.float32 and got.shape == want.shape == (n_mel, n_fft // 2 + 1)
    assert float(np.abs(got.astype(np.float64) - want).max()) <= 1e-6
    assert np.array_equal(slaney_mel_filterbank(16000, 400, 80), slaney_mel_filterbank(16000, 400, 80, 0.0, 8000.0))      # the defaults are unchanged


def test_mel_table_layout():
    from svcmi.vits_extend.stft import mel_table
    from svcmi.whisper.audio import slaney_mel_filterbank
    t = mel_table(32000, 1024, 100, 50.0, 16000.0, "cpu")
    assert t.dtype == torch.float32 and tuple(t.shape) == (513, 128) and t.is_contiguous() and mel_table(32000, 1024, 100, 50.0, 16000.0, "cpu") is t
    assert np.array_equal(t[:, :100].numpy().T, slaney_mel_filterbank(32000, 1024, 100, 50.0, 16000.0)) and bool((t[:, 100:] == 0).all())


def test_multi_resolution_loss_against_float64(ops):
    """The drop-in class on a batch of 2 at two small resolutions (LDS and global spans): sc over the whole batch tensor, mag a mean, both
    averaged over the resolutions."""
    from svcmi.vits_extend.stft_loss import MultiResolutionSTFTLoss
    n, resolutions = 1000, [(64, 16, 48), (64, 200, 64)]
    ps = [L.pair(n, seed) for seed in (0, 1)]
    x, y = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    sc, mag = MultiResolutionSTFTLoss("cpu", resolutions, ops=ops)(torch.from_numpy(x), torch.from_numpy(y))
    assert sc.dtype == mag.dtype == torch.float32 and sc.dim() == 0
    want_sc = want_mag = 0.0
    for n_fft, hop, win in resolutions:
        mx, my = L.magnitudes64(x, n_fft, hop, win), L.magnitudes64(y, n_fft, hop, win)
        want_sc += float(torch.norm(my - mx, p="fro") / torch.norm(my, p="fro")) / len(resolutions)
        want_mag += float((my.log() - mx.log()).abs().mean()) / len(resolutions)
    assert abs(float(sc) - want_sc) <= L.TOL * want_sc and abs(float(mag) - want_mag) <= L.TOL * want_mag


@pytest.mark.needs_reference
def test_live_against_the_reference_multi_resolution_loss(ops):
    """vits_extend/stft_loss.py of the reference (torch only) on a batch of 2 at the four configured resolutions, n = 6000."""
    from oracle import ref_import
    ref_import._prepare()
    from vits_extend.stft_loss import MultiResolutionSTFTLoss as RefLoss
    from svcmi.vits_extend.stft_loss import MultiResolutionSTFTLoss
    n = 6000
    ps = [L.pair(n, seed) for seed in (0, 1)]
    x, y = torch.from_numpy(np.stack([p[0] for p in ps])), torch.from_numpy(np.stack([p[1] for p in ps]))
    want_sc, want_mag = RefLoss("cpu", L.RESOLUTIONS)(x, y)
    sc, mag = MultiResolutionSTFTLoss("cpu", L.RESOLUTIONS, ops=ops)(x, y)
    r_sc, r_mag = abs(float(sc) - float(want_sc)) / float(want_sc), abs(float(mag) - float(want_mag)) / float(want_mag)
    print(f"sc {float(sc):.7f} vs {float(want_sc):.7f} ({r_sc:.2e})  mag {float(mag):.7f} vs {float(want_mag):.7f} ({r_mag:.2e})")
    assert r_sc <= L.TOL and r_mag <= L.TOL


@pytest.mark.needs_reference
def test_live_against_the_reference_tacotron_stft(ops, monkeypatch):
    """TacotronSTFT.mel_spectrogram of the reference.  Its two librosa imports are stubbed here: ``librosa.filters.mel`` returns the
    transformers filterbank, so this pins the RECIPE AROUND the filterbank (padding, window, magnitude, projection, clamp, log), not the
    filterbank itself -- test_filterbank_restatement_against_transformers does that.  The reference (fp32 torch.stft and matmul) is itself
    within the derived bound of the float64 oracle, so the two are within twice the bound of each other."""
    from transformers.audio_utils import mel_filter_bank
    from oracle import ref_import
    ref_import._prepare()

    def fake_mel(sr, n_fft, n_mels, fmin, fmax):
        return mel_filter_bank(num_frequency_bins=n_fft // 2 + 1, num_mel_filters=n_mels, min_frequency=fmin, max_frequency=fmax,
                               sampling_rate=sr, norm="slaney", mel_scale="slaney").T.astype(np.float32)

    lib, fil, util = types.ModuleType("librosa"), types.ModuleType("librosa.filters"), types.ModuleType("librosa.util")
    fil.mel, util.normalize = fake_mel, (lambda *a, **k: None)
    lib.filters, lib.util = fil, util
    for name, mod in (("librosa", lib), ("librosa.filters", fil), ("librosa.util", util)):
        monkeypatch.setitem(sys.modules, name, mod)
    monkeypatch.delitem(sys.modules, "vits_extend.stft", raising=False)
    from vits_extend.stft import TacotronSTFT as RefSTFT
    monkeypatch.delitem(sys.modules, "vits_extend.stft", raising=False)             # imported under the stubs: not left for other tests
    n_fft, hop, win, n_mel, fmin, fmax, n = L.MEL_SHAPES[0]
    x = np.stack([S.tone_noise(n, seed=n % 1009), S.tone_noise(n, seed=3)[::-1].copy()])
    want = RefSTFT(n_fft, hop, win, n_mel, S.SR, fmin, fmax, center=False, device="cpu").mel_spectrogram(torch.from_numpy(x))
    got = L.run_mel(ops, "cpu", x, n_fft, hop, win, n_mel, fmin, fmax)
    _, bound, _ = L.mel_oracle(x, n_fft, hop, win, n_mel, fmin, fmax)
    assert tuple(got.shape) == tuple(want.shape)
    ratio = float(((got.double() - want.double()).abs().numpy() / (2 * bound)).max())
    print(f"|ours - reference| / (2 bound) = {ratio:.3f}")
    assert ratio <= 1.0
