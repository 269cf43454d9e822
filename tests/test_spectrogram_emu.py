"""The fused linear spectrogram (csrc/spectrogram.hip) executed on the CPU by the SIMT emulator: tests/spectrogram_cases.py at every
shape against torch.stft in float64 inside the derived fp32 bound, the determinism contract, the argument checks, and -- where the
reference tree is present -- the reference's own spectrogram_torch."""
import numpy as np
import pytest
import torch

from tests import spectrogram_cases as S
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("n_fft,hop,win,n", S.SHAPES)
def test_shape_within_derived_bound(ops, n_fft, hop, win, n):
    worst = S.check_shape(ops, "cpu", n_fft, hop, win, n)
    print(f"({n_fft}, {hop}, {win}, {n}): worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_strided_batch_within_bound_and_equal_to_solo_runs(ops):
    worst = S.check_batch(ops, "cpu")
    print(f"batch 3, strided: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_interior_frames_equal_those_of_a_hop_aligned_crop(ops):
    S.check_crop(ops, "cpu")


def test_result_does_not_depend_on_the_thread_order(ops, monkeypatch):
    """SVCMI_EMU_ORDER=reverse runs the fibers of every scheduling round backwards: a missing barrier after the span staging would show."""
    x = S.tone_noise(320 * 40 + 5, seed=3)[None]
    a = S.run(ops, "cpu", x, 1024, 320, 1024)
    b7 = S.run(ops, "cpu", S.tone_noise(300, seed=4)[None], 64, 7, 64)
    monkeypatch.setenv("SVCMI_EMU_ORDER", "reverse")
    assert torch.equal(S.run(ops, "cpu", x, 1024, 320, 1024), a)
    assert torch.equal(S.run(ops, "cpu", S.tone_noise(300, seed=4)[None], 64, 7, 64), b7)


def test_argument_validation(ops):
    S.check_argument_validation(ops, "cpu")


def test_basis_is_the_windowed_dft_table():
    """The table against its definition evaluated independently (float64 FFT of windowed unit impulses), and the cache."""
    from svcmi.vits.spectrogram import spectrogram_basis
    for (n_fft, win) in ((64, 64), (64, 48), (256, 100)):
        b = spectrogram_basis(n_fft, win, "cpu")
        assert b.dtype == torch.float32 and tuple(b.shape) == (n_fft, n_fft + 2) and spectrogram_basis(n_fft, win, "cpu") is b
        w = torch.zeros(n_fft, dtype=torch.float64)
        left = (n_fft - win) // 2
        w[left:left + win] = torch.hann_window(win, dtype=torch.float64)
        f = torch.fft.rfft(torch.diag(w), dim=1)                                  # row i: w[i] exp(-2 pi j k i / n_fft)
        want = torch.stack([f.real, -f.imag], dim=-1).reshape(n_fft, n_fft + 2)
        assert float((b.double() - want).abs().max()) <= 2.0 ** -24


def test_center_true_is_refused_and_short_input_raises(ops):
    from svcmi.vits.spectrogram import spectrogram_torch
    y = torch.zeros(1, 2560)
    with pytest.raises(NotImplementedError):
        spectrogram_torch(y, 1024, 32000, 320, 1024, center=True, ops=ops)
    with pytest.raises(RuntimeError):
        spectrogram_torch(torch.zeros(1, 352), 1024, 32000, 320, 1024, ops=ops)


def test_compute_spec_writes_the_reference_file(ops, tmp_path):
    from scipy.io import wavfile
    from svcmi.vits.spectrogram import compute_spec
    from workload import config as C
    hp = C.AttrDict({"data": dict(C.BASE["data"], win_length=1024, max_wav_value=32768.0)})      # configs/base.yaml: data
    n = 3 * hp.data.hop_length + 5 * hp.data.filter_length
    pcm = np.round(S.tone_noise(n, seed=8) * 32767).astype(np.int16)
    wavfile.write(str(tmp_path / "a.wav"), hp.data.sampling_rate, pcm)
    compute_spec(hp.data, str(tmp_path / "a.wav"), str(tmp_path / "a.pt"), ops=ops)
    spec = torch.load(str(tmp_path / "a.pt"))
    x = (pcm.astype(np.float32) / np.float32(hp.data.max_wav_value))[None]
    assert spec.dtype == torch.float32 and spec.device.type == "cpu"
    assert tuple(spec.shape) == (hp.data.filter_length // 2 + 1, S.frames_of(hp.data.filter_length, hp.data.hop_length, n))
    assert S.worst_ratio(spec[None], x, hp.data.filter_length, hp.data.hop_length, hp.data.win_length) <= 1.0


@pytest.mark.needs_reference
@pytest.mark.parametrize("n_fft,hop,win,n", [(1024, 320, 1024, 2560), (64, 16, 48, 200)])
def test_live_against_the_reference_spectrogram_torch(ops, n_fft, hop, win, n):
    """The reference's own function (fp32 torch.stft) is itself within the bound of the float64 oracle, so the two are within twice the
    bound of each other."""
    from oracle import ref_import
    ref_import._prepare()
    from vits import spectrogram as ref_spectrogram
    for x in S.inputs(n_fft, n):
        want = ref_spectrogram.spectrogram_torch(torch.from_numpy(x)[None], n_fft, S.SR, hop, win, center=False)
        got = S.run(ops, "cpu", x[None], n_fft, hop, win)
        _, bound = S.oracle(x[None], n_fft, hop, win)
        assert tuple(got.shape) == tuple(want.shape)
        ratio = float(((got.double() - want.double()).abs().numpy() / (2 * bound)).max())
        print(f"({n_fft}, {hop}, {win}, {n}): |ours - reference| / (2 bound) = {ratio:.3f}")
        assert ratio <= 1.0
