"""The checkpoint-scoring kernels on a real MI355X: the checks of tests/spectral_loss_cases.py on the device, one full-size item (10 s at
32 kHz through the mel and the four configured resolutions), the determinism contract (batch, side stream) and the argument checks."""
import numpy as np
import pytest
import torch

from tests import spectral_loss_cases as L
from tests import spectrogram_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("n_fft,hop,win,n", L.SHAPES)
def test_distance_sums_against_float64(ops, n_fft, hop, win, n):
    worst = L.check_shape(ops, "cuda", n_fft, hop, win, n)
    print(f"({n_fft}, {hop}, {win}, {n}): worst relative error of the three sums = {worst:.3e}")
    assert worst <= L.TOL


def test_distance_of_a_signal_to_itself_is_exactly_zero(ops):
    L.check_self_distance(ops, "cuda")


def test_strided_batch_equals_solo_runs_and_swaps_with_its_items(ops):
    worst = L.check_batch(ops, "cuda")
    print(f"batch 3, strided: worst relative error = {worst:.3e}")
    assert worst <= L.TOL
    assert L.check_batch(ops, "cuda", *L.GLOBAL_SMALL) <= L.TOL                        # the global-memory span too


@pytest.mark.parametrize("shape", L.ABS_COUNTS)
def test_abs_diff_sum_against_float64(ops, shape):
    worst = L.check_abs_diff(ops, "cuda", shape)
    print(f"{shape}: worst relative error = {worst:.3e}")
    assert worst <= L.TOL


@pytest.mark.parametrize("n_fft,hop,win,n_mel,fmin,fmax,n", L.MEL_SHAPES)
def test_log_mel_within_derived_bound(ops, n_fft, hop, win, n_mel, fmin, fmax, n):
    worst = L.check_mel(ops, "cuda", n_fft, hop, win, n_mel, fmin, fmax, n)
    print(f"mel ({n_fft}, {hop}, {win}) x {n_mel}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_full_size_item_and_side_stream(ops):
    """10 s at 32 kHz: the mel inside its bound, the mel L1 and the three sums of each configured resolution within 1e-5 of float64, and
    the same bits from a launch on a side stream."""
    from svcmi.vits_extend.stft import TacotronSTFT
    n = L.FULL_N
    x, y = L.pair(n)
    xd, yd = torch.from_numpy(np.array(x))[None].cuda(), torch.from_numpy(np.array(y))[None].cuda()
    n_fft, hop, win, n_mel, fmin, fmax, _ = L.MEL_SHAPES[0]
    stft = TacotronSTFT(n_fft, hop, win, n_mel, S.SR, fmin, fmax, device="cuda", ops=ops)
    mel_x, mel_y = stft.mel_spectrogram(xd), stft.mel_spectrogram(yd)
    l1 = ops.abs_diff_sum(mel_x, mel_y)
    sums = [ops.stft_distance(xd, yd, _basis(r, "cuda"), r[0], r[1]) for r in L.RESOLUTIONS]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = [ops.stft_distance(xd, yd, _basis(r, "cuda"), r[0], r[1]) for r in L.RESOLUTIONS]
        l1_again = ops.abs_diff_sum(mel_x, mel_y)
    side.synchronize()
    torch.cuda.synchronize()
    for r, a, b in zip(L.RESOLUTIONS, sums, again):
        assert torch.equal(a, b), r
        worst = float(L.rel_errors(a.cpu().numpy(), L.oracle_sums(x[None], y[None], *r)).max())
        print(f"{r} x {n}: worst relative error of the three sums = {worst:.3e}")
        assert worst <= L.TOL, r
    assert torch.equal(l1, l1_again)
    assert tuple(mel_y.shape) == (1, n_mel, n // hop)
    ref_x, bound_x, _ = L.mel_oracle(np.array(x)[None], n_fft, hop, win, n_mel, fmin, fmax)
    ref_y, bound_y, _ = L.mel_oracle(np.array(y)[None], n_fft, hop, win, n_mel, fmin, fmax)
    ratio = max(float((np.abs(mel_x.cpu().numpy() - ref_x) / bound_x).max()), float((np.abs(mel_y.cpu().numpy() - ref_y) / bound_y).max()))
    print(f"mel x {n}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # the kernel owes the sum over the device's OWN mels; against the float64 mels that sum moves by at most the two bounds' sums
    own = float(np.abs(mel_x.cpu().numpy().astype(np.float64) - mel_y.cpu().numpy().astype(np.float64)).sum())
    want_l1, slack = float(np.abs(ref_x - ref_y).sum()), float(bound_x.sum() + bound_y.sum())
    print(f"mel L1 sum {float(l1[0]):.6f}: relative error {abs(float(l1[0]) - own) / own:.3e} (float64 mels: {want_l1:.6f} +- {slack:.6f})")
    assert abs(float(l1[0]) - own) <= L.TOL * own and abs(float(l1[0]) - want_l1) <= slack + L.TOL * own


def _basis(resolution, device):
    from svcmi.vits.spectrogram import spectrogram_basis
    return spectrogram_basis(resolution[0], resolution[2], device)


def test_argument_validation(ops):
    L.check_argument_validation(ops, "cuda")


def test_host_tensors_go_to_the_gpu(ops):
    from svcmi.vits_extend.stft_loss import MultiResolutionSTFTLoss
    x, y = L.pair(1500)
    xh, yh = torch.from_numpy(np.array(x))[None], torch.from_numpy(np.array(y))[None]
    sc, mag = MultiResolutionSTFTLoss("cuda", [(512, 50, 240)])(xh, yh)
    assert sc.is_cuda and mag.is_cuda
    want = L.oracle_sums(x[None], y[None], 512, 50, 240)[0]
    assert abs(float(sc) - np.sqrt(want[0] / want[1])) <= L.TOL * np.sqrt(want[0] / want[1])
    assert abs(float(mag) - want[2] / (257 * 31)) <= L.TOL * want[2] / (257 * 31)
