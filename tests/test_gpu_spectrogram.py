"""The fused linear spectrogram on a real MI355X: the checks of tests/spectrogram_cases.py on the device, one full-size clip, the
determinism contract (crop, batch, side stream) and the argument checks."""
import pytest
import torch

from tests import spectrogram_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("n_fft,hop,win,n", S.SHAPES)
def test_shape_within_derived_bound(ops, n_fft, hop, win, n):
    worst = S.check_shape(ops, "cuda", n_fft, hop, win, n)
    print(f"({n_fft}, {hop}, {win}, {n}): worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_strided_batch_within_bound_and_equal_to_solo_runs(ops):
    worst = S.check_batch(ops, "cuda")
    print(f"batch 3, strided: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_full_size_clip_and_side_stream(ops):
    """10 s at 32 kHz -> [513, 1000]: every element inside the bound, frames == n // hop, and the same bits from a side stream."""
    n_fft, hop, win, n = S.FULL
    x = S.tone_noise(n, seed=21)[None]
    xd = torch.from_numpy(x).cuda()
    out = S.run(ops, "cuda", xd, n_fft, hop, win)
    assert tuple(out.shape) == (1, 513, 1000) and out.shape[2] == n // hop
    worst = S.worst_ratio(out, x, n_fft, hop, win)
    print(f"{S.FULL}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = S.run(ops, "cuda", xd, n_fft, hop, win)
    side.synchronize()
    assert torch.equal(again, out)


def test_interior_frames_equal_those_of_a_hop_aligned_crop(ops):
    S.check_crop(ops, "cuda")


def test_argument_validation(ops):
    S.check_argument_validation(ops, "cuda")


def test_host_tensor_goes_to_the_gpu(ops):
    from svcmi.vits.spectrogram import spectrogram_torch
    x = torch.from_numpy(S.tone_noise(2560, seed=2))[None]
    out = spectrogram_torch(x, 1024, S.SR, 320, 1024)
    assert out.is_cuda and tuple(out.shape) == (1, 513, 8)
    assert torch.equal(out, S.run(ops, "cuda", x.cuda(), 1024, 320, 1024))
