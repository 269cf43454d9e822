"""The speaker encoder on a real MI355X: the checks of tests/speaker_cases.py on the device, the full-size model, and wav -> .npy
through the command line in a fresh process."""
import os

import numpy as np
import pytest
import torch

from tests import speaker_cases as S
from tests.kernel_cases import _close64
from workload import speaker as WS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("H", S.STEP_H)
def test_step_kernel_shapes(ops, H):
    S.check_step_shapes(ops, "cuda", H)


def test_step_kernel_full_width(ops):
    S.check_step_shape(ops, "cuda", 2, 5, 768)


def test_step_kernel_saturation(ops):
    S.check_saturation(ops, "cuda")


def test_step_kernel_exact_cell_growth(ops):
    S.check_exact_cell_growth(ops, "cuda")


def test_step_kernel_batch_independence_and_repeatability(ops):
    S.check_batch_independence(ops, "cuda")


@pytest.mark.parametrize("B,T", [(3, 7), (17, 33)])
def test_encoder_tiny(ops, B, T):
    S.check_encoder(ops, "cuda", WS.TINY, B, T)


def test_encoder_full_dims_short(ops):
    S.check_encoder(ops, "cuda", WS.FULL, 2, 5)


def test_encoder_full_size_embedding(ops):
    """One embedding at the pretrained model's size: 10 windows x 250 frames, 750 step launches."""
    enc, sd = S.make_encoder(ops, "cuda", WS.FULL)
    x = 2.0 * torch.randn(1, 400, 80, generator=torch.Generator().manual_seed(8))
    per64, mean64 = S.embedding64(sd, x, 250, 10)
    per32, mean32 = S.embedding64(sd, x, 250, 10, torch.float32)
    _close64(enc.compute_embedding(x.cuda(), return_mean=False), per64, per32, "full-size windows")
    _close64(enc.compute_embedding(x.cuda()), mean64, mean32, "full-size embedding")


def test_compute_embedding_offsets_and_short_clip(ops):
    S.check_compute_embedding(ops, "cuda")


def test_fixture_of_the_reference_class(ops, golden_dir, tmp_path):
    S.check_golden(ops, "cuda", golden_dir, tmp_path)


@pytest.mark.parametrize("n", [1024, 4000])
def test_mel_against_float64(ops, n):
    S.check_mel(ops, "cuda", n)


def test_mel_edges(ops):
    S.check_mel_edges(ops, "cuda")


def test_preemphasis_edge(ops):
    S.check_preemphasis(ops, "cuda")


def test_trim_and_sound_norm(ops):
    S.check_trim_and_norm(ops, "cuda")


def test_cli_wav_to_npy_in_a_fresh_process(ops, tmp_path):
    """python -m svcmi.speaker.infer MODEL CONFIG -s in.wav -t out.npy against the float64 restatement of the whole chain on a 1.5 s
    synthetic clip (tiny LSTM on the real 80-band front-end); the GPU loader gives the same file; no stray model_small.pth."""
    from scipy.io import wavfile
    sd, model, config = S.write_model(tmp_path)
    pcm = S.voice_clip(1.5, seed=1)
    wav, out = str(tmp_path / "in.wav"), str(tmp_path / "out.spk.npy")
    wavfile.write(wav, 16000, pcm)
    r = S.run_cli([model, config, "-s", wav, "-t", out], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert got.dtype == np.float32 and got.shape == (20,)
    assert not os.path.exists(str(tmp_path / "model_small.pth"))
    want64, ref32 = S.chain_restated(sd, pcm, torch.float64), S.chain_restated(sd, pcm, torch.float32)
    _close64(torch.from_numpy(got), want64, ref32, "wav -> embedding through the CLI")
    out_gpu = str(tmp_path / "out_gpu.npy")
    r = S.run_cli([model, config, "-s", wav, "-t", out_gpu, "--loader", "gpu"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(out_gpu), got)              # a 16 kHz file: the GPU loader is bit-equal to the host loader


def test_folder_mode_is_the_mean_of_the_single_runs(ops, tmp_path):
    from scipy.io import wavfile
    from svcmi.speaker import infer
    sd, model, config = S.write_model(tmp_path)
    folder = tmp_path / "singer"
    folder.mkdir()
    clips = [S.voice_clip(sec, seed=k) for k, sec in enumerate((1.2, 1.5, 4.5))]       # two short clips (whole-clip windows), one with real offsets
    for k, pcm in enumerate(clips):
        wavfile.write(str(folder / f"{k:02d}.wav"), 16000, pcm)
    enc, ap = infer.load(model, config, ops=ops, device="cuda")
    singles = [infer.embed_file(enc, ap, str(folder / f"{k:02d}.wav")) for k in range(3)]
    got = infer.embed_folder(enc, ap, str(folder))
    assert got.dtype == np.float32 and got.shape == (20,)
    want64 = torch.stack([S.chain_restated(sd, pcm, torch.float64) for pcm in clips]).mean(0)
    ref32 = torch.stack([S.chain_restated(sd, pcm, torch.float32) for pcm in clips]).mean(0)
    _close64(torch.from_numpy(got), want64, ref32, "folder mode")
    mean_singles = torch.from_numpy(np.stack(singles)).double().mean(0)
    a = float((ref32.double() - want64).abs().max())
    assert float((torch.from_numpy(got).double() - mean_singles).abs().max()) <= 8 * (2.0 ** -24 + a)
    out = str(tmp_path / "singer.spk.npy")
    infer.main([model, config, "--folder", str(folder), "--mean", out])
    assert np.array_equal(np.load(out), got)


def test_wrong_architecture_flag_raises(ops, tmp_path):
    from svcmi._lib import SvcmiError
    from svcmi.speaker import infer
    _, model, config = S.write_model(tmp_path, projection=False)
    with pytest.raises(SvcmiError):
        infer.load(model, config, ops=ops, device="cuda")
