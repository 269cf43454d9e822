"""The voice-activity detector on a real MI355X: the checks of tests/vad_cases.py on the device, the post-filter's command line in a
fresh process, and ``svc_inference.main`` with ``vad_post`` set at the tiny model size."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vad_cases as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(V.GOLDEN, "silero_vad.npz")


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("W", [1, 2, 125])
def test_frontend_against_float64(ops, W):
    V.check_frontend_windows(ops, "cuda", W)


def test_frontend_edges(ops):
    V.check_frontend_edges(ops, "cuda")


def test_frontend_bits_do_not_depend_on_the_launch(ops):
    V.check_frontend_bits(ops, "cuda")


@pytest.mark.parametrize("W", [1, 2, 135])
def test_scan_against_float64(ops, W):
    V.check_scan_lengths(ops, "cuda", W)


def test_scan_ragged_batch_and_repeatability(ops):
    V.check_scan_ragged_and_repeat(ops, "cuda")


def test_scan_state_carry(ops):
    V.check_scan_state_carry(ops, "cuda")


def test_scan_saturation(ops):
    V.check_scan_saturation(ops, "cuda")


def test_scan_exact_cell_growth(ops):
    V.check_scan_exact_cell_growth(ops, "cuda")


@pytest.mark.parametrize("name", ["035", "010"])
def test_probabilities_end_to_end(ops, name):
    V.check_probs_clip(ops, "cuda", name)


def test_batched_forward_and_decimation(ops):
    V.check_batched_forward(ops, "cuda")


def test_call_keeps_the_state_between_windows(ops):
    V.check_call_keeps_state(ops, "cuda")


def test_spans_equal_the_reference(ops):
    V.check_spans(ops, "cuda")


def test_mask(ops):
    V.check_mask(ops, "cuda")


def test_apply_vad_post(ops):
    V.check_apply_vad_post(ops, "cuda")


def test_post_command_line_with_a_resident_model(ops, tmp_path):
    V.check_post_cli(ops, "cuda", tmp_path)


def test_post_command_line_in_a_fresh_process(ops, tmp_path):
    """python -m svcmi.svc_inference_post --ref 035.wav --svc <32 kHz wav> --out o.wav: zero outside [3136, 100288), untouched inside."""
    from scipy.io import wavfile
    ref, svc = V.post_inputs()
    svc_path, out_path = str(tmp_path / "svc_out.wav"), str(tmp_path / "o.wav")
    wavfile.write(svc_path, 32000, svc)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "whisper-vits-svc_amd"), ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-m", "svcmi.svc_inference_post", "--ref", os.path.join(V.GOLDEN, "035.wav"), "--svc", svc_path,
                        "--out", out_path, "--vad", FIXTURE], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rate, y = wavfile.read(out_path)
    assert rate == 32000 and y.dtype == np.float32 and y.shape == (2 * ref.shape[0] - 37,)
    assert not y[:3136].any() and not y[100288:].any() and np.array_equal(y[3136:100288], svc[3136:100288])


def test_svc_inference_main_with_vad_post(ops, tmp_path, monkeypatch):
    """svc_inference.main with ``vad_post`` set (a Namespace without the attribute keeps working: tests/test_gpu_engine.py) hands the
    waveform, still on the device, and the 16 kHz input to apply_vad_post; svc_out.wav holds that function's result."""
    import json
    import shutil
    import yaml
    from scipy.io import wavfile
    from svcmi import svc_inference as SI
    from svcmi import svc_inference_post as SP
    from workload import config as C
    from workload import inputs as I
    from workload import weights as W
    monkeypatch.chdir(tmp_path)
    hp = C.tiny_hp()
    shutil.copyfile(os.path.join(V.GOLDEN, "035.wav"), "in.wav")
    torch.save({"model_g": W.make_vits_state(hp, seed=1234)}, "svc.pth")
    torch.save(W.make_whisper_state({**C.WHISPER_TINY_TEST, "n_audio_state": hp.vits.ppg_dim, "n_audio_head": 4}), "whisper.pt")
    torch.save(W.make_hubert_state(dict(C.HUBERT_TINY_TEST, proj=hp.vits.vec_dim)), "hubert.pt")
    torch.save(W.make_crepe_state("tiny"), "crepe.pth")
    np.save("spk.npy", I.synth_spk(hp.vits.spk_dim, seed=7).numpy())
    with open("cfg.yaml", "w") as f:
        yaml.safe_dump(json.loads(json.dumps(hp)), f)
    args = SI.build_parser().parse_args(["--config", "cfg.yaml", "--model", "svc.pth", "--wave", "in.wav", "--spk", "spk.npy", "--whisper", "whisper.pt",
                                         "--hubert", "hubert.pt", "--crepe", "crepe.pth", "--vad-post", FIXTURE])
    assert args.vad_post == FIXTURE and SI.build_parser().parse_args(["--config", "c", "--model", "m", "--wave", "w", "--spk", "s"]).vad_post is None
    seen = []
    real = SP.apply_vad_post

    def spy(ref16k, svc32k, vad, threshold=0.2):
        out = real(ref16k, svc32k, vad, threshold)
        seen.append((np.asarray(ref16k), svc32k.cpu().numpy(), svc32k.is_cuda, out.cpu().numpy()))
        return out
    monkeypatch.setattr(SP, "apply_vad_post", spy)
    torch.manual_seed(0)
    out = SI.main(args)
    assert len(seen) == 1
    ref, raw, on_device, masked = seen[0]
    assert on_device and np.array_equal(ref, V.clip("035").numpy())
    n = min(raw.shape[0], 2 * ref.shape[0])
    assert out.dtype == np.float32 and out.shape == (n,) and np.array_equal(out, masked)
    assert np.array_equal(out, V.mask_ref(raw, V.fixture_spans("035", 0.2), ref.shape[0]))
    assert not out[:3136].any() and not out[100288:].any() and np.array_equal(out[3136:100288], raw[3136:100288]) and raw[:3136].any()
    rate, written = wavfile.read("svc_out.wav")
    assert rate == 32000 and np.array_equal(written, out)
