"""The command line of the key sweep (svcmi.svc_inference_shift, the reference's svc_inference_shift.py) run in process on the emulator
device, features from files: file names, printed lines, the range assertions, and each file equal to svc_infer_sweep for its key."""
import json
import os

import numpy as np
import pytest
import torch

from tests.emu import emu_ops
from workload import config as C
from workload import inputs as I
from workload import weights as W

T50 = 3          # feature frames at 50 fps -> 6 synthesizer frames


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


def _files(hp):
    import yaml
    g = torch.Generator().manual_seed(21)
    torch.save({"model_g": W.make_vits_state(hp, seed=1234)}, "svc.pth")
    np.save("spk.npy", I.synth_spk(hp.vits.spk_dim, seed=7).numpy())
    np.save("in.ppg.npy", torch.randn(T50, hp.vits.ppg_dim, generator=g).numpy())
    np.save("in.vec.npy", torch.randn(T50, hp.vits.vec_dim, generator=g).numpy())
    with open("in.pit.csv", "w") as f:
        for i, v in enumerate((0, 187, 233, 96, 523, 441, 30)):          # one frame more than the features: trimmed like svc_infer does
            f.write(f"{i * 0.01:.2f},{v}\n")
    with open("cfg.yaml", "w") as f:
        yaml.safe_dump(json.loads(json.dumps(hp)), f)
    return ["--config", "cfg.yaml", "--model", "svc.pth", "--wave", "in.wav", "--spk", "spk.npy", "--ppg", "in.ppg.npy", "--vec", "in.vec.npy",
            "--pit", "in.pit.csv"]


def test_parser_has_the_reference_flags_and_the_engine_flags():
    from svcmi import svc_inference_shift as SS
    a = SS.build_parser().parse_args(["--config", "c", "--model", "m", "--wave", "w", "--spk", "s"])
    assert (a.shift_l, a.shift_r, a.ppg, a.vec, a.pit) == (0, 0, None, None, None)
    assert (a.f0, a.swipe_threshold, a.loader, a.precision, a.f0_precision, a.key_batch) == ("crepe", 0.0, "host", "f32", "f32", 16)
    assert a.enable_retrieval is False and a.retrieval_ratio == 0.5 and a.n_retrieval_vectors == 3
    assert a.whisper.endswith("large-v2.pt") and a.hubert.endswith("hubert-soft-0d54a1f4.pt") and a.crepe.endswith("full.pth")
    assert not hasattr(a, "shift") and not hasattr(a, "vad_post")
    with pytest.raises(SystemExit):
        SS.build_parser().parse_args(["--config", "c", "--model", "m", "--wave", "w", "--spk", "s", "--f0", "nope"])


@pytest.mark.parametrize("l,r", [(-13, 0), (0, -13), (13, 13), (0, 13), (3, 2)])
def test_range_assertions_fire(ops, tmp_path, monkeypatch, l, r):
    from svcmi import svc_inference_shift as SS
    monkeypatch.chdir(tmp_path)
    args = SS.build_parser().parse_args(["--config", "c", "--model", "m", "--wave", "w", "--spk", "s", "--shift_l", str(l), "--shift_r", str(r)])
    with pytest.raises(AssertionError):
        SS.main(args, device="cpu", ops=ops)
    assert not os.path.exists("_svc_out")              # refused before anything is made


def test_cli_writes_one_file_per_key(ops, tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    from svcmi import svc_inference as SI
    from svcmi import svc_inference_shift as SS
    from svcmi.pitch import load_csv_pitch
    from tests import engine_cases as E
    monkeypatch.chdir(tmp_path)
    hp = C.tiny_hp()
    argv = _files(hp)
    args = SS.build_parser().parse_args(argv + ["--shift_l", "-1", "--shift_r", "1"])
    torch.manual_seed(0)
    outs = SS.main(args, device="cpu", ops=ops)
    printed = capsys.readouterr().out.splitlines()
    assert printed[-4:] == ["pitch shift: [-1, 1]", "-1", "0", "1"]
    assert sorted(os.listdir("_svc_out")) == ["svc_out_-1.wav", "svc_out_0.wav", "svc_out_1.wav"]
    assert not os.path.exists("svc_out_pit.wav") and not os.path.exists("svc_out.wav")
    # the same keys through svc_infer_sweep by hand, with the same seed
    m, _ = E.make_model(hp, ops, "cpu")
    pit = load_csv_pitch("in.pit.csv")
    assert all(isinstance(v, int) for v in pit)
    ppg = torch.FloatTensor(np.repeat(np.load("in.ppg.npy"), 2, 0))
    vec = torch.FloatTensor(np.repeat(np.load("in.vec.npy"), 2, 0))
    torch.manual_seed(0)
    want = SI.svc_infer_sweep(m, None, torch.FloatTensor(np.load("spk.npy")), torch.FloatTensor(np.array(pit)), ppg, vec, hp, "cpu", [-1, 0, 1])
    n = 2 * T50 * hp.data.hop_length - 1
    for s, w in zip((-1, 0, 1), want):
        sr, written = wavfile.read(f"_svc_out/svc_out_{s}.wav")
        assert sr == hp.data.sampling_rate and written.dtype == np.float32 and written.shape == (n,)
        assert np.array_equal(written, w) and np.array_equal(outs[s], w)
    assert not np.array_equal(want[0], want[2])
