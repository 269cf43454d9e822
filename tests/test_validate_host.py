"""svcmi.svc_validate on the CPU emulator: a tiny seeded config and checkpoints (workload/), three items in a temp dir -- one scored, one with
a missing file, one too short.  The report's numbers against the float64 oracle applied to the engine's own waveforms, the skipped items
listed, the same seed -> a byte-identical report, a stable ranking of two checkpoints, and the exit status of an empty list."""
import json

import numpy as np
import pytest
import torch
import yaml

from tests import spectral_loss_cases as L
from tests.emu import emu_ops
from workload import config as C, weights as W

FRAMES = 6                                          # 6 x 320 = 1920 samples: above the 512 of the largest resolution's padding
RESOLUTIONS = "[(1024, 120, 600), (64, 16, 48)]"    # a string, as configs/base.yaml holds it
MEL = dict(win_length=1024, mel_channels=20, mel_fmin=50.0, mel_fmax=16000.0, max_wav_value=32768.0)


def _hp_dict():
    hp = C.tiny_hp()
    return {"data": dict(hp["data"], **MEL), "vits": dict(hp["vits"]), "gen": dict(hp["gen"]), "mrd": {"resolutions": RESOLUTIONS}}


def _write_item(root, name, frames, hp, seed, n_wav=None):
    """One item as svc_preprocessing leaves it: 32 kHz int16 wav, pitch at 100 fps, hubert / whisper at 50 fps (two rows more), speaker."""
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    n = frames * 320 if n_wav is None else n_wav
    wav = np.round(L.recipe(n + 640, 220.0, seed)[-n:] * 20000).astype(np.int16)          # the recipe's second half: no silent quarter here
    paths = {k: str(root / f"{name}.{k}.npy") for k in ("pitch", "hubert", "whisper", "spk")}
    paths["wave"], paths["spec"] = str(root / f"{name}.wav"), str(root / f"{name}.spec.pt")
    wavfile.write(paths["wave"], 32000, wav)
    np.save(paths["pitch"], (200.0 + 20.0 * rng.standard_normal(frames)).astype(np.float32))            # the shortest of the three: len_min = frames
    np.save(paths["hubert"], rng.standard_normal((frames // 2 + 2, hp["vits"]["vec_dim"])).astype(np.float32))
    np.save(paths["whisper"], rng.standard_normal((frames // 2 + 2, hp["vits"]["ppg_dim"])).astype(np.float32))
    np.save(paths["spk"], (rng.standard_normal(hp["vits"]["spk_dim"]) * 0.05).astype(np.float32))
    return "|".join(paths[k] for k in ("wave", "spec", "pitch", "hubert", "whisper", "spk"))


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    root = tmp_path_factory.mktemp("validate")
    hp = _hp_dict()
    (root / "cfg.yaml").write_text(yaml.safe_dump(hp))
    lines = [_write_item(root, "good", FRAMES, hp, 1), _write_item(root, "gone", FRAMES, hp, 2), _write_item(root, "short", 1, hp, 3)]
    (root / "gone.pitch.npy").unlink()
    (root / "valid.txt").write_text("\n".join(lines) + "\n")
    (root / "empty.txt").write_text("")
    sd = W.make_vits_state(C.AttrDict(hp), seed=1234)
    torch.save({"model_g": sd}, str(root / "a.pth"))
    worse = dict(sd)
    g = torch.Generator().manual_seed(5)
    decoder = [k for k in sd if k.startswith("dec.") and sd[k].is_floating_point()]
    assert decoder
    for k in decoder:
        worse[k] = sd[k] + 0.05 * sd[k].abs().mean() * torch.randn(sd[k].shape, generator=g)
    torch.save({"model_g": worse}, str(root / "b.pth"))
    return root


@pytest.fixture(scope="module")
def reports(ops, setup):
    """The CLI run twice on both checkpoints with the same seed; (status, text) each."""
    from svcmi import svc_validate as V
    out = []
    for i in range(2):
        dst = setup / f"report{i}.json"
        rc = V.main(["--config", str(setup / "cfg.yaml"), "--model", str(setup / "a.pth"), str(setup / "b.pth"), "--files", str(setup / "valid.txt"),
                     "--out", str(dst), "--seed", "77"], ops=ops, device="cpu")
        out.append((rc, dst.read_text()))
    return out


def test_same_seed_gives_a_byte_identical_report_and_a_stable_ranking(reports, setup):
    (rc0, t0), (rc1, t1) = reports
    assert rc0 == 0 and rc1 == 0 and t0 == t1
    rep = json.loads(t0)
    assert sorted(rep["ranking"]) == sorted([str(setup / "a.pth"), str(setup / "b.pth")])
    means = {c["model"]: c["mean"]["mel_l1"] for c in rep["checkpoints"]}
    assert means[rep["ranking"][0]] <= means[rep["ranking"][1]] and means[str(setup / "a.pth")] != means[str(setup / "b.pth")]
    for c in rep["checkpoints"]:
        assert len(c["items"]) == 1 and c["items"][0]["line"] == 1 and c["items"][0]["frames"] == FRAMES
        assert c["mean"] == {k: c["items"][0][k] for k in ("mel_l1", "sc", "mag")}


def test_skipped_items_are_listed(reports, setup):
    rep = json.loads(reports[0][1])
    assert [(s["line"], s["wave"]) for s in rep["skipped"]] == [(2, str(setup / "gone.wav")), (3, str(setup / "short.wav"))]
    assert "missing pitch" in rep["skipped"][0]["reason"] and "too short" in rep["skipped"][1]["reason"]


def test_numbers_equal_the_float64_oracle_on_the_engines_own_waveforms(ops, setup, reports):
    from svcmi import svc_validate as V
    from svcmi.svc_inference import load_config, load_svc_model
    from svcmi.vits.models import SynthesizerInfer
    hp = load_config(str(setup / "cfg.yaml"))
    model = SynthesizerInfer(hp.data.filter_length // 2 + 1, hp.data.segment_size // hp.data.hop_length, hp, ops=ops)
    load_svc_model(str(setup / "a.pth"), model)
    model.eval()
    model.to("cpu")
    waves = {}
    res = V.validate(model, V.read_items(str(setup / "valid.txt")), hp, "cpu", 77, ops=ops, keep_waves=waves)
    rec = res["items"][0]
    assert rec == json.loads(reports[0][1])["checkpoints"][0]["items"][0]                  # validate() is what the CLI ran
    fake, real = (w.numpy()[None] for w in waves[1])
    assert fake.shape == real.shape == (1, FRAMES * 320 - 1) and rec["samples"] == FRAMES * 320 - 1
    want_sc = want_mag = 0.0
    res_list = V.resolutions_of(hp)
    assert res_list == [(1024, 120, 600), (64, 16, 48)]
    for n_fft, hop, win in res_list:
        s = L.oracle_sums(fake, real, n_fft, hop, win)[0]
        want_sc += np.sqrt(s[0]) / np.sqrt(s[1]) / len(res_list)
        want_mag += s[2] / ((n_fft // 2 + 1) * (1 + fake.shape[1] // hop)) / len(res_list)
    assert abs(rec["sc"] - want_sc) <= L.TOL * want_sc and abs(rec["mag"] - want_mag) <= L.TOL * want_mag
    d = hp.data
    args = (d.filter_length, d.hop_length, d.win_length, d.mel_channels, d.mel_fmin, d.mel_fmax)
    ref_x, bound_x, _ = L.mel_oracle(fake, *args)
    ref_y, bound_y, _ = L.mel_oracle(real, *args)
    want_l1, slack = float(np.abs(ref_x - ref_y).mean()), float((bound_x + bound_y).mean())      # each mel inside its bound, then the 1e-5 of the sum
    assert abs(rec["mel_l1"] - want_l1) <= slack + L.TOL * want_l1


def test_an_empty_list_gives_a_non_zero_exit_status(ops, setup):
    from svcmi import svc_validate as V
    dst = setup / "none.json"
    rc = V.main(["--config", str(setup / "cfg.yaml"), "--model", str(setup / "a.pth"), "--files", str(setup / "empty.txt"), "--out", str(dst)],
                ops=ops, device="cpu")
    rep = json.loads(dst.read_text())
    assert rc == 1 and rep["checkpoints"][0]["mean"] is None and rep["checkpoints"][0]["items"] == []
