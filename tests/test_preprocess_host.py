"""The training-set preparation (svcmi.svc_preprocessing and the training recipes) where no GPU is needed: the wave normalisation
arithmetic, the file-list writer on a fake tree, the parser, the F0 post-filter against the reference's own crepe/filter.py,
compute_f0_train end to end on the SIMT emulator, and the driver's plumbing with stub networks."""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

from tests import preprocess_cases as P
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


# ------------------------------------------------------------------------------------------------ preprocess_a.py arithmetic
def wave(n, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (scale * np.sin(2 * np.pi * 211.0 * t) + 0.1 * scale * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("n,seed,scale", [(4001, 0, 0.3), (16000, 1, 0.9), (777, 2, 1e-4), (5000, 3, 3.0)])
def test_normalize_wave_int16_is_the_reference_arithmetic(n, seed, scale):
    from svcmi.svc_preprocessing import normalize_wave_int16
    x = wave(n, seed, scale)
    i16, f32 = normalize_wave_int16(torch.from_numpy(x), "x.wav")
    want = P.preprocess_a_numpy(x)
    assert i16.dtype == torch.int16 and f32.dtype == torch.float32
    assert np.array_equal(i16.numpy(), want)
    assert np.array_equal(f32.numpy(), want.astype(np.float32) / np.float32(32768.0))
    assert int(np.abs(want).max()) in (19659, 19660)            # 0.6 * 32767 = 19660.2, truncated; one step of fp32 rounding allowed below


def test_normalize_wave_int16_truncates_towards_zero():
    from svcmi.svc_preprocessing import normalize_wave_int16
    x = np.array([1.0, -1.0, 0.5, -0.5, 0.00004, -0.00004, 0.33333], dtype=np.float32)
    i16, _ = normalize_wave_int16(torch.from_numpy(x))
    assert np.array_equal(i16.numpy(), P.preprocess_a_numpy(x))
    assert i16[4] == 0 and i16[5] == 0 and i16[2] > 0 > i16[3] and int(i16[2]) == -int(i16[3])


def test_normalize_wave_int16_refuses_a_silent_clip():
    from svcmi.svc_preprocessing import normalize_wave_int16
    with pytest.raises(ValueError, match="silent.wav"):
        normalize_wave_int16(torch.zeros(100), "dataset_raw/s/silent.wav")


# ------------------------------------------------------------------------------------------------ preprocess_train.py
def fake_tree(root, singers=("a", "b"), per_singer=7):
    for s in singers:
        for kind in ("waves-32k", "specs", "pitch", "hubert", "whisper", "speaker"):
            os.makedirs(os.path.join(root, kind, s), exist_ok=True)
        os.makedirs(os.path.join(root, "singer"), exist_ok=True)
        open(os.path.join(root, "singer", f"{s}.spk.npy"), "w").close()
        for i in range(per_singer):
            for kind, ext in (("waves-32k", ".wav"), ("specs", ".pt"), ("pitch", ".pit.npy"), ("hubert", ".vec.npy"), ("whisper", ".ppg.npy"),
                              ("speaker", ".spk.npy")):
                open(os.path.join(root, kind, s, f"{i:02d}{ext}"), "w").close()


def test_file_lists_seeded_shuffle_and_missing_files(tmp_path):
    from svcmi.svc_preprocessing import collect_items, write_file_lists
    out, files = str(tmp_path / "data_svc"), str(tmp_path / "files")
    fake_tree(out)
    os.remove(os.path.join(out, "pitch", "a", "03.pit.npy"))          # an item with a missing file is left out and named
    open(os.path.join(out, "waves-32k", "a", "notes.txt"), "w").close()
    said = []
    items = collect_items(out, log=said.append)
    assert len(items) == 13 and any("pitch/a/03.pit.npy" in s for s in said) and len(said) == 1
    assert items == sorted(items)
    valid, train = write_file_lists(out, files, seed=5, log=lambda s: None)
    want = list(items)
    random.Random(5).shuffle(want)
    assert valid == sorted(want[:10]) and train == want[10:] and len(train) == 3
    assert open(os.path.join(files, "valid.txt")).read().splitlines() == valid
    assert open(os.path.join(files, "train.txt")).read().splitlines() == train
    for line in valid + train:
        parts = line.split("|")
        assert len(parts) == 6 and all(os.path.isfile(p) for p in parts)
        s, f = parts[0].split("/")[-2], os.path.basename(parts[0])[:-4]
        assert parts == [f"{out}/waves-32k/{s}/{f}.wav", f"{out}/specs/{s}/{f}.pt", f"{out}/pitch/{s}/{f}.pit.npy",
                         f"{out}/hubert/{s}/{f}.vec.npy", f"{out}/whisper/{s}/{f}.ppg.npy", f"{out}/speaker/{s}/{f}.spk.npy"]
    assert write_file_lists(out, files, seed=5, log=lambda s: None) == (valid, train)             # the seed reproduces the split
    assert write_file_lists(out, files, seed=6, log=lambda s: None) != (valid, train)


def test_file_lists_index_by_singer_and_few_items(tmp_path):
    from svcmi.svc_preprocessing import write_file_lists
    out, files = str(tmp_path / "data_svc"), str(tmp_path / "files")
    fake_tree(out, singers=("solo",), per_singer=4)
    valid, train = write_file_lists(out, files, index_by_singer=True, seed=1, log=lambda s: None)
    assert len(valid) == 4 and train == [] and open(os.path.join(files, "train.txt")).read() == ""
    assert all(line.split("|")[5] == f"{out}/singer/solo.spk.npy" for line in valid)
    os.remove(os.path.join(out, "singer", "solo.spk.npy"))
    assert write_file_lists(out, files, index_by_singer=True, seed=1, log=lambda s: None) == ([], [])


def test_singer_mean_is_the_float32_running_sum(tmp_path):
    from svcmi.svc_preprocessing import write_singer_mean
    d = tmp_path / "speaker" / "s"
    d.mkdir(parents=True)
    rng = np.random.default_rng(0)
    embeds = [rng.standard_normal(16).astype(np.float32) for _ in range(5)]
    for i, e in enumerate(embeds):
        np.save(str(d / f"{i}.spk.npy"), e)
    got = write_singer_mean(str(d), str(tmp_path / "singer" / "s.spk.npy"))
    want = ((((embeds[0] + embeds[1]) + embeds[2]) + embeds[3]) + embeds[4]) / 5
    saved = np.load(str(tmp_path / "singer" / "s.spk.npy"))
    assert saved.dtype == np.float32 and np.array_equal(saved, want) and np.array_equal(got, want)
    assert write_singer_mean(str(tmp_path / "nothing"), str(tmp_path / "singer" / "x.spk.npy")) is None


def test_parser_defaults():
    from svcmi.svc_preprocessing import build_parser
    a = build_parser().parse_args(["--config", "cfg.yaml"])
    assert (a.raw, a.out, a.files, a.loader, a.precision, a.index_by_singer, a.seed, a.stage_times) == \
        ("dataset_raw", "data_svc", "files", "host", "f32", False, None, False)
    assert a.whisper.endswith("large-v2.pt") and a.hubert.endswith("hubert-soft-0d54a1f4.pt") and a.crepe.endswith("full.pth")
    assert a.speaker_model.endswith("best_model.pth.tar") and a.speaker_config.endswith("config.json")
    b = build_parser().parse_args(["--config", "c", "--loader", "gpu", "--precision", "f16", "--index-by-singer", "--seed", "7"])
    assert (b.loader, b.precision, b.index_by_singer, b.seed) == ("gpu", "f16", True, 7)
    for bad in (["--loader", "nope"], ["--precision", "int8"], []):
        with pytest.raises(SystemExit):
            build_parser().parse_args((["--config", "c"] if bad else []) + bad)


# ------------------------------------------------------------------------------------------------ F0 post-filter, exact
def tracks(n, seed):
    """Periodicity over 0 .. 1 with ties and values exactly 0.5 (and NaNs); pitch with exact zeros and NaNs."""
    rng = np.random.default_rng(seed)
    per = rng.uniform(0.0, 1.0, n).astype(np.float32)
    per[rng.integers(0, n, max(1, n // 4))] = np.float32(0.5)
    per[::3] = per[0]                                                         # ties
    pit = rng.uniform(60.0, 900.0, n).astype(np.float32)
    pit[rng.integers(0, n, max(1, n // 5))] = 0.0
    if n > 5:
        pit[rng.integers(0, n, max(1, n // 6))] = np.nan
        per[rng.integers(0, n, max(1, n // 8))] = np.nan
        per[1], per[n - 2] = np.float32(0.0), np.float32(1.0)
    if n > 20:
        pit[10:16] = 0.0                                                      # a run of zeros: an exact-zero mean becomes NaN
        pit[30:33] = np.nan
        per[40:48] = np.nan                                                   # a window without a valid value
        per[60] = np.inf
    return pit, per


@pytest.mark.needs_reference
@pytest.mark.parametrize("n", [4, 5, 7, 8, 101])
def test_postfilter_equals_the_reference_filters_bit_for_bit(n):
    from svcmi.pitch import f0_train_postfilter
    from oracle import ref_import
    spec = importlib.util.spec_from_file_location("ref_crepe_filter", os.path.join(ref_import.REF, "crepe", "filter.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for seed in range(4):
        pit, per = tracks(n, seed)
        periodicity = ref.median(torch.from_numpy(per)[None], 7)
        pitch = ref.mean(torch.from_numpy(pit)[None], 5)
        pitch[periodicity < 0.5] = 0
        want = pitch.squeeze(0).numpy()
        got = f0_train_postfilter(pit, per)
        assert got.dtype == np.float32 and got.shape == (n,)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (n, seed)
        assert np.array_equal(got.view(np.uint32)[~np.isnan(got)], want.view(np.uint32)[~np.isnan(want)]), (n, seed)


def test_postfilter_refuses_short_tracks():
    from svcmi.pitch import f0_train_postfilter
    for n in (0, 1, 3):
        with pytest.raises(ValueError):
            f0_train_postfilter(np.ones(n, np.float32), np.ones(n, np.float32))
    with pytest.raises(ValueError):
        f0_train_postfilter(np.ones(5, np.float32), np.ones(6, np.float32))
    out = f0_train_postfilter(np.full(4, 100.0, np.float32), np.array([0.9, 0.9, 0.1, 0.1], np.float32))
    assert out.shape == (4,)


# ------------------------------------------------------------------------------------------------ recipes on the emulator
def test_compute_f0_train_against_the_oracle(ops):
    """The clip length is the one the GPU test uses (1 s + 37 samples = 101 frames at hop 160, so that the median-7 / mean-5 windows and
    the gate see a real track); emulating the tiny network over 101 frames takes several minutes on the CPU."""
    err = P.check_f0_train(ops, "cpu")
    print(f"periodicity: max |ours - oracle| = {err:.2e}")


# ------------------------------------------------------------------------------------------------ driver plumbing on the emulator
def test_driver_layout_failure_isolation_and_lists_with_stub_networks(ops, tmp_path, monkeypatch):
    """svc_preprocessing.main on the CPU: the loader, the normalisation, the spectrogram kernel (emulator), the file layout, the singer
    mean, the kept PPG file, per-file failure isolation and the lists are the real code; the four networks are stubs (they are far too
    slow to emulate at clip length and are covered on the GPU by tests/test_gpu_preprocess.py)."""
    import types
    import yaml
    from scipy.io import wavfile
    from svcmi import svc_preprocessing as SP
    from svcmi.hubert import inference as hubert_inf
    from svcmi.pitch import inference as pitch_inf
    from svcmi.speaker import infer as speaker_inf
    from svcmi.whisper import inference as whisper_inf
    from svcmi.whisper.audio import load_audio_device
    from tests import spectrogram_cases as S
    monkeypatch.setattr(whisper_inf, "load_model", lambda path, device, ops=None: types.SimpleNamespace(encoder=types.SimpleNamespace(precision=None)))
    monkeypatch.setattr(hubert_inf, "load_model", lambda path, device, ops=None: types.SimpleNamespace(precision=None))
    monkeypatch.setattr(pitch_inf, "load_crepe", lambda path, device, ops=None: types.SimpleNamespace(precision=None))
    monkeypatch.setattr(speaker_inf, "load", lambda *a, **k: (None, None))
    monkeypatch.setattr(whisper_inf, "pred_ppg_train", lambda w, a: torch.full((a.shape[0] // 320, 4), 2.0))
    monkeypatch.setattr(hubert_inf, "pred_vec_train", lambda m, a: a[: (a.shape[0] // 320) * 320].view(-1, 320)[:, :3].clone())
    monkeypatch.setattr(pitch_inf, "compute_f0_train_begin",
                        lambda a, device, model=None: (lambda dither=None: np.full(1 + a.shape[0] // 160, 220.0, np.float32)))
    monkeypatch.setattr(SP, "embed_wave", lambda enc, ap, wave, name="": np.asarray(wave[:8], dtype=np.float32) * np.float32(2))
    raw = tmp_path / "dataset_raw"
    rng = np.random.default_rng(0)
    for singer in ("a", "b"):
        (raw / singer).mkdir(parents=True)
        for i in range(2):
            n = 6615 + 441 * i                                            # 0.15 / 0.16 s at 44.1 kHz, stereo
            pcm = np.round(rng.uniform(-0.5, 0.5, (n, 2)) * 32767).astype(np.int16)
            wavfile.write(str(raw / singer / f"c{i}.wav"), 44100, pcm)
    (raw / "a" / "bad.wav").write_bytes(b"RIFF\x10\x00\x00\x00WAVEjunk")
    wavfile.write(str(raw / "b" / "silent.wav"), 44100, np.zeros((4410, 2), np.int16))
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump({"data": {"sampling_rate": 32000, "filter_length": 1024, "hop_length": 320, "win_length": 1024, "max_wav_value": 32768.0}}, f)
    out = str(tmp_path / "data_svc")
    os.makedirs(f"{out}/whisper/a")
    marker = np.zeros((2, 3), np.float32)
    np.save(f"{out}/whisper/a/c1.ppg.npy", marker)                         # already there: kept
    args = SP.build_parser().parse_args(["--raw", str(raw), "--out", out, "--files", str(tmp_path / "files"), "--config",
                                         str(tmp_path / "cfg.yaml"), "--loader", "gpu", "--seed", "3"])
    rep = SP.main(args, ops=ops, device="cpu")
    assert rep["returncode"] == 1 and rep["clips"] == 4
    assert sorted(os.path.basename(p) for p, _ in rep["failed"]) == ["bad.wav", "silent.wav"]
    assert "silent.wav" in dict((os.path.basename(p), e) for p, e in rep["failed"])["silent.wav"]
    assert np.array_equal(np.load(f"{out}/whisper/a/c1.ppg.npy"), marker)
    assert len(rep["valid"]) == 4 and rep["train"] == [] and rep["valid"] == sorted(rep["valid"])
    for line in rep["valid"]:
        assert all(os.path.isfile(p) for p in line.split("|")) and len(line.split("|")) == 6
    for s in ("a", "b"):
        for i in range(2):
            for sr in (16000, 32000):
                loaded = load_audio_device(str(raw / s / f"c{i}.wav"), sr=sr, device="cpu", ops=ops).numpy()
                rate, written = wavfile.read(f"{out}/waves-{sr // 1000}k/{s}/c{i}.wav")
                assert rate == sr and np.array_equal(written, P.preprocess_a_numpy(loaded))
            _, w16 = wavfile.read(f"{out}/waves-16k/{s}/c{i}.wav")
            _, w32 = wavfile.read(f"{out}/waves-32k/{s}/c{i}.wav")
            q16 = w16.astype(np.float32) / np.float32(32768)
            # the stubs saw the QUANTISED samples, on the device, not the loader's output
            assert np.array_equal(np.load(f"{out}/speaker/{s}/c{i}.spk.npy"), q16[:8] * np.float32(2))
            assert np.array_equal(np.load(f"{out}/hubert/{s}/c{i}.vec.npy"), q16[: (len(q16) // 320) * 320].reshape(-1, 320)[:, :3])
            assert np.load(f"{out}/pitch/{s}/c{i}.pit.npy").shape == (1 + len(q16) // 160,)
            spec = torch.load(f"{out}/specs/{s}/c{i}.pt")
            x32 = (w32.astype(np.float32) / np.float32(32768))[None]
            assert tuple(spec.shape) == (513, len(w32) // 320) and S.worst_ratio(spec[None], x32, 1024, 320, 1024) <= 1.0
        e = [np.load(f"{out}/speaker/{s}/c{i}.spk.npy") for i in range(2)]
        assert np.array_equal(np.load(f"{out}/singer/{s}.spk.npy"), (e[0] + e[1]) / 2)
    assert not os.path.exists(f"{out}/specs/b/silent.pt") and not os.path.exists(f"{out}/waves-16k/a/bad.wav")


def test_pred_vec_train_is_units_on_the_whole_clip(ops, tmp_path):
    from scipy.io import wavfile
    from svcmi.hubert import inference as hubert_inf
    from workload import config as C
    from workload import weights as W
    m = hubert_inf.load_model(W.make_hubert_state(C.HUBERT_TINY_TEST), "cpu", ops=ops)
    pcm = np.round(wave(1600, 4) * 32767).astype(np.int16)
    wavfile.write(str(tmp_path / "a.wav"), 16000, pcm)
    a = torch.from_numpy(pcm.astype(np.float32) / np.float32(32768))
    v = hubert_inf.pred_vec_train(m, a)
    assert tuple(v.shape) == ((1600 + 80 - 400) // 320 + 1, C.HUBERT_TINY_TEST["proj"]) and torch.equal(v, m.units(a.view(1, 1, -1))[0])
    assert torch.equal(hubert_inf.pred_vec_train(m, str(tmp_path / "a.wav")), v) and torch.equal(hubert_inf.pred_vec_train(m, a.numpy()), v)


def test_pred_ppg_train_pads_or_trims_to_30_s_and_keeps_n_over_320_rows(monkeypatch):
    """The recipe's own arithmetic with a stub front-end and encoder: 480000 samples go in whatever the clip length, no mel noise,
    rows [: n // 320] come out (at most the 1500 of one window, like the reference)."""
    import types
    from svcmi.whisper import audio as A
    from svcmi.whisper import inference as whisper_inf
    seen = []

    def fake_mel(wav, ops=None, device=None):
        seen.append((tuple(wav.shape), float(wav.abs().sum())))
        return torch.zeros(80, wav.shape[0] // 160)

    def fake_encoder(mel, noise, *a):
        assert tuple(mel.shape) == (1, 80, 3000) and noise is None
        return torch.arange(1500.0)[None, :, None].repeat(1, 1, 2)
    monkeypatch.setattr(A, "log_mel_spectrogram", fake_mel)
    w = types.SimpleNamespace(device=torch.device("cpu"), ops=None, encoder=fake_encoder)
    short = torch.ones(16037)
    out = whisper_inf.pred_ppg_train(w, short)
    assert tuple(out.shape) == (50, 2) and float(out[-1, 0]) == 49.0 and seen[-1] == ((480000,), 16037.0)
    out = whisper_inf.pred_ppg_train(w, np.ones(500000, np.float32))
    assert tuple(out.shape) == (1500, 2) and seen[-1] == ((480000,), 480000.0)
