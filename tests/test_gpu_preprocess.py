"""The training-set preparation on a real MI355X with tiny seeded models: the training recipes, and svcmi.svc_preprocessing on a raw
folder of 2 singers x 3 clips (44.1 kHz stereo int16) plus one corrupt file, with ``--loader gpu``."""
import json
import os

import numpy as np
import pytest
import torch

from tests import preprocess_cases as P
from tests import speaker_cases as SC
from workload import config as C
from workload import weights as W

pytestmark = pytest.mark.gpu

SEED = 77
SPEAKER_DIMS = dict(input_dim=80, proj_dim=256, lstm_dim=40, num_lstm_layers=3)
DATA = {"sampling_rate": 32000, "filter_length": 1024, "hop_length": 320, "win_length": 1024, "max_wav_value": 32768.0}
SECONDS = {"alto": (0.7, 1.0, 1.3), "bass": (0.9, 1.1, 0.8)}


def song(seconds, rate, seed):
    """A stereo int16 'song': two detuned, vibrato tones plus noise, different in the two channels."""
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * rate)) / rate
    left = 0.4 * np.sin(2 * np.pi * (220 + 30 * np.sin(2 * np.pi * 1.5 * t)) * t) + 0.02 * rng.standard_normal(t.shape[0])
    right = 0.3 * np.sin(2 * np.pi * (331 + 20 * np.sin(2 * np.pi * 2.0 * t)) * t) + 0.02 * rng.standard_normal(t.shape[0])
    return np.round(np.stack([left, right], axis=1) * 32767).astype(np.int16)


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


def test_compute_f0_train_against_the_oracle(ops):
    err = P.check_f0_train(ops, "cuda")
    print(f"periodicity: max |ours - oracle| = {err:.2e}")


@pytest.fixture(scope="module")
def run(ops, tmp_path_factory):
    """The driver once on the raw folder; the tests below read what it wrote."""
    import yaml
    from scipy.io import wavfile
    from svcmi import svc_preprocessing as SP
    root = tmp_path_factory.mktemp("prep")
    raw = root / "dataset_raw"
    for si, (singer, secs) in enumerate(SECONDS.items()):
        (raw / singer).mkdir(parents=True)
        for i, s in enumerate(secs):
            wavfile.write(str(raw / singer / f"clip{i}.wav"), 44100, song(s, 44100, seed=100 + 10 * si + i))
    (raw / "alto" / "broken.wav").write_bytes(b"RIFF\x10\x00\x00\x00WAVEjunk, not a wav file")
    (raw / "alto" / "readme.txt").write_text("not audio")
    torch.save(W.make_whisper_state(C.WHISPER_TINY_TEST), str(root / "whisper.pt"))
    torch.save(W.make_hubert_state(C.HUBERT_TINY_TEST), str(root / "hubert.pt"))
    torch.save(P.crepe_state_with_gate(), str(root / "crepe.pth"))
    _, spk_model, spk_config = SC.write_model(root, dims=SPEAKER_DIMS)
    with open(root / "cfg.yaml", "w") as f:
        yaml.safe_dump({"data": DATA}, f)
    argv = ["--raw", str(raw), "--out", str(root / "data_svc"), "--files", str(root / "files"), "--config", str(root / "cfg.yaml"),
            "--whisper", str(root / "whisper.pt"), "--hubert", str(root / "hubert.pt"), "--crepe", str(root / "crepe.pth"),
            "--speaker-model", spk_model, "--speaker-config", spk_config, "--loader", "gpu", "--seed", str(SEED)]
    args = SP.build_parser().parse_args(argv)
    report = SP.main(args, ops=ops)
    torch.cuda.synchronize()
    return {"root": root, "raw": raw, "out": str(root / "data_svc"), "files": str(root / "files"), "args": args, "report": report,
            "spk": (spk_model, spk_config)}


def clips():
    return [(s, f"clip{i}") for s in sorted(SECONDS) for i in range(3)]


def test_corrupt_file_is_reported_and_the_rest_is_complete(run):
    rep = run["report"]
    assert rep["returncode"] != 0 and rep["clips"] == 6
    assert [p for p, _ in rep["failed"]] == [str(run["raw"] / "alto" / "broken.wav")] and rep["failed"][0][1]
    for kind in ("waves-16k", "waves-32k", "pitch", "whisper", "hubert", "speaker", "specs"):
        for s in SECONDS:
            assert sorted(os.listdir(os.path.join(run["out"], kind, s))) == sorted(
                f"clip{i}" + {"waves-16k": ".wav", "waves-32k": ".wav", "pitch": ".pit.npy", "whisper": ".ppg.npy", "hubert": ".vec.npy",
                              "speaker": ".spk.npy", "specs": ".pt"}[kind] for i in range(3)), (kind, s)
    assert sorted(os.listdir(os.path.join(run["out"], "singer"))) == ["alto.spk.npy", "bass.spk.npy"]


def test_layout_dtypes_and_shapes(run):
    from scipy.io import wavfile
    out = run["out"]
    for s, f in clips():
        r16, w16 = wavfile.read(f"{out}/waves-16k/{s}/{f}.wav")
        r32, w32 = wavfile.read(f"{out}/waves-32k/{s}/{f}.wav")
        assert (r16, r32) == (16000, 32000) and w16.dtype == w32.dtype == np.int16 and w16.ndim == w32.ndim == 1
        n16, n32 = w16.shape[0], w32.shape[0]
        ppg, vec, pit = np.load(f"{out}/whisper/{s}/{f}.ppg.npy"), np.load(f"{out}/hubert/{s}/{f}.vec.npy"), np.load(f"{out}/pitch/{s}/{f}.pit.npy")
        spk, spec = np.load(f"{out}/speaker/{s}/{f}.spk.npy"), torch.load(f"{out}/specs/{s}/{f}.pt")
        assert ppg.dtype == np.float32 and ppg.shape == (n16 // 320, C.WHISPER_TINY_TEST["n_audio_state"])
        assert vec.dtype == np.float32 and vec.shape == ((n16 + 80 - 400) // 320 + 1, C.HUBERT_TINY_TEST["proj"])
        assert pit.dtype == np.float32 and pit.shape == (1 + n16 // 160,)
        assert spec.dtype == torch.float32 and spec.device.type == "cpu" and tuple(spec.shape) == (513, n32 // 320)
        assert spk.dtype == np.float32 and spk.shape == (256,)
        assert np.isfinite(ppg).all() and np.isfinite(vec).all() and np.isfinite(spk).all() and bool(torch.isfinite(spec).all())
    for s in SECONDS:
        mean = np.load(f"{out}/singer/{s}.spk.npy")
        e = [np.load(f"{out}/speaker/{s}/clip{i}.spk.npy") for i in range(3)]
        assert mean.dtype == np.float32 and np.array_equal(mean, ((e[0] + e[1]) + e[2]) / 3)


def test_written_waves_are_preprocess_a_on_the_loaders_output(run, ops):
    from scipy.io import wavfile
    from svcmi.whisper.audio import load_audio_device
    for s, f in clips():
        for sr in (16000, 32000):
            loaded = load_audio_device(str(run["raw"] / s / f"{f}.wav"), sr=sr, ops=ops).cpu().numpy()
            _, written = wavfile.read(f"{run['out']}/waves-{sr // 1000}k/{s}/{f}.wav")
            assert np.array_equal(written, P.preprocess_a_numpy(loaded)), (s, f, sr)


def test_features_are_those_of_the_reread_waves(run, ops):
    """Every artefact is bit-equal to the single-function call made on the RE-READ written wav: the features come from the quantised
    samples.  The F0 file under pinned draws: the driver seeds both generators with --seed and draws clip by clip in sorted order."""
    from svcmi.hubert import inference as hubert_inf
    from svcmi.pitch import compute_f0_train, load_crepe
    from svcmi.speaker import infer as speaker_inf
    from svcmi.vits.spectrogram import compute_spec
    from svcmi.whisper import inference as whisper_inf
    root, out = run["root"], run["out"]
    whisper = whisper_inf.load_model(str(root / "whisper.pt"), "cuda", ops=ops)
    hubert = hubert_inf.load_model(str(root / "hubert.pt"), "cuda", ops=ops)
    crepe = load_crepe(str(root / "crepe.pth"), "cuda", ops=ops)
    enc, ap = speaker_inf.load(*run["spk"], ops=ops, device="cuda")
    hps = C.AttrDict(DATA)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    for s, f in clips():
        w16 = f"{out}/waves-16k/{s}/{f}.wav"
        f0 = compute_f0_train(w16, "cuda", model=crepe)
        assert np.array_equal(np.load(f"{out}/pitch/{s}/{f}.pit.npy"), f0, equal_nan=True), (s, f)
        assert np.array_equal(np.load(f"{out}/whisper/{s}/{f}.ppg.npy"), whisper_inf.pred_ppg_train(whisper, w16).cpu().numpy()), (s, f)
        assert np.array_equal(np.load(f"{out}/hubert/{s}/{f}.vec.npy"), hubert_inf.pred_vec_train(hubert, w16).cpu().numpy()), (s, f)
        assert np.array_equal(np.load(f"{out}/speaker/{s}/{f}.spk.npy"), speaker_inf.embed_file(enc, ap, w16)), (s, f)
        compute_spec(hps, f"{out}/waves-32k/{s}/{f}.wav", str(root / "again.pt"), ops=ops)
        assert torch.equal(torch.load(f"{out}/specs/{s}/{f}.pt"), torch.load(str(root / "again.pt"))), (s, f)


def test_file_lists(run):
    out = run["out"]
    valid = open(os.path.join(run["files"], "valid.txt")).read().splitlines()
    train = open(os.path.join(run["files"], "train.txt")).read().splitlines()
    assert train == [] and len(valid) == 6 and valid == sorted(valid) and valid == run["report"]["valid"]
    for line, (s, f) in zip(valid, clips()):
        parts = line.split("|")
        assert parts == [f"{out}/waves-32k/{s}/{f}.wav", f"{out}/specs/{s}/{f}.pt", f"{out}/pitch/{s}/{f}.pit.npy",
                         f"{out}/hubert/{s}/{f}.vec.npy", f"{out}/whisper/{s}/{f}.ppg.npy", f"{out}/speaker/{s}/{f}.spk.npy"]
        assert all(os.path.isfile(p) for p in parts)


def test_existing_ppg_is_kept_and_silent_clip_is_named(run, ops, tmp_path):
    """A pass of its own over one clip and one all-zero clip: a PPG file that is already there is not rewritten
    (preprocess_ppg.py:69-70); the silent clip fails with its name, the other clip is complete and listed."""
    import copy
    import shutil
    from scipy.io import wavfile
    from svcmi import svc_preprocessing as SP
    raw, out = tmp_path / "dataset_raw", str(tmp_path / "data_svc")
    (raw / "bass").mkdir(parents=True)
    shutil.copy(str(run["raw"] / "bass" / "clip0.wav"), str(raw / "bass" / "clip0.wav"))
    wavfile.write(str(raw / "bass" / "silent.wav"), 44100, np.zeros((30000, 2), np.int16))
    os.makedirs(f"{out}/whisper/bass")
    marker = np.zeros((2, 3), np.float32)
    np.save(f"{out}/whisper/bass/clip0.ppg.npy", marker)
    args = copy.copy(run["args"])
    args.raw, args.out, args.files = str(raw), out, str(tmp_path / "files")
    rep = SP.main(args, ops=ops)
    assert np.array_equal(np.load(f"{out}/whisper/bass/clip0.ppg.npy"), marker)
    assert [os.path.basename(p) for p, _ in rep["failed"]] == ["silent.wav"] and "silent.wav" in rep["failed"][0][1]
    assert rep["clips"] == 1 and rep["returncode"] != 0 and len(rep["valid"]) == 1 and "clip0" in rep["valid"][0]
    assert json.dumps(rep["failed"])                                                # plain (path, error) strings
    assert np.array_equal(np.load(f"{out}/hubert/bass/clip0.vec.npy"), np.load(f"{run['out']}/hubert/bass/clip0.vec.npy"))
