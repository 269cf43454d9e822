"""The GPU wav loader on a real MI355X: the checks of tests/resample_cases.py on the device, one full-size clip, the loader against
the host loader, stream independence, and the device tensor through the three extractors."""
import numpy as np
import pytest
import torch

from workload import config as C
from workload import weights as W
from tests import engine_cases as E          # noqa: F401  (the tiny seeded models below are built the way its checks build them)
from tests import resample_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


def song(seconds, rate, seed):
    """A stereo int16 'song': two detuned, vibrato tones plus noise, different in the two channels."""
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * rate)) / rate
    left = 0.4 * np.sin(2 * np.pi * (220 + 30 * np.sin(2 * np.pi * 1.5 * t)) * t) + 0.02 * rng.standard_normal(t.shape[0])
    right = 0.3 * np.sin(2 * np.pi * (331 + 20 * np.sin(2 * np.pi * 2.0 * t)) * t) + 0.02 * rng.standard_normal(t.shape[0])
    return np.round(np.stack([left, right], axis=1) * 32767).astype(np.int16)


@pytest.mark.parametrize("rate_from,rate_to", R.RATE_PAIRS)
def test_rate_pair_within_derived_bound(ops, rate_from, rate_to):
    worst = R.check_rate_pair(ops, "cuda", rate_from, rate_to)
    print(f"{rate_from} -> {rate_to}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_both_tap_paths_give_the_fma_chain_bits(ops):
    R.check_fma_chain_bits(ops, "cuda")


def test_decode_only_is_load_audio_bit_for_bit(ops, tmp_path):
    R.check_decode_only(ops, "cuda", tmp_path)


def test_full_size_clip_and_side_stream(ops, tmp_path):
    """10 s of 44.1 kHz stereo int16 (441000 frames -> 160000 samples, 157 tiles): every output inside the bound, the loader against
    the host loader, and the same bits from a second call on a side stream."""
    from scipy.io import wavfile
    from svcmi.whisper import audio as A
    x = song(10.0, 44100, seed=11)
    assert x.shape == (441000, 2)
    y = R.run_kernel(ops, "cuda", x, 160, 441)
    ref, bound = R.oracle(R.host_decode(x), 160, 441)
    assert tuple(y.shape) == ref.shape == (160000,)
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    path = str(tmp_path / "song.wav")
    wavfile.write(path, 44100, x)
    got = R.check_loader_against_host(ops, "cuda", path)
    assert torch.equal(got, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = A.load_audio_device(path, ops=ops)
    side.synchronize()
    assert torch.equal(again, y)


def tiny_extractors(ops):
    from svcmi.hubert import inference as hubert_inf
    from svcmi.pitch import load_crepe
    from svcmi.whisper import inference as whisper_inf
    whisper = whisper_inf.load_model(W.make_whisper_state(C.WHISPER_TINY_TEST), "cuda", ops=ops)
    hubert = hubert_inf.load_model(W.make_hubert_state(C.HUBERT_TINY_TEST), "cuda", ops=ops)
    crepe = load_crepe(W.make_crepe_state("tiny"), "cuda", ops=ops)
    return whisper, hubert, crepe


@pytest.mark.parametrize("in_flight", [True, False])
def test_device_audio_through_the_extractors(ops, tmp_path, in_flight):
    """extract_features on the loader's device tensor against the same samples handed over as a numpy array: PPG and units bit-equal,
    F0 equal (the draws -- Whisper's mel noise, CREPE's input noise and dither -- pinned by seeding both generators)."""
    from scipy.io import wavfile
    from svcmi.svc_inference import extract_features
    from svcmi.whisper import audio as A
    path = str(tmp_path / "clip.wav")
    wavfile.write(path, 44100, song(1.3, 44100, seed=12))
    a = A.load_audio_device(path, ops=ops)
    assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (20800,)
    whisper, hubert, crepe = tiny_extractors(ops)

    def run(audio):
        torch.manual_seed(1234)
        np.random.seed(1234)
        ppg, vec, f0 = extract_features(audio, whisper, hubert, crepe, "cuda", in_flight=in_flight)
        torch.cuda.synchronize()
        return ppg, vec, f0

    ppg_d, vec_d, f0_d = run(a)
    ppg_h, vec_h, f0_h = run(a.cpu().numpy())
    assert tuple(ppg_d.shape) == (65, C.WHISPER_TINY_TEST["n_audio_state"]) and tuple(vec_d.shape) == (65, C.HUBERT_TINY_TEST["proj"])
    assert torch.equal(ppg_d, ppg_h) and torch.equal(vec_d, vec_h)
    assert f0_d.shape == f0_h.shape == (2 * (1 + 20800 // 320),) and np.array_equal(f0_d, f0_h, equal_nan=True)


def test_cli_parsers_take_a_loader_choice():
    from svcmi import svc_inference, svc_inference_batch
    base = ["--config", "c", "--model", "m", "--wave", "w", "--spk", "s"]
    for mod in (svc_inference, svc_inference_batch):
        assert mod.build_parser().parse_args(base).loader == "host"
        assert mod.build_parser().parse_args(base + ["--loader", "gpu"]).loader == "gpu"


def test_cli_with_gpu_loader(ops, tmp_path, monkeypatch):
    """``svc_inference --loader gpu`` on a 44.1 kHz stereo file: the three feature files and the output have the shapes of a
    1 s clip at 16 kHz."""
    import json
    import yaml
    from scipy.io import wavfile
    from workload import inputs as I
    from svcmi import svc_inference as SI
    from svcmi.pitch import load_csv_pitch
    monkeypatch.chdir(tmp_path)
    hp = C.tiny_hp()
    wavfile.write("in.wav", 44100, song(1.0, 44100, seed=13))
    torch.save({"model_g": W.make_vits_state(hp, seed=1234)}, "svc.pth")
    torch.save(W.make_whisper_state({**C.WHISPER_TINY_TEST, "n_audio_state": hp.vits.ppg_dim, "n_audio_head": 4}), "whisper.pt")
    torch.save(W.make_hubert_state(dict(C.HUBERT_TINY_TEST, proj=hp.vits.vec_dim)), "hubert.pt")
    torch.save(W.make_crepe_state("tiny"), "crepe.pth")
    np.save("spk.npy", I.synth_spk(hp.vits.spk_dim, seed=7).numpy())
    with open("cfg.yaml", "w") as f:
        yaml.safe_dump(json.loads(json.dumps(hp)), f)
    common = ["--config", "cfg.yaml", "--model", "svc.pth", "--wave", "in.wav", "--spk", "spk.npy",
              "--whisper", "whisper.pt", "--hubert", "hubert.pt", "--crepe", "crepe.pth"]
    torch.manual_seed(0)
    out = SI.main(SI.build_parser().parse_args(common + ["--loader", "gpu"]))
    ppg, vec, pit = np.load("svc_tmp.ppg.npy"), np.load("svc_tmp.vec.npy"), load_csv_pitch("svc_tmp.pit.csv")
    assert ppg.dtype == np.float32 and ppg.shape == (50, hp.vits.ppg_dim)           # 1 s -> 16000 samples -> 50 frames @50 fps
    assert vec.dtype == np.float32 and vec.shape == (50, hp.vits.vec_dim)
    assert len(pit) == 102                                                           # 2 * (1 + 16000 // 320)
    T = min(len(pit), 2 * vec.shape[0], 2 * ppg.shape[0])
    assert out.dtype == np.float32 and out.shape == (T * hp.data.hop_length - 1,) and np.isfinite(out).all()
    assert np.isfinite(ppg).all() and np.isfinite(vec).all()
