"""Host side of the singer sweep, no GPU and no emulator: ``tools.mix_speaker_rows`` against ``tools.mix_speakers`` (svc_eva.py) bit for
bit, and the command line of svcmi.svc_inference_singers -- which voices it plans, under which names, what it refuses before any work --
run in process with a stub model."""
import json
import os

import numpy as np
import pytest
import torch

from workload import config as C

T50 = 3          # feature frames at 50 fps -> 6 synthesizer frames
BASE = ["--config", "c", "--model", "m", "--wave", "w"]


def _rows(n, dim=256, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(dim, generator=g).numpy() for _ in range(n)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("weights", [(0.5, 0.5), (0.0, 1.0), (0.3, 0.7), (0, 0, 0.5, 0.5), (0.2, 0.3, 0.5)])
def test_mix_speaker_rows_holds_the_bits_of_mix_speakers(tmp_path, weights):
    from svcmi import tools
    rows = _rows(len(weights))
    paths = []
    for k, r in enumerate(rows):
        assert r.dtype == np.float32
        paths.append(str(tmp_path / f"s{k}.npy"))
        np.save(paths[-1], r)
    want = tools.mix_speakers(dict(zip(paths, weights)), save_path=str(tmp_path / "eva.spk.npy"))
    got = tools.mix_speaker_rows(rows, weights)
    assert got.dtype == np.float64 and got.shape == (256,)
    assert np.array_equal(_bits(got), _bits(want))
    # ... and the expression is the reference's: a float32 product, a float64 sum
    eva = np.zeros(256)
    for r, w in zip(rows, weights):
        eva = eva + r * w
    assert np.array_equal(_bits(got), _bits(eva))
    with pytest.raises(ValueError):
        tools.mix_speaker_rows(rows, weights[:-1])


def test_a_blend_is_the_row_a_saved_eva_file_would_give(tmp_path, monkeypatch):
    from svcmi import svc_inference_singers as SS
    from svcmi import tools
    monkeypatch.chdir(tmp_path)
    a, b = _rows(2, seed=8)
    np.save("a.spk.npy", a)
    np.save("b.spk.npy", b)
    args = SS.build_parser().parse_args(BASE + ["--spk", "a.spk.npy", "b.spk.npy", "--blend-steps", "4"])
    plan = SS.plan_voices(args)
    fed = SS.load_voices(plan)
    assert fed.dtype == torch.float32 and fed.shape == (5, 256)
    for i, (w0, w1) in enumerate(SS.blend_weights(4)):
        tools.mix_speakers({"a.spk.npy": w0, "b.spk.npy": w1}, save_path="eva.spk.npy")
        want = torch.FloatTensor(np.load("eva.spk.npy"))              # svc_inference.py's own load of svc_eva.py's file
        assert torch.equal(fed[i], want), i
    assert torch.equal(fed[0], torch.FloatTensor(a)) and torch.equal(fed[4], torch.FloatTensor(b))


def test_parser_flags():
    from svcmi import svc_inference_singers as SS
    a = SS.build_parser().parse_args(BASE + ["--spk", "s1", "s2", "s3"])
    assert a.spk == ["s1", "s2", "s3"] and (a.shift, a.singer_batch, a.blend_steps) == (0, 16, None)
    assert (a.ppg, a.vec, a.pit) == (None, None, None)
    assert (a.f0, a.swipe_threshold, a.loader, a.precision, a.f0_precision) == ("crepe", 0.0, "host", "f32", "f32")
    assert a.enable_retrieval is False and a.retrieval_ratio == 0.5 and a.n_retrieval_vectors == 3
    assert a.whisper.endswith("large-v2.pt") and a.hubert.endswith("hubert-soft-0d54a1f4.pt") and a.crepe.endswith("full.pth")
    for gone in ("shift_l", "shift_r", "key_batch", "vad_post"):
        assert not hasattr(a, gone)
    with pytest.raises(SystemExit):
        SS.build_parser().parse_args(BASE)                               # --spk is required
    with pytest.raises(SystemExit):
        SS.build_parser().parse_args(BASE + ["--spk"])


def test_voices_from_files_and_directories(tmp_path, monkeypatch):
    from svcmi import svc_inference_singers as SS
    monkeypatch.chdir(tmp_path)
    os.makedirs("singers")
    os.makedirs("other")
    for name in ("singers/singer0002.npy", "singers/singer0010.npy", "singers/singer0001.npy", "singers/notes.txt", "mine.spk.npy", "other/singer0002.spk.npy"):
        open(name, "w").close()
    parse = lambda *spk, extra=(): SS.build_parser().parse_args(BASE + ["--spk", *spk, *extra])
    plan = SS.plan_voices(parse("mine.spk.npy", "singers"))
    assert [p[0] for p in plan] == ["mine", "singer0001", "singer0002", "singer0010"]               # the directory in sorted order, after the file
    assert [p[1] for p in plan] == [["mine.spk.npy"]] + [[os.path.join("singers", f"singer{n}.npy")] for n in ("0001", "0002", "0010")]
    assert all(p[2] is None for p in plan)
    assert SS.stem("a/b/x.spk.npy") == "x" and SS.stem("x.npy") == "x" and SS.stem("x.bin") == "x.bin"
    with pytest.raises(ValueError, match="singer0002"):
        SS.plan_voices(parse("singers", "other/singer0002.spk.npy"))                                # two files, one output name
    with pytest.raises(ValueError):
        SS.plan_voices(parse("mine.spk.npy", "mine.spk.npy"))
    os.makedirs("empty")
    with pytest.raises(ValueError):
        SS.plan_voices(parse("empty"))
    # --blend-steps: exactly two embeddings
    for spk in (("mine.spk.npy",), ("singers",), ("mine.spk.npy", "singers/singer0001.npy", "singers/singer0002.npy")):
        with pytest.raises(ValueError):
            SS.plan_voices(parse(*spk, extra=("--blend-steps", "4")))
    with pytest.raises(ValueError):
        SS.plan_voices(parse("mine.spk.npy", "singers/singer0001.npy", extra=("--blend-steps", "0")))
    assert SS.blend_weights(4) == [(1.0, 0.0), (0.75, 0.25), (0.5, 0.5), (0.25, 0.75), (0.0, 1.0)]
    plan = SS.plan_voices(parse("mine.spk.npy", "singers/singer0001.npy", extra=("--blend-steps", "4")))
    assert [p[0] for p in plan] == ["blend_00of04", "blend_01of04", "blend_02of04", "blend_03of04", "blend_04of04"]
    assert all(p[1] == ["mine.spk.npy", "singers/singer0001.npy"] for p in plan) and [p[2] for p in plan] == SS.blend_weights(4)
    assert [p[0] for p in SS.plan_voices(parse("other", "mine.spk.npy", extra=("--blend-steps", "1")))] == ["blend_00of01", "blend_01of01"]


class StubModel:
    """Stands in for SynthesizerInfer under svc_infer_singers: a waveform that names its speaker row and the pitch it was given."""

    def __init__(self, hop):
        self.hop, self.calls = hop, []

    def pitch2source(self, f0, noise=None):
        return torch.zeros(f0.shape[0], 1, f0.shape[1] * self.hop)

    def inference_singers(self, ppg, vec, pit, spks, ppg_l, source, noise=None, return_parts=False):
        S, T = spks.shape[0], ppg.shape[1]
        assert ppg.shape[0] == vec.shape[0] == pit.shape[0] == 1 and int(ppg_l[0]) == T and source.shape == (1, 1, T * self.hop)
        self.calls.append(S)
        return (spks.sum(1) + pit.mean() / 1000).view(S, 1, 1) * torch.ones(S, 1, T * self.hop)


def _files(hp):
    import yaml
    g = torch.Generator().manual_seed(21)
    np.save("in.ppg.npy", torch.randn(T50, hp.vits.ppg_dim, generator=g).numpy())
    np.save("in.vec.npy", torch.randn(T50, hp.vits.vec_dim, generator=g).numpy())
    with open("in.pit.csv", "w") as f:
        for i, v in enumerate((0, 187, 233, 96, 523, 441, 30)):          # one frame more than the features: trimmed like svc_infer does
            f.write(f"{i * 0.01:.2f},{v}\n")
    with open("cfg.yaml", "w") as f:
        yaml.safe_dump(json.loads(json.dumps(hp)), f)
    return ["--config", "cfg.yaml", "--model", "svc.pth", "--wave", "in.wav", "--ppg", "in.ppg.npy", "--vec", "in.vec.npy", "--pit", "in.pit.csv"]


def test_cli_writes_one_file_per_voice(tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    from svcmi import svc_inference_singers as SS
    monkeypatch.chdir(tmp_path)
    hp = C.tiny_hp()
    hop = hp.data.hop_length
    argv = _files(hp)
    rows = _rows(3, dim=hp.vits.spk_dim, seed=12)
    os.makedirs("voices")
    for name, r in zip(("voices/b.npy", "voices/a.spk.npy", "solo.spk.npy"), rows):
        np.save(name, r)
    stub = StubModel(hop)
    monkeypatch.setattr(SS, "load_model", lambda args, hp_, device, ops=None: stub)
    pit = np.array([0, 187, 233, 96, 523, 441], np.float64)
    n = 2 * T50 * hop - 1

    def expect(row, shift):
        p = torch.FloatTensor(pit * 2 ** (shift / 12)) if shift else torch.FloatTensor(pit)
        return float(torch.FloatTensor(row).sum() + p.mean() / 1000)

    outs = SS.main(SS.build_parser().parse_args(argv + ["--spk", "solo.spk.npy", "voices", "--singer-batch", "2"]), device="cpu")
    printed = capsys.readouterr().out.splitlines()
    assert printed[-4:] == ["pitch shift:  0", "solo", "a", "b"]
    assert sorted(os.listdir("_svc_out")) == ["svc_out_a.wav", "svc_out_b.wav", "svc_out_solo.wav"] and list(outs) == ["solo", "a", "b"]
    assert stub.calls == [2, 1]                                          # groups of --singer-batch
    for name, row in (("solo", rows[2]), ("a", rows[1]), ("b", rows[0])):
        sr, written = wavfile.read(f"_svc_out/svc_out_{name}.wav")
        assert sr == hp.data.sampling_rate and written.dtype == np.float32 and written.shape == (n,)
        assert np.array_equal(written, outs[name]) and np.allclose(written, expect(row, 0), rtol=1e-6, atol=0)
    assert not os.path.exists("svc_out.wav") and not os.path.exists("svc_out_pit.wav")
    # a blend at another key: --shift goes through shift_pitch as in svc_inference.main
    stub.calls.clear()
    outs = SS.main(SS.build_parser().parse_args(argv + ["--spk", "voices/a.spk.npy", "voices/b.npy", "--blend-steps", "2", "--shift", "12"]), device="cpu")
    printed = capsys.readouterr().out.splitlines()
    assert printed[-5] == "pitch shift:  12" and printed[-4].startswith("source pitch statics")
    assert printed[-3:] == ["blend_00of02", "blend_01of02", "blend_02of02"]
    assert stub.calls == [3] and {"svc_out_blend_00of02.wav", "svc_out_blend_01of02.wav", "svc_out_blend_02of02.wav"} <= set(os.listdir("_svc_out"))
    mid = torch.FloatTensor(np.zeros(hp.vits.spk_dim) + rows[1] * 0.5 + rows[0] * 0.5).numpy()
    for name, row in (("blend_00of02", rows[1]), ("blend_01of02", mid), ("blend_02of02", rows[0])):
        assert np.allclose(outs[name], expect(row, 12), rtol=1e-6, atol=0), name


def test_cli_refuses_before_any_work(tmp_path, monkeypatch):
    from svcmi import svc_inference_singers as SS
    monkeypatch.chdir(tmp_path)
    for name in ("x.npy", "x.spk.npy"):
        open(name, "w").close()
    monkeypatch.setattr(SS, "ensure_features", lambda *a, **k: pytest.fail("features were extracted"))
    for spk, extra in ((["x.npy", "x.spk.npy"], []), (["x.npy"], ["--blend-steps", "3"])):
        with pytest.raises(ValueError):
            SS.main(SS.build_parser().parse_args(BASE + ["--spk", *spk, *extra]), device="cpu")
    assert not os.path.exists("_svc_out")
