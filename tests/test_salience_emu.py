"""The salience F0 extractor's kernels (csrc/salience.hip), stage (svcmi_salience_f0_fwd) and drop-ins (svcmi.pitch.core.salience,
svcmi.pitch.compute_f0_salience, svc_inference --f0 salience) executed on the CPU by the SIMT emulator: the checks of tests/salience_cases.py."""
import os

import numpy as np
import pytest
import torch

from tests import salience_cases as C
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("T", [2, 3, 33])
def test_stft_against_float64(ops, T):
    C.check_stft_frames(ops, "cpu", T)


def test_stft_bits_do_not_depend_on_the_launch(ops):
    C.check_stft_bits(ops, "cpu")


def test_map_from_a_given_spectrum(ops):
    C.check_map_clip(ops, "cpu", "glide")


def test_map_of_silence_is_zero_without_nan(ops):
    C.check_map_silence(ops, "cpu")


@pytest.mark.parametrize("T", [2, 3, 33])
def test_dp_equals_the_float64_programme(ops, T):
    C.check_dp_random(ops, "cpu", T)


def test_dp_exact_ties_take_the_lowest_index(ops):
    C.check_dp_zero_columns(ops, "cpu")


def test_dp_rounding_tie(ops):
    C.check_dp_rounding_tie(ops, "cpu")


def test_dp_limits(ops):
    C.check_dp_limits(ops, "cpu")


def test_dp_repeatable(ops):
    C.check_dp_repeatable(ops, "cpu")


@pytest.mark.parametrize("name", C.CLIPS)
def test_end_to_end_equals_the_reference(ops, name):
    C.check_end_to_end(ops, "cpu", name)


def test_salience_returns_what_the_reference_returns(ops):
    C.check_salience_api(ops, "cpu")


def test_edges(ops):
    C.check_edges(ops, "cpu")


def test_extract_features_takes_salience_without_a_crepe_model(ops, monkeypatch):
    """extract_features(..., f0="salience") never touches ``crepe`` (None here); the other two extractors are stubbed."""
    from svcmi import svc_inference as SI
    from svcmi.hubert import inference as hubert_inf
    from svcmi.whisper import inference as whisper_inf
    monkeypatch.setattr(whisper_inf, "ppg_from_audio", lambda m, a: "ppg")
    monkeypatch.setattr(hubert_inf, "units_windowed", lambda m, a: "vec")
    ppg, vec, f0 = SI.extract_features(C.clip("glide"), None, None, None, "cpu", f0="salience", ops=ops)
    assert (ppg, vec) == ("ppg", "vec") and np.array_equal(f0, C.golden()["track_glide"])
    with pytest.raises(ValueError, match="f0"):
        SI.extract_features(C.clip("glide"), None, None, None, "cpu", f0="yin", ops=ops)


def test_command_line_with_salience_never_opens_the_crepe_checkpoint(ops, tmp_path, monkeypatch):
    """svc_inference.main with --f0 salience, the tiny seeded models and a --crepe path that does not exist: svc_tmp.pit.csv equals
    save_csv_pitch of the golden track.  Run twice: all three features from the wav, and with only --pit missing.  The F0 extractor runs
    on the emulator; the two network extractors and the synthesizer, which take tens of minutes there at any clip length, are replaced by
    stand-ins of the right shapes (tests/test_gpu_salience.py runs the same command with nothing replaced)."""
    from svcmi import svc_inference as SI
    from svcmi.hubert import inference as hubert_inf
    from svcmi.whisper import inference as whisper_inf
    C.prepare_cli_files(tmp_path, monkeypatch)
    hp = SI.load_config("cfg.yaml")
    frames = 1 + C.clip("035").shape[0] // 320
    monkeypatch.setattr(whisper_inf, "ppg_from_audio", lambda m, a: torch.zeros(frames, hp.vits.ppg_dim))
    monkeypatch.setattr(hubert_inf, "units_windowed", lambda m, a: torch.zeros(frames, hp.vits.vec_dim))
    seen = []

    def synth(model, retrieval, spk, pit, ppg, vec, hp_, device, **kw):
        seen.append(pit.numpy().copy())
        return np.zeros(8, np.float32)
    monkeypatch.setattr(SI, "svc_infer", synth)
    want = open("want.csv").read()
    SI.main(SI.build_parser().parse_args(C.CLI_ARGS), device="cpu", ops=ops)
    assert open("svc_tmp.pit.csv").read() == want
    os.remove("svc_tmp.pit.csv")
    SI.main(SI.build_parser().parse_args(C.CLI_ARGS + ["--ppg", "svc_tmp.ppg.npy", "--vec", "svc_tmp.vec.npy"]), device="cpu", ops=ops)
    assert open("svc_tmp.pit.csv").read() == want
    assert len(seen) == 2 and np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], np.floor(C.golden()["track_035"]).astype(np.float32))
