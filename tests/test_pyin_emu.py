"""The pYIN F0 extractor's kernels (csrc/pyin.hip), stage (svcmi_pyin_f0_fwd) and drop-ins (svcmi.pitch.core.pyin, svcmi.pitch.compute_f0_pyin,
svc_inference --f0 pyin) executed on the CPU by the SIMT emulator: the checks of tests/pyin_cases.py.  Where the reference checkout is
present, the float64 programme of the case file is proven equal to it bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests import pyin_cases as C
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("T", [2, 3, 33])
def test_cmndf_against_longdouble(ops, T):
    C.check_cmndf_frames(ops, "cpu", T)


def test_cmndf_smallest_geometry(ops):
    C.check_cmndf_frames(ops, "cpu", 41, small=True)


def test_cmndf_of_silence_is_zero_without_nan(ops):
    C.check_cmndf_silence(ops, "cpu")


def test_cmndf_bits_do_not_depend_on_the_launch(ops):
    C.check_cmndf_bits(ops, "cpu")


def test_observation_from_built_rows(ops):
    C.check_observe_built(ops, "cpu")


def test_observation_from_the_golden_rows(ops):
    C.check_observe_golden(ops, "cpu")


@pytest.mark.parametrize("T", [2, 3, 33])
def test_viterbi_equals_the_dense_programme(ops, T):
    C.check_viterbi_random(ops, "cpu", T)


def test_viterbi_sizes_and_limits(ops):
    C.check_viterbi_sizes(ops, "cpu")


def test_viterbi_exact_ties_take_the_lowest_index(ops):
    C.check_viterbi_ties(ops, "cpu")


def test_viterbi_rounding_tie(ops):
    C.check_viterbi_rounding_tie(ops, "cpu")


def test_viterbi_takes_an_impossible_transition_when_it_must(ops):
    C.check_viterbi_impossible(ops, "cpu")


def test_viterbi_repeatable(ops):
    C.check_viterbi_repeatable(ops, "cpu")


@pytest.mark.parametrize("name", C.CLIPS)
def test_end_to_end_equals_the_reference(ops, name):
    C.check_end_to_end(ops, "cpu", name)


def test_pyin_returns_what_the_reference_returns(ops):
    C.check_pyin_api(ops, "cpu")


def test_compute_f0_pyin(ops):
    C.check_compute_f0_pyin(ops, "cpu")


def test_edges(ops):
    C.check_edges(ops, "cpu")


def test_extract_features_takes_pyin_without_a_crepe_model(ops, monkeypatch):
    """extract_features(..., f0="pyin") never touches ``crepe`` (None here); the other two extractors are stubbed."""
    from svcmi import svc_inference as SI
    from svcmi.hubert import inference as hubert_inf
    from svcmi.whisper import inference as whisper_inf
    monkeypatch.setattr(whisper_inf, "ppg_from_audio", lambda m, a: "ppg")
    monkeypatch.setattr(hubert_inf, "units_windowed", lambda m, a: "vec")
    ppg, vec, f0 = SI.extract_features(C.clip("glide"), None, None, None, "cpu", f0="pyin", ops=ops)
    want = C.golden()["f0_glide"]
    assert (ppg, vec) == ("ppg", "vec") and f0.shape == (2 * len(want),) and np.array_equal(f0[0::2] == 0, want == 0)
    assert "pyin" in SI.F0_METHODS


def test_command_line_with_pyin_never_opens_the_crepe_checkpoint(ops, tmp_path, monkeypatch):
    """svc_inference.main with --f0 pyin, the tiny seeded models and a --crepe path that does not exist: svc_tmp.pit.csv holds the golden
    track (zeros exactly, voiced frames within the f0 tolerance).  Run twice: all three features from the wav, and with only --pit
    missing.  The F0 extractor runs on the emulator; the two network extractors and the synthesizer are replaced by stand-ins of the
    right shapes (tests/test_gpu_pyin.py runs the same command with nothing replaced)."""
    from svcmi import svc_inference as SI
    from svcmi.hubert import inference as hubert_inf
    from svcmi.whisper import inference as whisper_inf
    want, tol = C.prepare_cli_files(tmp_path, monkeypatch)
    hp = SI.load_config("cfg.yaml")
    frames = 1 + C.clip("035").shape[0] // 320
    monkeypatch.setattr(whisper_inf, "ppg_from_audio", lambda m, a: torch.zeros(frames, hp.vits.ppg_dim))
    monkeypatch.setattr(hubert_inf, "units_windowed", lambda m, a: torch.zeros(frames, hp.vits.vec_dim))
    seen = []

    def synth(model, retrieval, spk, pit, ppg, vec, hp_, device, **kw):
        seen.append(pit.numpy().copy())
        return np.zeros(8, np.float32)
    monkeypatch.setattr(SI, "svc_infer", synth)
    SI.main(SI.build_parser().parse_args(C.CLI_ARGS), device="cpu", ops=ops)
    first = C.check_csv("svc_tmp.pit.csv", want, tol)
    os.remove("svc_tmp.pit.csv")
    SI.main(SI.build_parser().parse_args(C.CLI_ARGS + ["--ppg", "svc_tmp.ppg.npy", "--vec", "svc_tmp.vec.npy"]), device="cpu", ops=ops)
    assert np.array_equal(C.check_csv("svc_tmp.pit.csv", want, tol), first)
    assert len(seen) == 2 and np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], first.astype(np.float32))


# ------------------------------------------------------------------------------------------------ the programme against the reference
def _reference():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_pyin_golden", os.path.join(root, "scripts", "make_pyin_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_reference("/root/reference")


@pytest.mark.needs_reference
def test_programme_equals_the_reference_on_every_frame_of_the_golden_clips():
    """O, lag_thr, val_thr of every frame (NaN positions included), rms, the path's f0 and conf: the case file's float64 programme against
    the reference's own ``pyin`` internals, bit for bit; plus seeded noise frames and a 50 Hz tone through the thresholding alone."""
    ref = _reference()
    pl = C.plan("cpu")
    B = pl.B
    rng = np.random.default_rng(7)
    for k in range(24):
        fr = rng.standard_normal(2048) * (10.0 ** -rng.integers(0, 4)) if k % 4 else np.sin(2 * np.pi * 50.0 * np.arange(2048) / 16000 + k)
        c = ref.cumulative_mean_normalized_difference_function(fr.astype(np.float32).astype(np.float64), pl.p_max)
        assert C.same_bits(c, C.cmndf_f64(fr.astype(np.float32).astype(np.float64), pl.p_max))
        with np.errstate(divide="ignore", invalid="ignore"):
            Om, lag, val = ref.probabilistic_thresholding(c.copy(), pl.thresholds_np, pl.p_min, pl.p_max, 0.01, pl.F_axis, 16000, pl.beta_np)
        mine = C.observe_frame(c, pl.thresholds_np, pl.beta_np, pl.p_min, pl.p_max, 0.01, pl.F_axis, 16000)
        assert C.same_bits(Om[:B], mine[0]) and not Om[B:].any() and C.same_bits(lag, mine[1]) and C.same_bits(val, mine[2]), k
    kept = {}
    real = ref.yin_multi_thr

    def tap(*a, **k):
        kept["out"] = real(*a, **k)
        return kept["out"]
    ref.yin_multi_thr = tap
    g = C.golden()
    for name in C.CLIPS:
        x = C.clip(name)
        with np.errstate(divide="ignore", invalid="ignore"):
            f0, t, conf = ref.pyin(x, **C.P)
            mine = C.pyin_ref(x, pl)
        O, rms, lag, val = kept["out"]
        assert C.same_bits(mine["O"], O) and C.same_bits(mine["lag_thr"], lag) and C.same_bits(mine["val_thr"], val) and C.same_bits(mine["rms"], rms)
        assert C.same_bits(mine["f0"], f0) and C.same_bits(mine["conf"], conf)
        assert C.same_bits(f0, g[f"f0_{name}"]) and np.array_equal(mine["path"], g[f"path_{name}"])
