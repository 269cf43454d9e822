"""The pYIN F0 extractor on a real MI355X: the checks of tests/pyin_cases.py on the device, and ``svc_inference.main`` with ``--f0 pyin`` at
the tiny model size with a CREPE path that does not exist."""
import os

import numpy as np
import pytest
import torch

from tests import pyin_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("T", [2, 3, 33])
def test_cmndf_against_longdouble(ops, T):
    C.check_cmndf_frames(ops, "cuda", T)


def test_cmndf_smallest_geometry(ops):
    C.check_cmndf_frames(ops, "cuda", 41, small=True)


def test_cmndf_of_silence_is_zero_without_nan(ops):
    C.check_cmndf_silence(ops, "cuda")


def test_cmndf_bits_do_not_depend_on_the_launch(ops):
    C.check_cmndf_bits(ops, "cuda")


def test_observation_from_built_rows(ops):
    C.check_observe_built(ops, "cuda")


def test_observation_from_the_golden_rows(ops):
    C.check_observe_golden(ops, "cuda")


@pytest.mark.parametrize("T", [2, 3, 33])
def test_viterbi_equals_the_dense_programme(ops, T):
    C.check_viterbi_random(ops, "cuda", T)


def test_viterbi_sizes_and_limits(ops):
    C.check_viterbi_sizes(ops, "cuda")


def test_viterbi_exact_ties_take_the_lowest_index(ops):
    C.check_viterbi_ties(ops, "cuda")


def test_viterbi_rounding_tie(ops):
    C.check_viterbi_rounding_tie(ops, "cuda")


def test_viterbi_takes_an_impossible_transition_when_it_must(ops):
    C.check_viterbi_impossible(ops, "cuda")


def test_viterbi_repeatable(ops):
    C.check_viterbi_repeatable(ops, "cuda")


@pytest.mark.parametrize("name", C.CLIPS)
def test_end_to_end_equals_the_reference(ops, name):
    C.check_end_to_end(ops, "cuda", name)


def test_pyin_returns_what_the_reference_returns(ops):
    C.check_pyin_api(ops, "cuda")


def test_compute_f0_pyin(ops):
    C.check_compute_f0_pyin(ops, "cuda")


def test_edges(ops):
    C.check_edges(ops, "cuda")


def test_extract_features_takes_pyin_without_a_crepe_model(ops, monkeypatch):
    """extract_features(..., f0="pyin") with ``crepe=None``; the two network extractors are stubbed (their own tests run them)."""
    from svcmi import svc_inference as SI
    from svcmi.hubert import inference as hubert_inf
    from svcmi.whisper import inference as whisper_inf
    monkeypatch.setattr(whisper_inf, "ppg_from_audio", lambda m, a: torch.zeros(1, device="cuda"))
    monkeypatch.setattr(hubert_inf, "units_windowed", lambda m, a: torch.zeros(1, device="cuda"))
    _, _, f0 = SI.extract_features(C.clip("glide"), torch.nn.Module(), None, None, "cuda", f0="pyin")
    want = C.golden()["f0_glide"]
    assert f0.shape == (2 * len(want),) and np.array_equal(f0[0::2] == 0, want == 0)


def test_command_line_with_pyin_never_opens_the_crepe_checkpoint(ops, tmp_path, monkeypatch):
    """svc_inference.main with --f0 pyin, the tiny seeded models and a --crepe path that does not exist: svc_tmp.pit.csv holds the golden
    track, with all three features from the wav and with only --pit missing.  Nothing is replaced."""
    from svcmi import svc_inference as SI
    want, tol = C.prepare_cli_files(tmp_path, monkeypatch)
    torch.manual_seed(0)
    out = SI.main(SI.build_parser().parse_args(C.CLI_ARGS))
    assert out.dtype == np.float32 and np.isfinite(out).all()
    first = C.check_csv("svc_tmp.pit.csv", want, tol)
    os.remove("svc_tmp.pit.csv")
    torch.manual_seed(0)
    out2 = SI.main(SI.build_parser().parse_args(C.CLI_ARGS + ["--ppg", "svc_tmp.ppg.npy", "--vec", "svc_tmp.vec.npy"]))
    assert np.array_equal(C.check_csv("svc_tmp.pit.csv", want, tol), first) and out2.shape == out.shape
