"""The salience F0 extractor on a real MI355X: the checks of tests/salience_cases.py on the device, and ``svc_inference.main`` with
``--f0 salience`` at the tiny model size with a CREPE path that does not exist."""
import os

import numpy as np
import pytest
import torch

from tests import salience_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("T", [2, 3, 33])
def test_stft_against_float64(ops, T):
    print(f"salience STFT, {T} frames: worst error / bound {C.check_stft_frames(ops, 'cuda', T):.3f}")


def test_stft_of_a_clip_against_float64(ops):
    print(f"salience STFT, 035.wav: worst error / bound {C.check_stft_clip(ops, 'cuda'):.3f}")


def test_stft_bits_do_not_depend_on_the_launch(ops):
    C.check_stft_bits(ops, "cuda")


@pytest.mark.parametrize("name", C.CLIPS)
def test_map_from_a_given_spectrum(ops, name):
    C.check_map_clip(ops, "cuda", name)


def test_map_of_silence_is_zero_without_nan(ops):
    C.check_map_silence(ops, "cuda")


@pytest.mark.parametrize("T", [2, 3, 33])
def test_dp_equals_the_float64_programme(ops, T):
    C.check_dp_random(ops, "cuda", T)


def test_dp_exact_ties_take_the_lowest_index(ops):
    C.check_dp_zero_columns(ops, "cuda")


def test_dp_rounding_tie(ops):
    C.check_dp_rounding_tie(ops, "cuda")


def test_dp_limits(ops):
    C.check_dp_limits(ops, "cuda")


def test_dp_repeatable(ops):
    C.check_dp_repeatable(ops, "cuda")


@pytest.mark.parametrize("name", C.CLIPS)
def test_end_to_end_equals_the_reference(ops, name):
    C.check_end_to_end(ops, "cuda", name)


def test_salience_returns_what_the_reference_returns(ops):
    C.check_salience_api(ops, "cuda")


def test_edges(ops):
    C.check_edges(ops, "cuda")


def test_command_line_with_salience_never_opens_the_crepe_checkpoint(ops, tmp_path, monkeypatch):
    """svc_inference.main with --f0 salience, the tiny seeded models and a --crepe path that does not exist: svc_tmp.pit.csv equals
    save_csv_pitch of the golden track, with all three features from the wav and with only --pit missing."""
    from svcmi import svc_inference as SI
    C.prepare_cli_files(tmp_path, monkeypatch)
    want = open("want.csv").read()
    torch.manual_seed(0)
    out = SI.main(SI.build_parser().parse_args(C.CLI_ARGS))
    assert out.dtype == np.float32 and np.isfinite(out).all() and open("svc_tmp.pit.csv").read() == want
    os.remove("svc_tmp.pit.csv")
    torch.manual_seed(0)
    out2 = SI.main(SI.build_parser().parse_args(C.CLI_ARGS + ["--ppg", "svc_tmp.ppg.npy", "--vec", "svc_tmp.vec.npy"]))
    assert open("svc_tmp.pit.csv").read() == want and out2.shape == out.shape
