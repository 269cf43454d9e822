"""The SWIPE' F0 extractor on a real MI355X: the checks of tests/swipe_cases.py on the device in the production geometry (the whole
golden clips against the reference's record) and in the small ones, and ``svc_inference.main`` with ``--f0 swipe`` at the tiny model size
with a CREPE path that does not exist.  Reads only tests/golden/."""
import os

import numpy as np
import pytest
import torch

from tests import swipe_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("geometry", ["small", "mid", "full"])
def test_kernels_one_by_one(ops, geometry):
    geo, n = {"small": (C.SMALL, 333), "mid": (C.MID, 900), "full": (None, 700)}[geometry]
    print(C.check_kernels(ops, "cuda", geo, n=n))


@pytest.mark.parametrize("geometry", ["small", "full"])
def test_stage_shapes(ops, geometry):
    print(C.check_stage_shapes(ops, "cuda", C.SMALL if geometry == "small" else None))


@pytest.mark.parametrize("geometry", ["small", "full"])
def test_silence_is_f_min_with_confidence_zero(ops, geometry):
    C.check_silence(ops, "cuda", C.SMALL if geometry == "small" else None)


def test_arg_max_at_the_last_candidate(ops):
    C.check_last_candidate(ops, "cuda")


def test_arg_max_at_candidate_zero_wraps(ops):
    C.check_wrap(ops, "cuda")


def test_exact_ties_take_the_lowest_index(ops):
    C.check_ties(ops, "cuda")


def test_stage_bits_do_not_depend_on_the_launch(ops):
    C.check_repeatable(ops, "cuda")


@pytest.mark.parametrize("name", C.CLIPS)
def test_end_to_end_equals_the_reference(ops, name):
    C.check_end_to_end(ops, "cuda", name)


def test_swipe_slim_returns_what_the_reference_returns(ops):
    C.check_api(ops, "cuda")


@pytest.mark.parametrize("name", ["035", "010"])
def test_compute_f0_swipe(ops, name):
    C.check_compute_f0_swipe(ops, "cuda", name)


def test_command_line_with_swipe_never_opens_the_crepe_checkpoint(ops, tmp_path, monkeypatch):
    """svc_inference.main with --f0 swipe, the tiny seeded models and a --crepe path that does not exist, on the whole 035.wav:
    svc_tmp.pit.csv holds the recipe's track, with all three features from the wav and with only --pit missing.  Nothing is replaced."""
    from svcmi import svc_inference as SI
    from svcmi.pitch import compute_f0_swipe
    x = C.prepare_cli_files(tmp_path, monkeypatch)
    want = compute_f0_swipe(x, "cuda")
    torch.manual_seed(0)
    out = SI.main(SI.build_parser().parse_args(C.CLI_ARGS))
    assert out.dtype == np.float32 and np.isfinite(out).all()
    first = C.check_csv("svc_tmp.pit.csv", want)
    os.remove("svc_tmp.pit.csv")
    torch.manual_seed(0)
    out2 = SI.main(SI.build_parser().parse_args(C.CLI_ARGS + ["--ppg", "svc_tmp.ppg.npy", "--vec", "svc_tmp.vec.npy"]))
    assert np.array_equal(C.check_csv("svc_tmp.pit.csv", want), first) and out2.shape == out.shape
