"""The YIN F0 extractor on a real MI355X: the checks of tests/yin_cases.py on the device."""
import pytest

from tests import yin_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("T", [2, 3, 33])
def test_cmndf_rows_hold_the_bits_of_pyin(ops, T):
    C.check_cmndf_equals_pyin(ops, "cuda", T)


@pytest.mark.parametrize("T", [2, 3, 33])
def test_cmndf_rows_hold_the_bits_of_pyin_smallest_geometry(ops, T):
    C.check_cmndf_equals_pyin(ops, "cuda", T, small=True)


def test_cmndf_of_a_single_frame(ops):
    C.check_cmndf_one_frame(ops, "cuda")


def test_pick_from_built_rows(ops):
    C.check_pick_built(ops, "cuda")


def test_pick_with_a_single_lag(ops):
    C.check_pick_single_lag(ops, "cuda")


def test_pick_from_the_golden_rows(ops):
    C.check_pick_golden(ops, "cuda")


@pytest.mark.parametrize("small", [False, True])
def test_aperiodicity_against_longdouble(ops, small):
    C.check_ap_lags(ops, "cuda", small=small)


def test_aperiodicity_of_silence_is_exactly_zero(ops):
    C.check_ap_silence(ops, "cuda")


def test_aperiodicity_of_short_clips(ops):
    C.check_ap_short_clips(ops, "cuda")


def test_aperiodicity_bits_do_not_depend_on_the_launch(ops):
    C.check_ap_bits(ops, "cuda")


@pytest.mark.parametrize("name", C.CLIPS)
def test_end_to_end_equals_the_reference(ops, name):
    C.check_end_to_end(ops, "cuda", name)


def test_yin_returns_what_the_reference_returns(ops):
    C.check_yin_api(ops, "cuda")


def test_compute_f0_yin(ops):
    C.check_compute_f0_yin(ops, "cuda")


def test_edges(ops):
    C.check_edges(ops, "cuda")
