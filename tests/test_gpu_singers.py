"""The singer sweep on a real MI355X: the checks of tests/singers_cases.py on the device."""
import pytest

from tests import singers_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("S", [1, 3, 32])
@pytest.mark.parametrize("i", [4, 40, 192])
@pytest.mark.parametrize("t", [1, 33, 37])
def test_sample_rows_hold_the_bits_of_sample_prior(ops, t, i, S):
    C.check_sample_bits(ops, "cuda", t, i, S)


def test_sample_reads_a_strided_statistics_view(ops):
    C.check_sample_strided(ops, "cuda")


def test_sample_bits_do_not_depend_on_the_row_split(ops):
    C.check_sample_split(ops, "cuda")


def test_one_singer_is_the_solo_run(ops):
    C.check_one_singer_is_the_solo_run(ops, "cuda")


def test_three_singers_against_solo_runs_and_the_oracle(ops):
    C.check_three_singers(ops, "cuda")


def test_groups_of_singers(ops):
    C.check_grouping(ops, "cuda")


def test_two_chunks(ops):
    C.check_two_chunks(ops, "cuda")


def test_retrieval_runs_once_per_chunk(ops):
    C.check_retrieval_once_per_chunk(ops, "cuda")


def test_base_model_at_the_default_singer_batch(ops):
    C.check_base_model(ops, "cuda")


def test_driver_arguments(ops):
    C.check_driver_arguments(ops, "cuda")
