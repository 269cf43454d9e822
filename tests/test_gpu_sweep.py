"""The key sweep on a real MI355X: the checks of tests/sweep_cases.py on the device."""
import pytest

from tests import sweep_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.mark.parametrize("t", [1, 3, 37])
def test_pitch_rows_hold_the_bits_of_the_float64_product(ops, t):
    C.check_pitch_bits(ops, "cuda", t)


@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("H", [4, 192])
@pytest.mark.parametrize("t", [1, 37])
def test_embed_rows_hold_the_bits_of_embed_pitch(ops, t, H, K):
    C.check_embed_bits(ops, "cuda", t, H, K)


def test_embed_reads_a_strided_front_sum(ops):
    C.check_embed_strided(ops, "cuda")


def test_one_key_at_shift_zero_is_the_solo_run(ops):
    C.check_one_key_is_the_solo_run(ops, "cuda")


def test_three_keys_against_solo_runs_and_the_oracle(ops):
    C.check_three_keys(ops, "cuda")


def test_groups_of_keys(ops):
    C.check_grouping(ops, "cuda")


def test_two_chunks(ops):
    C.check_two_chunks(ops, "cuda")


def test_retrieval_runs_once_per_chunk(ops):
    C.check_retrieval_once_per_chunk(ops, "cuda")


def test_base_model_at_the_default_key_batch(ops):
    C.check_base_model(ops, "cuda")


def test_driver_arguments(ops):
    C.check_driver_arguments(ops, "cuda")
