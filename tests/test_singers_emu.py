"""The singer sweep's kernel (csrc/sweep.hip: sweep_sample_prior), stage (svcmi_synth_singers_fwd) and driver (svc_infer_singers) executed on
the CPU by the SIMT emulator: the checks of tests/singers_cases.py.  The emulator runs a synthesizer frame in about two seconds, so the
one-singer case alone keeps T = 37 here and the other stage cases run at T = 5 or 6 (odd / shorter than every tile; the unvoiced frame
and the two clamp pitches are in the clip at every length); tests/test_gpu_singers.py runs all of them at full length, with the two-chunk
and base-width cases."""
import pytest

from tests import singers_cases as C
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("S", [1, 3, 32])
@pytest.mark.parametrize("i", [4, 40, 192])
@pytest.mark.parametrize("t", [1, 33, 37])
def test_sample_rows_hold_the_bits_of_sample_prior(ops, t, i, S):
    C.check_sample_bits(ops, "cpu", t, i, S)


def test_sample_reads_a_strided_statistics_view(ops):
    C.check_sample_strided(ops, "cpu")


def test_sample_bits_do_not_depend_on_the_row_split(ops):
    C.check_sample_split(ops, "cpu")


def test_one_singer_is_the_solo_run(ops):
    C.check_one_singer_is_the_solo_run(ops, "cpu")


def test_three_singers_against_solo_runs_and_the_oracle(ops):
    C.check_three_singers(ops, "cpu", T=5)


def test_groups_of_singers(ops):
    C.check_grouping(ops, "cpu", T=5)


def test_retrieval_runs_once_per_chunk(ops):
    C.check_retrieval_once_per_chunk(ops, "cpu", T=6, check_changed=False)


def test_driver_arguments(ops):
    C.check_driver_arguments(ops, "cpu")
