"""The key sweep's kernels (csrc/sweep.hip), stage (svcmi_synth_sweep_fwd) and driver (svc_infer_sweep) executed on the CPU by the SIMT
emulator: the checks of tests/sweep_cases.py.  The emulator runs a synthesizer frame in about two seconds, so the one-key case alone keeps
T = 37 here and the other stage cases run at T = 5 (odd, shorter than every tile; the unvoiced frame and the two clamp pitches are in
the clip at every length); tests/test_gpu_sweep.py runs all of them at full length."""
import pytest

from tests import sweep_cases as C
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("t", [1, 3, 37])
def test_pitch_rows_hold_the_bits_of_the_float64_product(ops, t):
    C.check_pitch_bits(ops, "cpu", t)


@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("H", [4, 192])
@pytest.mark.parametrize("t", [1, 37])
def test_embed_rows_hold_the_bits_of_embed_pitch(ops, t, H, K):
    C.check_embed_bits(ops, "cpu", t, H, K)


def test_embed_reads_a_strided_front_sum(ops):
    C.check_embed_strided(ops, "cpu")


def test_one_key_at_shift_zero_is_the_solo_run(ops):
    C.check_one_key_is_the_solo_run(ops, "cpu")


def test_three_keys_against_solo_runs_and_the_oracle(ops):
    C.check_three_keys(ops, "cpu", T=5)


def test_groups_of_keys(ops):
    C.check_grouping(ops, "cpu", T=5)


def test_retrieval_runs_once_per_chunk(ops):
    C.check_retrieval_once_per_chunk(ops, "cpu", T=6, check_changed=False)


def test_driver_arguments(ops):
    C.check_driver_arguments(ops, "cpu")
