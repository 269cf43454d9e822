"""The GPU wav loader's kernel (csrc/resample.hip) executed on the CPU by the SIMT emulator: tests/resample_cases.py at every rate
pair, length and format against scipy's float64 resampler, inside the derived fp32 bound."""
import pytest

from tests import resample_cases as R
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("rate_from,rate_to", R.RATE_PAIRS)
def test_rate_pair_within_derived_bound(ops, rate_from, rate_to):
    worst = R.check_rate_pair(ops, "cpu", rate_from, rate_to)
    print(f"{rate_from} -> {rate_to}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_both_tap_paths_give_the_fma_chain_bits(ops):
    R.check_fma_chain_bits(ops, "cpu")


def test_decode_only_is_load_audio_bit_for_bit(ops, tmp_path):
    R.check_decode_only(ops, "cpu", tmp_path)


def test_loader_matches_host_loader(ops, tmp_path):
    for path in R.write_wavs(tmp_path, 44100, frames=3000):
        R.check_loader_against_host(ops, "cpu", path)
