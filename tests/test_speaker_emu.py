"""The speaker encoder's kernels (csrc/lstm.hip) and stage (svcmi_speaker_encoder_fwd) executed on the CPU by the SIMT emulator:
tests/speaker_cases.py -- the step kernel at every small shape, its numeric edges, the encoder at tiny dimensions, the fixture made by
the reference's own class, and the mel front-end."""
import pytest

from tests import speaker_cases as S
from tests.emu import emu_ops
from workload import speaker as WS


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("H", S.STEP_H)
def test_step_kernel_shapes(ops, H):
    S.check_step_shapes(ops, "cpu", H)


def test_step_kernel_saturation(ops):
    S.check_saturation(ops, "cpu")


def test_step_kernel_exact_cell_growth(ops):
    S.check_exact_cell_growth(ops, "cpu")


def test_step_kernel_batch_independence_and_repeatability(ops):
    S.check_batch_independence(ops, "cpu")


@pytest.mark.parametrize("B,T", [(3, 7), (17, 33)])
def test_encoder_tiny(ops, B, T):
    S.check_encoder(ops, "cpu", WS.TINY, B, T)


def test_compute_embedding_offsets_and_short_clip(ops):
    S.check_compute_embedding(ops, "cpu")


def test_fixture_of_the_reference_class(ops, golden_dir, tmp_path):
    S.check_golden(ops, "cpu", golden_dir, tmp_path)


@pytest.mark.parametrize("n", [1024, 4000])
def test_mel_against_float64(ops, n):
    S.check_mel(ops, "cpu", n)


def test_mel_edges(ops):
    S.check_mel_edges(ops, "cpu")


def test_preemphasis_edge(ops):
    S.check_preemphasis(ops, "cpu")


def test_trim_and_sound_norm(ops):
    S.check_trim_and_norm(ops, "cpu")


def test_wrong_architecture_raises(ops):
    from svcmi._lib import SvcmiError
    from svcmi.speaker.models.lstm import LSTMSpeakerEncoder
    with pytest.raises(SvcmiError):
        LSTMSpeakerEncoder(12, 20, 40, 3, use_lstm_with_projection=False, device="cpu", ops=ops)
