"""The voice-activity detector's kernels (csrc/vad.hip), stage (svcmi_vad_probs_fwd) and drop-ins (svcmi.vad, svcmi.svc_inference_post)
executed on the CPU by the SIMT emulator: the checks of tests/vad_cases.py."""
import os

import pytest
import torch

from tests import vad_cases as V
from tests.emu import emu_ops

REF_JIT = "/root/reference/vad/assets/silero_vad.jit"


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("W", [1, 2, 125])
def test_frontend_against_float64(ops, W):
    V.check_frontend_windows(ops, "cpu", W)


def test_frontend_edges(ops):
    V.check_frontend_edges(ops, "cpu")


def test_frontend_bits_do_not_depend_on_the_launch(ops):
    V.check_frontend_bits(ops, "cpu")


@pytest.mark.parametrize("W", [1, 2, 135])
def test_scan_against_float64(ops, W):
    V.check_scan_lengths(ops, "cpu", W)


def test_scan_ragged_batch_and_repeatability(ops):
    V.check_scan_ragged_and_repeat(ops, "cpu")


def test_scan_state_carry(ops):
    V.check_scan_state_carry(ops, "cpu")


def test_scan_saturation(ops):
    V.check_scan_saturation(ops, "cpu")


def test_scan_exact_cell_growth(ops):
    V.check_scan_exact_cell_growth(ops, "cpu")


@pytest.mark.parametrize("name", ["035", "010"])
def test_probabilities_end_to_end(ops, name):
    V.check_probs_clip(ops, "cpu", name)


def test_batched_forward_and_decimation(ops):
    V.check_batched_forward(ops, "cpu")


def test_call_keeps_the_state_between_windows(ops):
    V.check_call_keeps_state(ops, "cpu")


def test_spans_equal_the_reference(ops):
    V.check_spans(ops, "cpu")


def test_mask(ops):
    V.check_mask(ops, "cpu")


def test_apply_vad_post(ops):
    V.check_apply_vad_post(ops, "cpu")


def test_post_command_line(ops, tmp_path):
    V.check_post_cli(ops, "cpu", tmp_path)


def test_model_rejects_what_it_does_not_support(ops):
    vad = V.model(ops, "cpu")
    with pytest.raises(ValueError, match="8 kHz"):
        vad(torch.zeros(256), 8000)
    with pytest.raises(ValueError, match="512"):
        vad(torch.zeros(1024), 16000)
    with pytest.raises(ValueError, match="512"):
        vad.audio_forward(torch.zeros(4096), 16000, num_samples=1024)
    with pytest.raises(ValueError):
        vad(torch.zeros(1, 1, 512), 16000)


@pytest.mark.skipif(not os.path.exists(REF_JIT), reason="the reference's silero_vad.jit is not present")
def test_init_jit_model_reads_the_archive(ops):
    """The tensors taken out of the TorchScript archive are the fixture's, and the model made from them gives the fixture's spans."""
    from svcmi.vad.utils import get_speech_timestamps, init_jit_model
    vad = init_jit_model(REF_JIT, "cpu", ops=ops)
    sd = V.real_sd()
    w = vad.weights
    assert torch.equal(w.basis_t[:, :258].t(), sd["feature_extractor.forward_basis_buffer"][:, 0])
    assert torch.equal(w.whh1_t.t(), sd["decoder.rnn.weight_hh_l1"]) and torch.equal(w.blocks[3]["pw_w"], sd["encoder.11.0.pw_conv.0.weight"][:, :, 0])
    got = get_speech_timestamps(V.clip("035"), vad, threshold=0.2)
    assert [(t["start"], t["end"]) for t in got] == V.fixture_spans("035", 0.2)
