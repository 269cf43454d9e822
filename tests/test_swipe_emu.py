"""The SWIPE' F0 extractor's kernels (csrc/swipe.hip), stage (svcmi_swipe_f0_fwd) and drop-ins (svcmi.pitch.core.swipe_slim,
svcmi.pitch.compute_f0_swipe, svc_inference --f0 swipe) executed on the CPU by the SIMT emulator: the checks of tests/swipe_cases.py.

The emulator runs about a million lane-steps a second, and ONE frame tile of the production geometry (six windows up to 2048) is ten
million: the shape checks therefore run in a small geometry whose tiles all have ragged edges (Fs 4000, 100 .. 800 Hz, R 50: four windows
32 .. 256, 72 candidates, 104 log-frequency bins, table widths 17 .. 129) and in a two-window geometry that reaches the magnitude
kernel's global-memory form (512 and 1024); the production geometry runs once, through the command line on a two-frame cut of 035.wav.
The whole clips against the reference's record are tests/test_gpu_swipe.py's; here the record is checked against the float64 programme,
and the programme against the device at the small shapes.  Where the reference checkout is present, the programme is proven equal to it."""
import os

import numpy as np
import pytest
import torch

from tests import swipe_cases as C
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


def test_golden_record_is_the_float64_programme():
    C.check_golden_is_the_programme()


def test_kernels_one_by_one_small_geometry(ops):
    C.check_kernels(ops, "cpu", C.SMALL, n=333)


def test_kernels_one_by_one_global_memory_form(ops):
    C.check_kernels(ops, "cpu", C.MID, n=900)


def test_stage_shapes(ops):
    C.check_stage_shapes(ops, "cpu", C.SMALL)


def test_silence_is_f_min_with_confidence_zero(ops):
    C.check_silence(ops, "cpu", C.SMALL)


def test_arg_max_at_the_last_candidate(ops):
    C.check_last_candidate(ops, "cpu")


def test_arg_max_at_candidate_zero_wraps(ops):
    C.check_wrap(ops, "cpu")


def test_exact_ties_take_the_lowest_index(ops):
    C.check_ties(ops, "cpu")


def test_stage_bits_do_not_depend_on_the_launch(ops):
    C.check_repeatable(ops, "cpu")


def test_swipe_slim_returns_what_the_reference_returns(ops):
    C.check_api(ops, "cpu", C.SMALL, C.tone(500, 230.0, 4000, seed=9))


def test_extract_features_takes_swipe_without_a_crepe_model(ops, monkeypatch):
    """extract_features(..., f0="swipe") never touches ``crepe`` (None here) and passes the threshold on; the recipe is stubbed (the
    command-line test below runs it)."""
    from svcmi import svc_inference as SI
    from svcmi.hubert import inference as hubert_inf
    from svcmi.pitch import inference as pitch_inf
    from svcmi.whisper import inference as whisper_inf
    monkeypatch.setattr(whisper_inf, "ppg_from_audio", lambda m, a: "ppg")
    monkeypatch.setattr(hubert_inf, "units_windowed", lambda m, a: "vec")
    monkeypatch.setattr(pitch_inf, "compute_f0_swipe_begin", lambda a, dev, strength_threshold=0.0, ops=None: lambda: ("f0", strength_threshold, ops))
    assert SI.extract_features(np.zeros(8, np.float32), None, None, None, "cpu", f0="swipe", ops=ops, swipe_threshold=0.25) == ("ppg", "vec", ("f0", 0.25, ops))
    assert "swipe" in SI.F0_CHOICES


def test_command_line_with_swipe_never_opens_the_crepe_checkpoint(ops, tmp_path, monkeypatch):
    """svc_inference.main with --f0 swipe, the tiny seeded models and a --crepe path that does not exist, on the first 600 samples of
    035.wav (two frames: the emulator's budget): svc_tmp.pit.csv holds the recipe's track -- the float64 programme's, a value within the
    f0 tolerance of its integer part --; then, with only --pit missing, ``--swipe-threshold`` reaches the recipe.  The F0 extractor runs on the emulator in the
    production geometry; the two network extractors and the synthesizer are replaced by stand-ins of the right shapes
    (tests/test_gpu_swipe.py runs the same command on the whole clip with nothing replaced)."""
    from svcmi import svc_inference as SI
    from svcmi.hubert import inference as hubert_inf
    from svcmi.whisper import inference as whisper_inf
    x = C.prepare_cli_files(tmp_path, monkeypatch, n=600)
    pl = C.plan("cpu")
    S = C.strength_ref(x, pl)
    f0, conf, _, _ = C.finish_ref(S, pl, edge="clamp")
    want, tol = np.repeat(f0, 2), np.repeat(C.f0_sensitivity(S, pl) + 1e-9 * f0, 2)
    hp = SI.load_config("cfg.yaml")
    monkeypatch.setattr(whisper_inf, "ppg_from_audio", lambda m, a: torch.zeros(2, hp.vits.ppg_dim))
    monkeypatch.setattr(hubert_inf, "units_windowed", lambda m, a: torch.zeros(2, hp.vits.vec_dim))
    seen = []

    def synth(model, retrieval, spk, pit, ppg, vec, hp_, device, **kw):
        seen.append(pit.numpy().copy())
        return np.zeros(8, np.float32)
    monkeypatch.setattr(SI, "svc_infer", synth)
    SI.main(SI.build_parser().parse_args(C.CLI_ARGS), device="cpu", ops=ops)
    first = C.check_csv("svc_tmp.pit.csv", want, tol)
    assert first.shape == (4,) and bool((first > 0).all()) and float(conf.min()) < 0.9 < 1.0
    os.remove("svc_tmp.pit.csv")
    # with only --pit missing the command calls the recipe itself; a second run of the production geometry would double the test's
    # time, so the recipe is replaced by a recorder here: the wave, the device, the threshold and the library must reach it
    from svcmi.pitch import inference as pitch_inf
    calls = []
    monkeypatch.setattr(pitch_inf, "compute_f0_swipe", lambda *a, **k: (calls.append((a, k)), np.array([0.0, 101.7, 0.0, 99.2]))[1])
    SI.main(SI.build_parser().parse_args(C.CLI_ARGS + ["--ppg", "svc_tmp.ppg.npy", "--vec", "svc_tmp.vec.npy", "--swipe-threshold", "0.25"]),
            device="cpu", ops=ops)
    assert calls == [(("in.wav", "cpu"), dict(strength_threshold=0.25, ops=ops))]
    assert C.check_csv("svc_tmp.pit.csv", np.array([0.0, 101.0, 0.0, 99.0])).tolist() == [0.0, 101.0, 0.0, 99.0]
    assert len(seen) == 2 and np.array_equal(seen[0], first.astype(np.float32)) and seen[1].tolist() == [0.0, 101.0, 0.0, 99.0]


# ------------------------------------------------------------------------------------------------ the programme against the reference
@pytest.mark.needs_reference
def test_programme_equals_the_reference():
    """``strength_ref`` against the reference's own S (captured inside ``swipe_slim``) to 1e-13 and ``finish_ref`` on that S against the
    reference's f0 and conf bit for bit, on the glide and in the small geometry (a harmonic tone); the reference's IndexError on 010."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_swipe_golden", os.path.join(root, "scripts", "make_swipe_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ref = mod.load_reference("/root/reference")
    for geo, x in ((C.P, C.clip("glide")), (C.SMALL, C.tone(700, 230.0, 4000, seed=1))):
        pl = C.plan("cpu", geo)
        (f0, t, conf), S = mod.run_reference(ref, x, geo, np.float64)
        assert float(np.abs(C.strength_ref(x, pl) - S).max()) <= 1e-13
        mine = C.finish_ref(S, pl, edge="raise")
        assert np.array_equal(mine[0].view(np.int64), f0.view(np.int64)) and np.array_equal(mine[1].view(np.int64), conf.view(np.int64))
    err, S = mod.run_reference(ref, C.clip("010"), C.P, np.float64)
    assert isinstance(err, IndexError) and str(err) == "index 635 is out of bounds for axis 0 with size 635"
    assert np.array_equal(C.finish_ref(S, C.plan("cpu"), edge="clamp")[2], C.golden()["amax_010"])
