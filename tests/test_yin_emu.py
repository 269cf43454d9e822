"""The YIN F0 extractor's kernels (csrc/yin.hip), stage (svcmi_yin_f0_fwd) and drop-ins (svcmi.pitch.core.yin,
svcmi.pitch.compute_f0_yin) executed on the CPU by the SIMT emulator: the checks of tests/yin_cases.py.  Where the reference checkout is
present, the float64 programme of the case file is proven equal to it bit for bit."""
import os

import pytest

from tests import yin_cases as C
from tests.emu import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("T", [2, 3, 33])
def test_cmndf_rows_hold_the_bits_of_pyin(ops, T):
    C.check_cmndf_equals_pyin(ops, "cpu", T)


@pytest.mark.parametrize("T", [2, 3, 33])
def test_cmndf_rows_hold_the_bits_of_pyin_smallest_geometry(ops, T):
    C.check_cmndf_equals_pyin(ops, "cpu", T, small=True)


def test_cmndf_of_a_single_frame(ops):
    C.check_cmndf_one_frame(ops, "cpu")


def test_pick_from_built_rows(ops):
    C.check_pick_built(ops, "cpu")


def test_pick_with_a_single_lag(ops):
    C.check_pick_single_lag(ops, "cpu")


def test_pick_from_the_golden_rows(ops):
    C.check_pick_golden(ops, "cpu")


@pytest.mark.parametrize("small", [False, True])
def test_aperiodicity_against_longdouble(ops, small):
    C.check_ap_lags(ops, "cpu", small=small)


def test_aperiodicity_of_silence_is_exactly_zero(ops):
    C.check_ap_silence(ops, "cpu")


def test_aperiodicity_of_short_clips(ops):
    C.check_ap_short_clips(ops, "cpu")


def test_aperiodicity_bits_do_not_depend_on_the_launch(ops):
    C.check_ap_bits(ops, "cpu")


@pytest.mark.parametrize("name", C.CLIPS)
def test_end_to_end_equals_the_reference(ops, name):
    C.check_end_to_end(ops, "cpu", name)


def test_yin_returns_what_the_reference_returns(ops):
    C.check_yin_api(ops, "cpu")


def test_compute_f0_yin(ops):
    C.check_compute_f0_yin(ops, "cpu")


def test_edges(ops):
    C.check_edges(ops, "cpu")


# ------------------------------------------------------------------------------------------------ the programme against the reference
def _script():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_yin_golden", os.path.join(root, "scripts", "make_yin_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.needs_reference
def test_programme_equals_the_reference_on_every_frame_of_the_golden_clips():
    """The CMNDF rows, both lags with their types, f0 and ap of every frame: the case file's float64 programme against the reference's own
    ``yin``, bit for bit, on the three clips and on seeded noise and tone frames; the stored track is the reference's; and the two
    exceptions carry the reference's texts."""
    from svcmi.pitch.core.yin import yin
    script = _script()
    tap = script.Tap(script.load_reference("/root/reference"))
    g = C.golden()
    noise = script.seeded_frames(C)
    script.compare(C, tap.run(noise, C.P), C.yin_ref(noise), "seeded frames")
    for name in C.CLIPS:
        x = C.clip(name)
        ref = tap.run(x, C.P)
        script.compare(C, ref, C.yin_ref(x), name)
        assert C.same_bits(ref["f0"], g[f"f0_{name}"]) and C.same_bits(ref["ap"], g[f"ap_{name}"])
    for bad in (dict(F_min=2000.0), dict(F_min=5.0)):
        texts = []
        for fn, extra in ((tap.mod.yin, {}), (yin, dict(device="cpu", ops=emu_ops()))):
            with pytest.raises(Exception) as e:
                fn(C.clip("glide"), **{**C.P, **bad}, **extra)
            texts.append(str(e.value))
        assert texts[0] == texts[1] and "F_min" in texts[0]
