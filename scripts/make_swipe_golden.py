"""Regenerate tests/golden/swipe_f0.npz from the reference checkout:

    python scripts/make_swipe_golden.py /path/to/reference/checkout

Runs only where the reference is present, never on the GPU machine.  It imports the reference's ``pitch/core/swipe_slim.py`` BY PATH (with
``yin.py`` beside it) and runs ``swipe_slim`` with the parameters of ``compute_f0_swipe`` (Fs 16000, H 320, 45 .. 1760 Hz, R 10).  Stand-ins
for what is not installed here, in the convention of scripts/make_salience_golden.py:

  librosa.stft   zero centre padding by n_fft / 2, ``scipy.signal.get_window('hann', N, fftbins=True)``, ``scipy.fft.rfft``; computed in
                 fp32 (complex64, like librosa's for an fp32 signal) or in float64 (the variant)
  numba.njit     the identity (yin.py decorates with it)
  np.bool8       ``np.bool_`` (numpy 2 dropped the alias ``prime_and_one`` uses)

S is a local of ``swipe_slim``; it is captured by handing the module a numpy proxy whose ``argmax`` keeps its argument.

Inputs: tests/golden/035.wav, tests/golden/vad_010.wav and ``make_salience_golden.glide()`` (stored in the file too).  Per input ``<name>``:

  amax_<name>     the arg-max per frame, int16 [frames]
  f0_<name>       float64 [frames]
  conf_<name>     float64 [frames]
  S_<name>        the columns SCOLS of S, float64 [len(SCOLS), B] (time-major rows)
  rival_<name>    per frame the winner minus the best other local maximum of the column, float64 [frames]
  f0sens_<name>   per frame the largest |f0' - f0| over the 8 sign patterns of +-1e-5 on the three S values the parabola reads
  wave_glide      the glide, float32

For 035 and glide f0 / conf are what the reference returned.  For 010 the reference raises ``IndexError: index 635 is out of bounds for
axis 0 with size 635`` (its arg-max sits at the last candidate in some frames): the record is made from the captured S with the clamp
rule (shift 0 in those frames) by ``tests/swipe_cases.finish_ref``, which the other two inputs prove equal to the reference's tail.

Only data goes into the file.  The script ASSERTS, per input,
  * ``swipe_cases.strength_ref`` (the float64 programme on the plan's tables: W_N from the identity through ``interp1d``) equals the
    reference's S to 1e-13;
  * ``swipe_cases.finish_ref`` on the reference's S returns the reference's f0 and conf bit for bit (035, glide), and raises the
    reference's IndexError with its message under ``edge="raise"`` (010);
  * the reference's own arg-max is the same in every frame with an fp32 and with a float64 STFT;
  * every ``rival`` is at least 2e-5 (twice the bar the device's S is held to).
An input that fails is to be replaced, not tolerated."""
import importlib
import os
import sys
import types

import numpy as np
import scipy.fft
import scipy.signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "whisper-vits-svc_amd"), os.path.join(ROOT, "scripts")]
GOLDEN = os.path.join(ROOT, "tests", "golden")
WAVS = {"035": "035.wav", "010": "vad_010.wav"}
STFT_DTYPE = [np.float32]


def stft(x, n_fft=2048, hop_length=None, win_length=None, window="hann", pad_mode="constant", center=True):
    assert pad_mode == "constant" and win_length == n_fft and window == "hann" and center
    dt = STFT_DTYPE[0]
    xp = np.pad(np.asarray(x, dtype=dt), n_fft // 2)
    frames = 1 + len(x) // hop_length
    idx = np.arange(n_fft)[None, :] + hop_length * np.arange(frames)[:, None]
    win = scipy.signal.get_window("hann", n_fft, fftbins=True).astype(dt)
    return scipy.fft.rfft(xp[idx] * win, axis=1).T          # [bins, frames]; complex64 for fp32 frames


class NumpyTap:
    """numpy, except that ``argmax`` keeps its argument: swipe_slim's S."""

    def __init__(self):
        self.S = None

    def __getattr__(self, name):
        return getattr(np, name)

    def argmax(self, a, axis=None):
        self.S = np.array(a)
        return np.argmax(a, axis=axis)


def load_reference(ref_root):
    """The reference's swipe_slim module, imported as ``ref_pitch_core.swipe_slim`` from a synthetic package that points at pitch/core."""
    if not hasattr(np, "bool8"):
        np.bool8 = np.bool_
    lib = types.ModuleType("librosa")
    lib.stft = stft
    nb = types.ModuleType("numba")
    nb.njit = lambda f: f
    pkg = types.ModuleType("ref_pitch_core")
    pkg.__path__ = [os.path.join(ref_root, "pitch", "core")]
    saved = {k: sys.modules.get(k) for k in ("librosa", "numba")}
    sys.modules.update(librosa=lib, numba=nb, ref_pitch_core=pkg)
    try:
        mod = importlib.import_module("ref_pitch_core.swipe_slim")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    mod.np = NumpyTap()
    return mod


def run_reference(mod, x, params, dtype=np.float32):
    """(f0, t, conf) or the IndexError the reference raised, and its S."""
    STFT_DTYPE[0] = dtype
    try:
        try:
            out = mod.swipe_slim(x.astype(dtype), **params)
        except IndexError as e:
            out = e
    finally:
        STFT_DTYPE[0] = np.float32
    return out, mod.np.S


def load_wav(name):
    from scipy.io import wavfile
    rate, x = wavfile.read(os.path.join(GOLDEN, name))
    assert rate == 16000 and x.dtype == np.int16 and x.ndim == 1
    return x.astype(np.float32) / 32768.0


def main(ref_root):
    from make_salience_golden import glide
    from tests import swipe_cases as C
    from svcmi.pitch.core.swipe_slim import Plan
    mod = load_reference(ref_root)
    pl = Plan(device="cpu", strength_threshold=0, **C.P)
    inputs = {name: load_wav(f) for name, f in WAVS.items()}
    inputs["glide"] = glide()
    out = {"wave_glide": inputs["glide"], "scols": np.array(C.SCOLS, dtype=np.int32)}
    for name, x in inputs.items():
        res, S32 = run_reference(mod, x, C.P, np.float32)
        res64, S64 = run_reference(mod, x, C.P, np.float64)
        assert S32.shape == (pl.B, -(-len(x) // C.P["H"]))
        mine = C.strength_ref(x, pl)
        e_prog = float(np.abs(mine - S64).max())
        a32, a64 = np.argmax(S32, axis=0), np.argmax(S64, axis=0)
        edge = int((a64 == pl.B - 1).sum())
        rival = C.rival_gap(S64)
        print(f"{name}: {S64.shape[1]} frames, programme vs reference S {e_prog:.2e}, fp32 vs fp64 STFT S {np.abs(S32 - S64).max():.2e}, arg-max "
              f"differs in {int((a32 != a64).sum())} frames, {edge} frames at the last candidate, smallest rival gap {rival.min():.2e}")
        assert e_prog <= 1e-13, f"{name}: the float64 programme is not the reference"
        assert np.array_equal(a32, a64), f"{name}: the reference's own arg-max is not stable under an fp32 STFT -- replace this input"
        assert rival.min() >= 2e-5, f"{name}: a rival peak within 2e-5 of the winner -- replace this input"
        if isinstance(res64, IndexError):
            assert edge > 0 and str(res64) == f"index {pl.B} is out of bounds for axis 0 with size {pl.B}"
            try:
                C.finish_ref(S64, pl, edge="raise")
            except IndexError as e:
                assert str(e) == str(res64)
            else:
                raise AssertionError("finish_ref did not raise")
            f0, conf, amax, _ = C.finish_ref(S64, pl, edge="clamp")
        else:
            assert edge == 0
            f0, conf, amax, _ = C.finish_ref(S64, pl, edge="raise")
            assert np.array_equal(f0.view(np.int64), res64[0].view(np.int64)) and np.array_equal(conf.view(np.int64), res64[2].view(np.int64)), \
                f"{name}: finish_ref is not the reference's tail"
            assert np.array_equal(res64[1], np.arange(0, len(x), C.P["H"]) / C.P["Fs"])
        assert np.array_equal(amax, a64)
        out[f"amax_{name}"] = amax.astype(np.int16)
        out[f"f0_{name}"] = f0
        out[f"conf_{name}"] = conf
        out[f"S_{name}"] = np.ascontiguousarray(S64[:, list(C.SCOLS)].T)
        out[f"rival_{name}"] = rival
        out[f"f0sens_{name}"] = C.f0_sensitivity(S64, pl)
    path = os.path.join(GOLDEN, "swipe_f0.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SVCMI_REFERENCE", ""))
