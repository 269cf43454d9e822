"""Regenerate tests/golden/salience_f0.npz from the reference checkout:

    python scripts/make_salience_golden.py /path/to/reference/checkout

Runs only where the reference is present, never on the GPU machine.  It imports the reference's ``pitch/core/salience.py`` BY PATH and runs
``salience`` with the parameters of ``compute_f0_salience`` (pitch/inference.py:31-44) plus that function's tail (x2 repeat, 3-point moving
average).  The module's two imports that are not installed here are replaced by small stand-ins written below:

  librosa.stft   zero centre padding by n_fft / 2, ``scipy.signal.get_window('hann', N, fftbins=True)``, fp32 frames, ``scipy.fft.rfft``
                 (complex64 for an fp32 signal, like librosa's)
  numba.njit     the identity

Inputs: tests/golden/035.wav, tests/golden/vad_010.wav and a seeded 2 s glide made by ``glide()`` below (stored in the file too: its bits
then do not depend on the libm of the machine that runs the tests).  Per input ``<name>``:

  path_<name>    the trajectory's bin indices, int16 [frames]
  track_<name>   the final compute_f0_salience track, float64 [2 frames]
  sal_<name>     salience of the chosen bin over its column's maximum, float64 [frames]
  zmax_<name>    max(Z)
  zcols_<name>   columns ZCOLS of Z, float64 [len(ZCOLS), B] (time-major rows)
  wave_glide     the glide, float32

Only data goes into the file.  The script ASSERTS, per input, that the reference's path is identical in three variants -- the STFT made in
float64, the STFT made in fp32, and Z rounded to fp32 before the dynamic programme -- which is what makes "equal in every frame" a fair
demand on an fp32 device path; an input that fails is to be replaced, not tolerated."""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy.fft
import scipy.signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PARAMS = dict(Fs=16000, H=320, N=2048, F_min=45.0, F_max=1760.0)
ZCOLS = (0, 1, 50, 100)
WAVS = {"035": "035.wav", "010": "vad_010.wav"}
STFT_DTYPE = [np.float32]          # what the stand-in computes in (switched for the float64 variant)


def glide(seed=7, seconds=2.0, fs=16000):
    """110 Hz rising 1.5 octaves over the clip, six harmonics at 0.6^h, plus 0.003 N(0, 1); scaled by 0.2."""
    n = int(seconds * fs)
    t = np.arange(n) / fs
    f = 110.0 * 2.0 ** (1.5 * t / seconds)
    phase = 2.0 * np.pi * np.cumsum(f) / fs
    x = sum(0.6 ** h * np.sin((h + 1) * phase) for h in range(6))
    x = 0.2 * x + 0.003 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)


def stft(x, n_fft=2048, hop_length=None, win_length=None, pad_mode="constant"):
    assert pad_mode == "constant" and win_length == n_fft
    dt = STFT_DTYPE[0]
    xp = np.pad(np.asarray(x, dtype=dt), n_fft // 2)
    frames = 1 + len(x) // hop_length
    idx = np.arange(n_fft)[None, :] + hop_length * np.arange(frames)[:, None]
    win = scipy.signal.get_window("hann", n_fft, fftbins=True).astype(dt)
    return scipy.fft.rfft(xp[idx] * win, axis=1).T          # [bins, frames]; complex64 for fp32 frames


def load_reference(ref_root):
    lib = types.ModuleType("librosa")
    lib.stft = stft
    nb = types.ModuleType("numba")
    nb.njit = lambda f: f
    saved = {k: sys.modules.get(k) for k in ("librosa", "numba")}
    sys.modules.update(librosa=lib, numba=nb)
    try:
        spec = importlib.util.spec_from_file_location("ref_salience", os.path.join(ref_root, "pitch", "core", "salience.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def load_wav(name):
    from scipy.io import wavfile
    rate, x = wavfile.read(os.path.join(GOLDEN, name))
    assert rate == 16000 and x.dtype == np.int16 and x.ndim == 1
    return x.astype(np.float32) / 32768.0


def rep_and_path(mod, x, dtype, round_z=False):
    STFT_DTYPE[0] = dtype
    try:
        Z, F = mod.compute_salience_rep(x.astype(dtype), PARAMS["Fs"], N=PARAMS["N"], H=PARAMS["H"], F_min=PARAMS["F_min"], F_max=PARAMS["F_max"],
                                        R=10.0, num_harm=10, freq_smooth_len=11, alpha=0.9, gamma=0.0)
    finally:
        STFT_DTYPE[0] = np.float32
    Zd = Z.astype(np.float32).astype(np.float64) if round_z else Z
    T_coef = (np.arange(Z.shape[1]) * PARAMS["H"]) / PARAMS["Fs"]
    return Z, mod.compute_trajectory_cr(Zd, T_coef, F, None, tol=5, score_low=0.01, score_high=1.0)


def main(ref_root):
    mod = load_reference(ref_root)
    inputs = {name: load_wav(f) for name, f in WAVS.items()}
    inputs["glide"] = glide()
    out = {"wave_glide": inputs["glide"], "zcols": np.array(ZCOLS, dtype=np.int32)}
    for name, x in inputs.items():
        with np.errstate(divide="ignore", invalid="ignore"):
            f0, t, sal = mod.salience(x, **PARAMS)
            Z32, p32 = rep_and_path(mod, x, np.float32)
            Z64, p64 = rep_and_path(mod, x, np.float64)
            _, p32r = rep_and_path(mod, x, np.float32, round_z=True)
        assert f0.shape == (1 + len(x) // PARAMS["H"],)
        differ = (int((p32 != p64).sum()), int((p32 != p32r).sum()))
        dev = float(np.abs(Z32 - Z64).max() / Z64.max())
        print(f"{name}: {len(f0)} frames, path differs in {differ[0]} (fp64 STFT) / {differ[1]} (fp32 Z) frames, Z fp32 vs fp64 {dev:.2e} of max Z")
        assert differ == (0, 0), f"{name}: the reference's own path is not stable under fp32 rounding -- replace this input"
        assert np.array_equal(f0, (PARAMS["F_min"] * np.power(2, (np.arange(0, Z32.shape[0]) * 10.0 / 1200)))[p32])
        track = np.convolve(np.repeat(f0, 2, -1), np.ones((3,)) / 3, mode="same")          # pitch/inference.py:42-43
        out[f"path_{name}"] = p32.astype(np.int16)
        out[f"track_{name}"] = track.astype(np.float64)
        out[f"sal_{name}"] = sal.astype(np.float64)
        out[f"zmax_{name}"] = np.float64(Z32.max())
        out[f"zcols_{name}"] = np.ascontiguousarray(Z32[:, list(ZCOLS)].T)
    path = os.path.join(GOLDEN, "salience_f0.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SVCMI_REFERENCE", ""))
