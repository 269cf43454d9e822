"""Regenerate tests/golden/pyin_f0.npz from the reference checkout:

    python scripts/make_pyin_golden.py /path/to/reference/checkout

Runs only where the reference is present, never on the GPU machine.  It imports the reference's ``pitch/core/pyin.py`` BY PATH (with
``yin.py`` beside it) and runs ``pyin`` with the parameters of ``compute_f0_pyin`` (Fs 16000, N 2048, H 320, 45 .. 1760 Hz).  ``numba.njit``
is replaced by the identity: the reference then executes under plain numpy, which is the behaviour the device path reproduces.

Inputs: tests/golden/035.wav, tests/golden/vad_010.wav and ``make_salience_golden.glide()`` (stored in the file too).  Per input ``<name>``:

  path_<name>      the decoded states, int16 [frames] (< B voiced, >= B unvoiced)
  f0_<name>        the refined track in Hz, 0 where unvoiced, float64 [frames]
  conf_<name>      float64 [frames]
  rms_<name>       float64 [frames]
  cmndf_<name>     the CMNDF rows of the frames ROWS, float64 [len(ROWS), p_max + 1]
  O_<name>         the matching observation columns (after normalisation), float64 [len(ROWS), 2B]
  lag_thr_<name>, val_thr_<name>    float64 [len(ROWS), 99]
  f0sens_<name>    the largest |f0' - f0| per frame over the 8 runs of perturbation (a), float64 [frames]
  wave_glide       the glide, float32

Only data goes into the file.  The script ASSERTS, per input,
  * that the float64 programme of tests/pyin_cases.py equals the reference bit for bit: O, lag_thr and val_thr of EVERY frame (NaN
    positions included) plus 40 seeded noise frames, the path, f0 and conf;
  * that the reference's own path, voicing and conf are unchanged (a) when the CMNDF is multiplied elementwise by 1 + DELTA u, u uniform in
    [-1, 1], over 8 seeds -- DELTA is the relative bound derived for the CMNDF kernel -- and (b) when O is multiplied by 1 + 1e-12 u, per
    element in the voiced half and per frame in the unvoiced half;
  * that no rms lies within 1e-6 of the 0.01 threshold.
An input that fails is to be replaced, not tolerated."""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "whisper-vits-svc_amd"), os.path.join(ROOT, "scripts")]
GOLDEN = os.path.join(ROOT, "tests", "golden")
WAVS = {"035": "035.wav", "010": "vad_010.wav"}
SEEDS = 8


def load_reference(ref_root):
    """The reference's pyin module, imported as ``ref_pitch_core.pyin`` from a synthetic package that points at pitch/core."""
    nb = types.ModuleType("numba")
    nb.njit = lambda f: f
    pkg = types.ModuleType("ref_pitch_core")
    pkg.__path__ = [os.path.join(ref_root, "pitch", "core")]
    saved = sys.modules.get("numba")
    sys.modules.update(numba=nb, ref_pitch_core=pkg)
    try:
        return importlib.import_module("ref_pitch_core.pyin")
    finally:
        if saved is None:
            sys.modules.pop("numba", None)
        else:
            sys.modules["numba"] = saved


def load_wav(name):
    from scipy.io import wavfile
    rate, x = wavfile.read(os.path.join(GOLDEN, name))
    assert rate == 16000 and x.dtype == np.int16 and x.ndim == 1
    return x.astype(np.float32) / 32768.0


class Tap:
    """Wraps the reference's CMNDF and yin_multi_thr: remembers the unperturbed CMNDF rows (they cost most of a run), multiplies them or
    O by a given factor, and keeps what yin_multi_thr returned."""

    def __init__(self, mod):
        self.mod, self.cm, self.cm_scale, self.o_scale, self.frame, self.last = mod, {}, None, None, 0, None
        self.cmndf0, self.multi0 = mod.cumulative_mean_normalized_difference_function, mod.yin_multi_thr
        mod.cumulative_mean_normalized_difference_function = self.cmndf
        mod.yin_multi_thr = self.multi

    def cmndf(self, frame, lag_max):
        key = (frame.tobytes(), lag_max)
        if key not in self.cm:
            self.cm[key] = self.cmndf0(frame, lag_max)
        c = self.cm[key].copy()
        if self.cm_scale is not None:
            c = c * self.cm_scale[self.frame]
        self.frame += 1
        return c

    def multi(self, *a, **k):
        self.frame = 0
        O, rms, p, v = self.multi0(*a, **k)
        if self.o_scale is not None:
            O = O * self.o_scale
        self.last = (O.copy(), rms.copy(), p.copy(), v.copy())
        return O, rms, p, v

    def run(self, x, params, cm_scale=None, o_scale=None):
        self.cm_scale, self.o_scale = cm_scale, o_scale
        with np.errstate(divide="ignore", invalid="ignore"):
            f0, t, conf = self.mod.pyin(x, **params)
        return f0, conf, self.last


def main(ref_root):
    from make_salience_golden import glide
    from tests import pyin_cases as C
    mod = load_reference(ref_root)
    tap = Tap(mod)
    pl = C.plan("cpu")
    B, nt, width = pl.B, len(pl.thresholds_np), pl.p_max + 1
    inputs = {name: load_wav(f) for name, f in WAVS.items()}
    inputs["glide"] = glide()
    out = {"wave_glide": inputs["glide"], "rows": np.array(C.ROWS, dtype=np.int32)}

    # the thresholding on seeded noise frames (white noise at three levels, a 50 Hz tone): programme == reference
    rng = np.random.default_rng(2024)
    for k in range(40):
        fr = rng.standard_normal(C.P["N"]) * (10.0 ** -rng.integers(0, 4)) if k % 4 else np.sin(2 * np.pi * 50.0 * np.arange(C.P["N"]) / 16000 + k)
        c = tap.cmndf0(fr.astype(np.float32).astype(np.float64), pl.p_max)
        with np.errstate(divide="ignore", invalid="ignore"):
            Om, lag, val = mod.probabilistic_thresholding(c.copy(), pl.thresholds_np, pl.p_min, pl.p_max, 0.01, pl.F_axis, 16000, pl.beta_np)
        mine = C.observe_frame(c, pl.thresholds_np, pl.beta_np, pl.p_min, pl.p_max, 0.01, pl.F_axis, 16000)
        assert C.same_bits(Om[:B], mine[0]) and not Om[B:].any() and C.same_bits(lag, mine[1]) and C.same_bits(val, mine[2]), k

    for name, x in inputs.items():
        f0, conf, (O, rms, lag, val) = tap.run(x, C.P)
        T = len(f0)
        assert T == 1 + len(x) // C.P["H"] and O.shape == (2 * B, T)
        with np.errstate(divide="ignore", invalid="ignore"):
            mine = C.pyin_ref(x, pl)
        quirks = sum(i["quirk"] for i in C.observe_rows(mine["cmndf"], pl)[3])
        assert C.same_bits(mine["O"], O) and C.same_bits(mine["lag_thr"], lag) and C.same_bits(mine["val_thr"], val), name
        assert C.same_bits(mine["rms"], rms) and C.same_bits(mine["f0"], f0) and C.same_bits(mine["conf"], conf), name
        path = mine["path"]
        assert np.abs(rms - 0.01).min() > 1e-6, f"{name}: an rms within 1e-6 of the 0.01 threshold -- replace this input"
        sens = np.zeros(T)
        for seed in range(SEEDS):
            r = np.random.default_rng(1000 + seed)
            fa, ca, _ = tap.run(x, C.P, cm_scale=1 + C.DELTA * r.uniform(-1, 1, size=(T, width)))
            so = np.concatenate([r.uniform(-1, 1, size=(B, T)), np.repeat(r.uniform(-1, 1, size=(1, T)), B, axis=0)])
            fb, cb, _ = tap.run(x, C.P, o_scale=1 + 1e-12 * so)
            with np.errstate(divide="ignore", invalid="ignore"):
                pa = C.pyin_ref(x, pl, cmndf_scale=1 + C.DELTA * np.random.default_rng(1000 + seed).uniform(-1, 1, size=(T, width)))["path"]
            assert np.array_equal(pa, path) and np.array_equal(fa > 0, f0 > 0) and C.same_bits(ca, conf), f"{name}: not stable under (a), seed {seed} -- replace this input"
            assert np.array_equal(fb > 0, f0 > 0) and np.abs(cb - conf).max() <= 4e-12 and np.abs(fb - f0).max() == 0, f"{name}: not stable under (b), seed {seed}"
            sens = np.maximum(sens, np.abs(fa - f0))
        rows = list(C.ROWS)
        print(f"{name}: {T} frames, {int((f0 > 0).sum())} voiced, NaN in val_thr of {int(np.isnan(val).any(axis=0).sum())} frames, deletion quirk in "
              f"{quirks}, f0sens max {sens.max():.2e} Hz ({(sens / np.maximum(f0, 1)).max() / C.DELTA:.1f} DELTA relative)")
        out[f"path_{name}"] = path.astype(np.int16)
        out[f"f0_{name}"], out[f"conf_{name}"], out[f"rms_{name}"], out[f"f0sens_{name}"] = f0, conf, rms, sens
        out[f"cmndf_{name}"] = mine["cmndf"][rows]
        out[f"O_{name}"] = np.ascontiguousarray(O[:, rows].T)
        out[f"lag_thr_{name}"], out[f"val_thr_{name}"] = np.ascontiguousarray(lag[:, rows].T), np.ascontiguousarray(val[:, rows].T)
    path = os.path.join(GOLDEN, "pyin_f0.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SVCMI_REFERENCE", ""))
