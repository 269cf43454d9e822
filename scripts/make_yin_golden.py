"""Regenerate tests/golden/yin_f0.npz from the reference checkout:

    python scripts/make_yin_golden.py /path/to/reference/checkout

Runs only where the reference is present, never on the GPU machine.  It imports the reference's ``pitch/core/yin.py`` BY PATH and runs
``yin`` with the parameters of ``compute_f0_yin`` (Fs 16000, N 2048, H 320, 45 .. 1760 Hz, threshold 0.15).  ``numba.njit`` is replaced by
the identity: the reference then executes under plain numpy, which is the behaviour the device path reproduces.

Inputs: those of the pYIN golden file -- tests/golden/035.wav, tests/golden/vad_010.wav and ``make_salience_golden.glide()`` (stored in
tests/golden/pyin_f0.npz, read from there by the tests).  Per input ``<name>``:

  f0_<name>, ap_<name>            float64 [frames]
  lag_<name>, lag_first_<name>    the second and the first thresholding's result, float64 [frames]
  kind_<name>                     int32 [frames]: 1 = the first thresholding took the arg-min branch, 2 = the second returned through the
                                  shortcut of an empty window, 4 = the second took the arg-min branch
  f0sens_<name>, apsens_<name>    the largest |f0' - f0| and |ap' - ap| per frame over the 8 perturbed runs, float64 [frames]
  cmndf_<name>                    the CMNDF rows of the frames ROWS, float64 [len(ROWS), lag_max + 1]

Only data goes into the file.  The script ASSERTS
  * that the float64 programme of tests/yin_cases.py equals the reference bit for bit on every frame of the three inputs and on 40
    seeded noise and tone frames: the CMNDF rows, both lags, their Python types (int or float), f0 and ap;
  * that the reference's own decisions are stable: with the CMNDF multiplied elementwise by 1 + DELTA u, u uniform in [-1, 1], over 8
    seeds -- DELTA is the relative bound derived for the CMNDF kernel (tests/pyin_cases.py) -- the integer parts of both lags, their types
    and the kind bits are unchanged in every frame;
  * that no ap lies within 1e-6 of 0.2, the ``ap_threshold`` the tests use.
An input that fails is to be replaced, not tolerated."""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "whisper-vits-svc_amd"), os.path.join(ROOT, "scripts")]
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEEDS = 8


def load_reference(ref_root):
    """The reference's yin module, imported as ``ref_pitch_core.yin`` from a synthetic package that points at pitch/core."""
    nb = types.ModuleType("numba")
    nb.njit = lambda f: f
    pkg = types.ModuleType("ref_pitch_core")
    pkg.__path__ = [os.path.join(ref_root, "pitch", "core")]
    saved = sys.modules.get("numba")
    sys.modules.update(numba=nb, ref_pitch_core=pkg)
    try:
        return importlib.import_module("ref_pitch_core.yin")
    finally:
        if saved is None:
            sys.modules.pop("numba", None)
        else:
            sys.modules["numba"] = saved


class Tap:
    """Wraps the reference's CMNDF and absolute_thresholding: remembers the unperturbed CMNDF rows (they cost most of a run), multiplies
    them by a given factor, and keeps what every thresholding returned."""

    def __init__(self, mod):
        self.mod, self.cm, self.scale, self.frame, self.rows, self.lags = mod, {}, None, 0, [], []
        self.cmndf0, self.thresh0 = mod.cumulative_mean_normalized_difference_function, mod.absolute_thresholding
        mod.cumulative_mean_normalized_difference_function = self.cmndf
        mod.absolute_thresholding = self.thresh

    def cmndf(self, frame, lag_max):
        key = (frame.tobytes(), lag_max)
        if key not in self.cm:
            self.cm[key] = self.cmndf0(frame, lag_max)
        c = self.cm[key].copy()
        self.rows.append(self.cm[key])
        if self.scale is not None:
            c = c * self.scale[self.frame]
        self.frame += 1
        return c

    def thresh(self, *a, **k):
        out = self.thresh0(*a, **k)
        self.lags.append(out)
        return out

    def run(self, x, params, scale=None):
        """-> dict(f0, t, ap, cmndf [frames, lag_max + 1] (unperturbed), first, new: the lists of the two thresholdings' results)."""
        self.scale, self.frame, self.rows, self.lags = scale, 0, [], []
        f0, t, ap = self.mod.yin(x, **params)
        assert len(self.lags) == 2 * len(f0) == 2 * len(self.rows)
        return dict(f0=f0, t=t, ap=ap, cmndf=np.stack(self.rows), first=self.lags[0::2], new=self.lags[1::2])


def seeded_frames(C):
    """A clip whose 40 frames are white noise at three levels and 50 Hz tones, hop by hop."""
    rng = np.random.default_rng(2024)
    H = C.P["H"]
    t = np.arange(H) / 16000
    parts = [rng.standard_normal(H) * (10.0 ** -rng.integers(0, 4)) if k % 4 else np.sin(2 * np.pi * 50.0 * (t + k * H / 16000) + k) for k in range(39)]
    return np.concatenate(parts).astype(np.float32)


def compare(C, ref, mine, name):
    """The programme against the reference, bit for bit, types included."""
    assert C.same_bits(mine["cmndf"], ref["cmndf"]), name
    for key, ints in (("first", "first_int"), ("new", "lag_int")):
        got = mine["lag_first" if key == "first" else "lag"]
        assert C.same_bits(got, np.array([float(v) for v in ref[key]])), (name, key)
        assert np.array_equal(mine[ints], np.array([C.is_int(v) for v in ref[key]])), (name, key, "types")
    assert C.same_bits(mine["f0"], ref["f0"]) and C.same_bits(mine["ap"], ref["ap"]), name


def main(ref_root):
    from tests import yin_cases as C
    mod = load_reference(ref_root)
    tap = Tap(mod)
    pl = C.plan()
    width = pl.lag_max + 1
    noise = seeded_frames(C)
    ref = tap.run(noise, C.P)
    assert len(ref["f0"]) == 40
    compare(C, ref, C.yin_ref(noise), "seeded frames")
    out = {"rows": np.array(C.ROWS, dtype=np.int32)}
    for name in C.CLIPS:
        x = C.clip(name)
        ref = tap.run(x, C.P)
        T = len(ref["f0"])
        assert T == 1 + len(x) // C.P["H"] and np.array_equal(ref["t"], np.arange(T) * C.P["H"] / C.P["Fs"])
        mine = C.yin_ref(x)
        compare(C, ref, mine, name)
        gap = np.abs(ref["ap"] - C.AP_THRESHOLD).min()
        assert gap > 1e-6, f"{name}: an ap within 1e-6 of {C.AP_THRESHOLD} -- replace this input"
        f0sens, apsens = np.zeros(T), np.zeros(T)
        for seed in range(SEEDS):
            scale = 1 + C.DELTA * np.random.default_rng(1000 + seed).uniform(-1, 1, size=(T, width))
            pert = tap.run(x, C.P, scale=scale)
            pm = C.yin_ref(x, cmndf=mine["cmndf"], cmndf_scale=scale)
            compare(C, pert, pm, f"{name} seed {seed}")
            same = (np.array_equal(np.floor(pm["lag"]), np.floor(mine["lag"])) and np.array_equal(np.floor(pm["lag_first"]), np.floor(mine["lag_first"]))
                    and np.array_equal(pm["kind"], mine["kind"]) and np.array_equal(pm["lag_int"], mine["lag_int"]) and np.array_equal(pm["first_int"], mine["first_int"]))
            assert same, f"{name}: not stable under the perturbation, seed {seed} -- replace this input"
            f0sens = np.maximum(f0sens, np.abs(pert["f0"] - ref["f0"]))
            apsens = np.maximum(apsens, np.abs(pert["ap"] - ref["ap"]))
        kind = mine["kind"]
        print(f"{name}: {T} frames, both lags and the branches unchanged in {SEEDS} perturbed runs, max f0 shift {f0sens.max():.1e} Hz, max ap shift {apsens.max():.1e}, closest ap to "
              f"{C.AP_THRESHOLD}: {gap:.1e}; first search arg-min in {int((kind & 1 > 0).sum())} frames, integer result in {int(mine['lag_int'].sum())} "
              f"(shortcut {int((kind & 2 > 0).sum())}, arg-min {int((kind & 4 > 0).sum())}), ap > {C.AP_THRESHOLD} in {int((ref['ap'] > C.AP_THRESHOLD).sum())}")
        out[f"f0_{name}"], out[f"ap_{name}"], out[f"lag_{name}"], out[f"lag_first_{name}"] = ref["f0"], ref["ap"], mine["lag"], mine["lag_first"]
        out[f"kind_{name}"], out[f"f0sens_{name}"], out[f"apsens_{name}"] = kind.astype(np.int32), f0sens, apsens
        out[f"cmndf_{name}"] = mine["cmndf"][list(C.ROWS)]
    path = os.path.join(GOLDEN, "yin_f0.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SVCMI_REFERENCE", ""))
