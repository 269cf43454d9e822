"""Regenerate tests/golden/silero_vad.npz (and tests/golden/vad_010.wav) from the reference checkout:

    python scripts/make_vad_golden.py /path/to/reference/checkout

Runs only where the reference is present, never on the GPU machine.  From ``vad/assets/silero_vad.jit`` it takes the 16 kHz model's
TENSORS (``state_dict()`` entries ``_model.*``, stored as ``sd/<name>`` without the prefix; the 8 kHz twin and the archive's TorchScript
code stay where they are), runs the scripted model window by window on two clips, and runs the reference's own
``vad.utils.get_speech_timestamps``:

  probs_<clip>         the scripted model's fp32 probability of every 512-sample window (035: 125 windows, 010: 135)
  ref_dev_<clip>       max |probs - float64 restatement| (tests/vad_cases.py VadRef): the unit of the tests' bound
  spans_<clip>_<thr>   the reference's spans at thresholds 0.2 and 0.5, int64 [S, 2]
  sm_*                 state-machine cases: seeded probability tracks (fp32, concatenated; sm_windows = windows per track, sm_samples =
                       audio length) under a handful of parameter sets (sm_params: JSON; sm_pset: index per track) with the spans the
                       reference's function returns when a stand-in model replays the track (sm_spans float64 [total, 2], sm_nspans)

``vad/utils.py`` imports torchaudio at the top without needing it here: if it is not installed, an empty stub module stands in."""
import json
import os
import shutil
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "whisper-vits-svc_amd"))

from tests import vad_cases as V      # noqa: E402

PARAM_SETS = [
    dict(threshold=0.5),
    dict(threshold=0.2),
    dict(threshold=0.65),                                   # 0.65 - 0.15 is exactly 0.5 in double: a float32 track can sit ON the lower level
    dict(threshold=0.5, max_speech_duration_s=2.0, min_silence_duration_ms=300),
    dict(threshold=0.5, max_speech_duration_s=1.5, min_silence_duration_ms=2000),
    dict(threshold=0.3, min_speech_duration_ms=100, min_silence_duration_ms=50, speech_pad_ms=100),
    dict(threshold=0.5, return_seconds=True),
    dict(threshold=0.5, sampling_rate=32000),
]


def make_tracks(seed=2024, per_set=25):
    """(pset, track float32 [W], samples) for every case: the same mix of shapes under every parameter set."""
    rng = np.random.default_rng(seed)
    cases = []
    for ps, params in enumerate(PARAM_SETS):
        thr = params["threshold"]
        lo = thr - 0.15
        for k in range(per_set):
            W = int(rng.integers(1, 401)) if k >= 4 else (1, 2, 400, 399)[k]
            kind = k % 12
            if kind == 0:
                t = np.full(W, 0.93)                                                     # all speech
            elif kind == 1:
                t = np.full(W, 0.01)                                                     # all silence
            elif kind == 2:
                t = rng.uniform(0, 1, W)                                                 # white
            elif kind == 3:                                                              # values exactly ON the two levels
                t = rng.choice(np.array([thr, lo, np.nextafter(np.float32(thr), np.float32(0)), np.nextafter(np.float32(lo), np.float32(0)), 0.9, 0.01]), W)
            elif kind == 4:                                                              # silence with single-window blips
                t = np.full(W, 0.02)
                t[rng.integers(0, W, max(1, W // 9))] = 0.95
            elif kind == 5:                                                              # speech with single-window dips
                t = np.full(W, 0.9)
                t[rng.integers(0, W, max(1, W // 7))] = 0.01
            elif kind in (6, 7, 8):                                                      # segments of random length: speech / silence / in between
                t = np.empty(W)
                i = 0
                while i < W:
                    n = int(rng.integers(1, 40))
                    t[i:i + n] = rng.choice([0.95, 0.03, (thr + lo) / 2, 0.6, 0.1]) + rng.uniform(-0.02, 0.02)
                    i += n
            elif kind == 9:                                                              # long speech with short pauses (the split logic's quiet stretches)
                t = np.full(W, 0.9)
                for s in rng.integers(0, W, max(1, W // 30)):
                    t[s:s + int(rng.integers(2, 9))] = 0.02
            elif kind == 10:                                                             # a slow random walk
                t = np.clip(0.5 + np.cumsum(rng.normal(0, 0.08, W)), 0, 1)
            else:                                                                        # speech that starts in window 0 and ends in the last
                t = np.full(W, 0.04)
                t[:max(1, W // 3)] = 0.8
                t[-max(1, W // 4):] = 0.85
            t = np.clip(t, 0.0, 1.0).astype(np.float32)
            step = params.get("sampling_rate", 16000) // 16000
            n16 = W * 512 if k % 3 == 0 else int(rng.integers((W - 1) * 512 + 1, W * 512 + 1))
            n = n16 * step if step == 1 else n16 * step - int(rng.integers(0, step))     # x[::step] has n16 samples either way
            cases.append((ps, t, n))
    return cases


class Replay:
    """Stand-in for the scripted model: replays a track through the reference's call protocol."""

    def __init__(self, track):
        self.track, self.i = track, 0

    def reset_states(self):
        self.i = 0

    def __call__(self, chunk, sr):
        assert chunk.shape[-1] == 512 and sr == 16000
        v = torch.tensor(float(self.track[self.i]), dtype=torch.float64)
        self.i += 1
        return v


def main(ref_root):
    if "torchaudio" not in sys.modules:
        try:
            import torchaudio      # noqa: F401
        except ImportError:
            sys.modules["torchaudio"] = types.ModuleType("torchaudio")
    sys.path.insert(0, ref_root)
    from vad.utils import get_speech_timestamps, init_jit_model
    model = init_jit_model(os.path.join(ref_root, "vad", "assets", "silero_vad.jit"))
    model.eval()
    out = {}
    sd = {k[len("_model."):]: v.detach().clone() for k, v in model.state_dict().items() if k.startswith("_model.")}
    for k, v in sd.items():
        out["sd/" + k] = v.numpy()
    shutil.copyfile(os.path.join(ref_root, "configs", "singers_sample", "30-wave-boy", "010.wav"), os.path.join(V.GOLDEN, V.CLIPS["010"]))
    os.chmod(os.path.join(V.GOLDEN, V.CLIPS["010"]), 0o644)
    ref = V.VadRef(sd)
    with torch.no_grad():
        for name in V.CLIPS:
            x = V.clip(name)
            model.reset_states()
            w = ref.windows(x).float()
            probs = torch.stack([model(w[i], 16000).reshape(()) for i in range(w.shape[0])])
            p64 = ref.probs(x)
            out[f"probs_{name}"] = probs.numpy().astype(np.float32)
            out[f"ref_dev_{name}"] = np.float64((probs.double() - p64).abs().max())
            margin = float(torch.minimum((probs - 0.2).abs(), (probs - 0.05).abs()).min())
            print(f"{name}: {w.shape[0]} windows, ref_dev {out[f'ref_dev_' + name]:.3e}, decision margin at 0.2: {margin:.4f}")
            for thr in (0.2, 0.5):
                tags = get_speech_timestamps(x.clone(), model, threshold=thr, sampling_rate=16000)
                out[f"spans_{name}_{int(round(thr * 100)):03d}"] = np.array([[t["start"], t["end"]] for t in tags], dtype=np.int64).reshape(-1, 2)
                print(f"  threshold {thr}: {[(t['start'], t['end']) for t in tags]}")
    cases = make_tracks()
    spans, nspans = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ps, t, n in cases:
            tags = get_speech_timestamps(torch.zeros(n), Replay(t), **PARAM_SETS[ps])
            nspans.append(len(tags))
            spans += [[float(g["start"]), float(g["end"])] for g in tags]
    thr_hits = sum(int((t == np.float32(PARAM_SETS[ps]["threshold"])).any()) for ps, t, _ in cases)
    low_hits = sum(int((t.astype(np.float64) == PARAM_SETS[ps]["threshold"] - 0.15).any()) for ps, t, _ in cases)
    splits = sum(1 for (ps, _, _), k in zip(cases, nspans) if "max_speech_duration_s" in PARAM_SETS[ps] and k > 1)
    print(f"{len(cases)} state-machine cases, {sum(nspans)} spans; tracks exactly on the threshold: {thr_hits}, on threshold - 0.15: {low_hits}, "
          f"max-duration cases with more than one span: {splits}")
    assert thr_hits and low_hits and splits
    out.update(sm_tracks=np.concatenate([t for _, t, _ in cases]).astype(np.float32), sm_windows=np.array([len(t) for _, t, _ in cases], dtype=np.int32),
               sm_samples=np.array([n for _, _, n in cases], dtype=np.int64), sm_pset=np.array([ps for ps, _, _ in cases], dtype=np.int32),
               sm_params=np.array(json.dumps(PARAM_SETS)), sm_spans=np.array(spans, dtype=np.float64).reshape(-1, 2),
               sm_nspans=np.array(nspans, dtype=np.int32))
    path = os.path.join(V.GOLDEN, "silero_vad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SVCMI_REFERENCE", ""))
