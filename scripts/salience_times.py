"""Timing of the salience F0 extractor against CREPE on the GPU (writes profiles/salience_f0.md):

    python scripts/salience_times.py [--rounds 7] [--iters 20] [--out profiles/salience_f0.md]

One 10 s clip at 16 kHz (tests/golden/035.wav tiled; 501 frames), everything warm, HIP events on the launching stream, per line the
median of the rounds and their min .. max:
    stft / map / dp        the three kernel-level entry points of csrc/salience.hip, each alone
    compute_f0_salience    end to end from the device waveform: the stage call, the device -> host copy of the path, the host tail
    compute_f0_sing        the same clip through CREPE-full (seeded weights of workload/: same shapes and launches as crepe/assets/full.pth),
                           fp32, Viterbi on the device, the device -> host copy, the host tail
Prints one JSON line and writes the markdown table.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "whisper-vits-svc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np          # noqa: E402
import torch                # noqa: E402


def time_events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters          # ms per call


def main(args):
    from scipy.io import wavfile
    from svcmi import Ops
    from svcmi.pitch import compute_f0_salience, compute_f0_sing, load_crepe
    from svcmi.pitch.core import salience as S
    from workload import weights as W
    from workload.stamp import csrc_sha
    ops = Ops()
    clip = wavfile.read(os.path.join(ROOT, "tests", "golden", "035.wav"))[1].astype(np.float32) / 32768.0
    n = 10 * 16000
    x = torch.from_numpy(np.tile(clip, -(-n // clip.shape[0]))[:n].copy()).cuda()
    plan = S.salience_plan(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, device="cuda")
    X = ops.salience_stft(plan.struct, x)
    _, z, _ = ops.salience_map(plan.struct, X)
    crepe = load_crepe(W.make_crepe_state("full"), "cuda", ops=ops)
    noise = torch.randn(n)
    variants = {"stft": lambda: ops.salience_stft(plan.struct, x), "map": lambda: ops.salience_map(plan.struct, X),
                "dp": lambda: ops.salience_dp(z, plan.struct.tol, plan.log_hi, plan.log_lo),
                "compute_f0_salience": lambda: compute_f0_salience(x, "cuda", ops=ops),
                "compute_f0_sing": lambda: compute_f0_sing(x, "cuda", model=crepe, noise=noise)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(time_events(fn, args.iters if k != "compute_f0_sing" else max(2, args.iters // 5)))
    res = {"what": "salience_times", "csrc": csrc_sha(), "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
           "frames": int(X.shape[0]), "stft_bins": int(plan.n_bins), "pitch_bins": int(plan.B)}
    for k, v in times.items():
        res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(json.dumps(res))
    if args.out:
        rows = "\n".join(f"| {k} | {res[k + '_ms']['median']:.3f} | {res[k + '_ms']['min']:.3f} .. {res[k + '_ms']['max']:.3f} |" for k in variants)
        with open(args.out, "w") as f:
            f.write(f"""# Salience F0 extractor against CREPE, one 10 s clip

Written by `scripts/salience_times.py` ({res['device']}, kernel sources {res['csrc']}): {res['frames']} frames, {res['stft_bins']} of 1025 STFT
bins, {res['pitch_bins']} pitch bins; warm, HIP events on the launching stream, {args.rounds} rounds of {args.iters} calls (CREPE: {max(2, args.iters // 5)}), ms per call.

| what | median | min .. max |
|---|---|---|
{rows}

`stft`, `map` and `dp` are the kernel-level entry points alone; the two `compute_f0_*` lines run from the device waveform to the float
track on the host (device -> host copy and host tail included).  CREPE runs the seeded full-capacity weights in fp32.

```json
{json.dumps(res)}
```
""")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "salience_f0.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("salience_times.py needs the GPU")
    main(a)
