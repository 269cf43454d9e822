"""Timing of the YIN F0 extractor on the GPU (writes profiles/yin_f0.md):

    python scripts/yin_times.py [--rounds 7] [--iters 50] [--reference-cpu-s SECONDS] [--out profiles/yin_f0.md]

One 10 s clip at 16 kHz (tests/golden/035.wav tiled; 501 frames), everything warm, HIP events on the launching stream, per line the
median of the rounds and their min .. max:
    cmndf / pick / aperiodicity    the three kernel-level entry points of csrc/yin.hip, each alone (cmndf is pYIN's kernel)
    stage                          svcmi_yin_f0_fwd: the three launches on one workspace
    compute_f0_yin                 end to end from the device waveform: the stage call, the device -> host copy, the repeat
    compute_f0_pyin                the pYIN recipe on the same clip in the same run, for the comparison
``--reference-cpu-s``: the reference's ``yin`` on the same clip under numpy (numba as the identity), measured separately on a CPU, for
the table.  Prints one JSON line and writes the markdown table.  Needs the GPU: there is no CPU path."""
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

PYIN_MS, SWIPE_MS, SALIENCE_MS, CREPE_MS = 2.45, 0.89, 19.2, 12.2          # profiles/pyin_f0.md, swipe_f0.md, salience_f0.md: the same clip


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
    from svcmi.pitch import compute_f0_pyin, compute_f0_yin
    from svcmi.pitch.core import yin as Y
    from workload.stamp import csrc_sha
    ops = Ops()
    clip = wavfile.read(os.path.join(ROOT, "tests", "golden", "035.wav"))[1].astype(np.float32) / 32768.0
    n = 10 * 16000
    x = torch.from_numpy(np.tile(clip, -(-n // clip.shape[0]))[:n].copy()).cuda()
    plan = Y.yin_plan(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, threshold=0.15)
    cm = ops.yin_cmndf(plan.struct, x)
    lag = ops.yin_pick(plan.struct, cm)[0].contiguous()
    variants = {"cmndf": lambda: ops.yin_cmndf(plan.struct, x), "pick": lambda: ops.yin_pick(plan.struct, cm),
                "aperiodicity": lambda: ops.yin_aperiodicity(plan.struct, x, lag), "stage": lambda: ops.yin_f0_fwd(plan.struct, x),
                "compute_f0_yin": lambda: compute_f0_yin(x, "cuda", ops=ops), "compute_f0_pyin": lambda: compute_f0_pyin(x, "cuda", ops=ops)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(time_events(fn, args.iters))
    res = {"what": "yin_times", "csrc": csrc_sha(), "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
           "frames": int(cm.shape[0]), "lags": int(plan.lag_max), "reference_cpu_s": args.reference_cpu_s}
    for k, v in times.items():
        res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(json.dumps(res))
    if args.out:
        rows = "\n".join(f"| {k} | {res[k + '_ms']['median']:.3f} | {res[k + '_ms']['min']:.3f} .. {res[k + '_ms']['max']:.3f} |" for k in variants)
        ref = f"{args.reference_cpu_s:.1f} s" if args.reference_cpu_s else "not measured"
        with open(args.out, "w") as f:
            f.write(f"""# YIN F0 extractor, one 10 s clip

Written by `scripts/yin_times.py` ({res['device']}, kernel sources {res['csrc']}): {res['frames']} frames, {res['lags']} lags of 2048
samples; warm, HIP events on the launching stream, {args.rounds} rounds of {args.iters} calls, ms per call.

| what | median | min .. max |
|---|---|---|
{rows}
| compute_f0_pyin (profiles/pyin_f0.md) | {PYIN_MS:.3f} | |
| compute_f0_swipe (profiles/swipe_f0.md) | {SWIPE_MS:.3f} | |
| compute_f0_salience (profiles/salience_f0.md) | {SALIENCE_MS:.3f} | |
| compute_f0_sing, CREPE (profiles/salience_f0.md) | {CREPE_MS:.3f} | |
| the reference's yin on a CPU, numpy | {ref} | |

`cmndf`, `pick` and `aperiodicity` are the kernel-level entry points alone (each allocates its outputs); `stage` is the one call that
makes the three launches; `compute_f0_yin` runs from the device waveform to the float track on the host (device -> host copy and host
tail included).  `compute_f0_pyin` is timed in the same run; the lines below it are copied from their own profiles.

```json
{json.dumps(res)}
```
""")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reference-cpu-s", type=float, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "yin_f0.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("yin_times.py needs the GPU")
    main(a)
