"""Timing of the pYIN F0 extractor on the GPU (writes profiles/pyin_f0.md):

    python scripts/pyin_times.py [--rounds 7] [--iters 20] [--reference-cpu-s SECONDS] [--out profiles/pyin_f0.md]

One 10 s clip at 16 kHz (tests/golden/035.wav tiled; 501 frames), everything warm, HIP events on the launching stream, per line the
median of the rounds and their min .. max:
    cmndf / observe / viterbi    the three kernel-level entry points of csrc/pyin.hip, each alone
    compute_f0_pyin              end to end from the device waveform: the stage call (four launches), the device -> host copy, the repeat
``--reference-cpu-s``: the reference's ``pyin`` on the same clip under numpy (numba as the identity), measured separately on a CPU, for
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

SALIENCE_MS, CREPE_MS = 19.2, 12.2          # profiles/salience_f0.md: compute_f0_salience and compute_f0_sing on the same clip


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
    from svcmi.pitch import compute_f0_pyin
    from svcmi.pitch.core import pyin as Y
    from workload.stamp import csrc_sha
    ops = Ops()
    clip = wavfile.read(os.path.join(ROOT, "tests", "golden", "035.wav"))[1].astype(np.float32) / 32768.0
    n = 10 * 16000
    x = torch.from_numpy(np.tile(clip, -(-n // clip.shape[0]))[:n].copy()).cuda()
    plan = Y.pyin_plan(Fs=16000, N=2048, H=320, F_min=45.0, F_max=1760.0, device="cuda")
    cm, _ = ops.pyin_cmndf(plan.struct, x)
    _, _, _, logO = ops.pyin_observe(plan.struct, cm, want_log=True)
    variants = {"cmndf": lambda: ops.pyin_cmndf(plan.struct, x), "observe": lambda: ops.pyin_observe(plan.struct, cm, want_log=True),
                "viterbi": lambda: ops.pyin_viterbi(logO, plan.band, plan.log_tiny, plan.log_cross, plan.log_c),
                "compute_f0_pyin": lambda: compute_f0_pyin(x, "cuda", ops=ops)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(time_events(fn, args.iters))
    res = {"what": "pyin_times", "csrc": csrc_sha(), "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
           "frames": int(cm.shape[0]), "lags": int(plan.p_max), "pitch_bins": int(plan.B), "states": 2 * int(plan.B),
           "reference_cpu_s": args.reference_cpu_s}
    for k, v in times.items():
        res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(json.dumps(res))
    if args.out:
        rows = "\n".join(f"| {k} | {res[k + '_ms']['median']:.3f} | {res[k + '_ms']['min']:.3f} .. {res[k + '_ms']['max']:.3f} |" for k in variants)
        ref = f"{args.reference_cpu_s:.1f} s" if args.reference_cpu_s else "not measured"
        with open(args.out, "w") as f:
            f.write(f"""# pYIN F0 extractor, one 10 s clip

Written by `scripts/pyin_times.py` ({res['device']}, kernel sources {res['csrc']}): {res['frames']} frames, {res['lags']} lags of 2048
samples, {res['pitch_bins']} pitch bins = {res['states']} states; warm, HIP events on the launching stream, {args.rounds} rounds of {args.iters} calls, ms per call.

| what | median | min .. max |
|---|---|---|
{rows}
| compute_f0_salience (profiles/salience_f0.md) | {SALIENCE_MS:.3f} | |
| compute_f0_sing, CREPE (profiles/salience_f0.md) | {CREPE_MS:.3f} | |
| the reference's pyin on a CPU, numpy | {ref} | |

`cmndf`, `observe` and `viterbi` are the kernel-level entry points alone; `compute_f0_pyin` runs from the device waveform to the float
track on the host (device -> host copy and host tail included).

```json
{json.dumps(res)}
```
""")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reference-cpu-s", type=float, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pyin_f0.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pyin_times.py needs the GPU")
    main(a)
