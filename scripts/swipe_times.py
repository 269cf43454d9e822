"""Timing of the SWIPE' F0 extractor on the GPU (writes profiles/swipe_f0.md):

    python scripts/swipe_times.py [--rounds 7] [--iters 50] [--reference-cpu-s SECONDS] [--out profiles/swipe_f0.md]

One 10 s clip at 16 kHz (tests/golden/035.wav tiled; 500 frames), everything warm, HIP events on the launching stream, per line the
median of the rounds and their min .. max:
    mag / resample / strength    the three per-window kernel entry points of csrc/swipe.hip, each alone, all six windows one after the other
    accum / finish               the time interpolation with the weighted sum, and the float64 finish (with its flag-zeroing launch)
    stage                        svcmi_swipe_f0_fwd: all 21 launches
    compute_f0_swipe             end to end from the device waveform: the stage, the device -> host copy, the repeat
The two products' floating-point operations over the fp32 matrix rate (MATRIX_TFLOPS) give their matrix-pipe time; the note sets the
measured time beside it.  The deviations from the reference's record (tests/golden/swipe_f0.npz) on the three golden clips are measured
in the same run.  ``--reference-cpu-s``: the reference's ``swipe_slim`` on the same clip on a CPU, measured separately, for the table.
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

PYIN_MS, SALIENCE_MS, CREPE_MS = 2.4, 19.2, 12.2          # profiles/pyin_f0.md, profiles/salience_f0.md: the same clip end to end
MATRIX_TFLOPS = 157.0                                     # fp32 matrix rate of the MI355X (README)


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
    from svcmi.pitch import compute_f0_swipe
    from svcmi.pitch.core import swipe_slim as W
    from tests import swipe_cases as C
    from workload.stamp import csrc_sha
    ops = Ops()
    clip = wavfile.read(os.path.join(ROOT, "tests", "golden", "035.wav"))[1].astype(np.float32) / 32768.0
    n = 10 * 16000
    x = torch.from_numpy(np.tile(clip, -(-n // clip.shape[0]))[:n].copy()).cuda()
    plan = W.swipe_plan(Fs=16000, H=320, F_min=45.0, F_max=1760.0, R=10, device="cuda")
    s, nw = plan.struct, len(plan.windows)
    Y = [ops.swipe_mag(s, o, x) for o in range(nw)]
    L = [ops.swipe_resample(s, o, Y[o]) for o in range(nw)]
    SN = [ops.swipe_strength(s, o, L[o]) for o in range(nw)]
    S = ops.swipe_accum(s, SN, n)
    variants = {"mag": lambda: [ops.swipe_mag(s, o, x) for o in range(nw)],
                "resample": lambda: [ops.swipe_resample(s, o, Y[o]) for o in range(nw)],
                "strength": lambda: [ops.swipe_strength(s, o, L[o]) for o in range(nw)],
                "accum": lambda: ops.swipe_accum(s, SN, n),
                "finish": lambda: ops.swipe_finish(S, plan.n_log, plan.F_min, plan.step, 0.0),
                "stage": lambda: ops.swipe_f0_fwd(s, x),
                "compute_f0_swipe": lambda: compute_f0_swipe(x, "cuda", ops=ops)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(time_events(fn, args.iters))
    frames = [int(y.shape[0]) for y in Y]
    flops = {"mag": sum(4.0 * T * w["N"] * (w["N"] // 2 + 1) for T, w in zip(frames, plan.windows)),
             "resample": sum(2.0 * T * plan.n_log * (w["N"] // 2 + 1) for T, w in zip(frames, plan.windows)),
             "strength": sum(2.0 * T * plan.n_log * len(w["cand"]) for T, w in zip(frames, plan.windows))}
    dev = {name: dict(zip(("S", "f0_of_tolerance", "conf"), C.check_end_to_end(ops, "cuda", name))) for name in C.CLIPS}
    res = {"what": "swipe_times", "csrc": csrc_sha(), "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
           "frames": int(S.shape[0]), "window_frames": frames, "candidates": int(plan.B), "log_bins": int(plan.n_log), "launches": 3 * nw + 3,
           "gflop": {k: round(v / 1e9, 3) for k, v in flops.items()}, "matrix_pipe_ms": {k: round(v / (MATRIX_TFLOPS * 1e9), 4) for k, v in flops.items()},
           "deviation": dev, "reference_cpu_s": args.reference_cpu_s}
    for k, v in times.items():
        res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(json.dumps(res))
    if args.out:
        rows = "\n".join(f"| {k} | {res[k + '_ms']['median']:.3f} | {res[k + '_ms']['min']:.3f} .. {res[k + '_ms']['max']:.3f} | "
                         f"{(str(res['gflop'][k]) + ' GFLOP, ' + format(res['matrix_pipe_ms'][k], '.4f') + ' ms of matrix pipe') if k in flops else ''} |"
                         for k in variants)
        devs = "\n".join(f"| {name} | {d['S']:.2e} | 0 | {d['f0_of_tolerance']:.3f} | {d['conf']:.2e} |" for name, d in dev.items())
        ref = f"{args.reference_cpu_s:.2f} s" if args.reference_cpu_s else "not measured"
        prod = res["resample_ms"]["median"] + res["strength_ms"]["median"]
        pipe = res["matrix_pipe_ms"]["resample"] + res["matrix_pipe_ms"]["strength"]
        with open(args.out, "w") as f:
            f.write(f"""# SWIPE' F0 extractor, one 10 s clip

Written by `scripts/swipe_times.py` ({res['device']}, kernel sources {res['csrc']}): {res['frames']} output frames, six window sizes
64 .. 2048 with {frames} STFT frames, {res['log_bins']} log-frequency bins, {res['candidates']} candidates; {res['launches']} launches per clip
(three per window size: magnitudes, resampling, strength; then accumulate, flag zero, finish); warm, HIP events on the launching
stream, {args.rounds} rounds of {args.iters} calls, ms per call.

| what | median | min .. max | work |
|---|---|---|---|
{rows}
| compute_f0_pyin (profiles/pyin_f0.md) | {PYIN_MS:.3f} | | |
| compute_f0_salience (profiles/salience_f0.md) | {SALIENCE_MS:.3f} | | |
| compute_f0_sing, CREPE (profiles/salience_f0.md) | {CREPE_MS:.3f} | | |
| the reference's swipe_slim on a CPU (numpy / scipy, taken separately) | {ref} | | |

`mag`, `resample`, `strength` run the six windows one after the other through the kernel-level entry points (each allocates its output);
`stage` is the one C call; `compute_f0_swipe` runs from the device waveform to the float track on the host (device -> host copy and host
tail included).  The two products take {prod:.3f} ms against {pipe:.4f} ms of fp32 matrix-pipe time at {MATRIX_TFLOPS:.0f} TFLOP/s:
{100 * pipe / prod:.1f} % of the pipe's rate.

Deviations from the reference's record on the whole golden clips (`tests/golden/swipe_f0.npz`; bars: S 1e-5, arg-max equal in every
frame, f0 within its tolerance f0sens + 1e-9 f0, conf 1e-5):

| clip | max abs S - S_ref (stored columns) | frames whose arg-max differs | worst f0 deviation / its tolerance | max abs conf - conf_ref |
|---|---|---|---|---|
{devs}

```json
{json.dumps(res)}
```
""")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reference-cpu-s", type=float, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "swipe_f0.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("swipe_times.py needs the GPU")
    main(a)
