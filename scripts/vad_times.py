"""Timing of the voice-activity post-filter on the GPU (DESIGN.md 4.8 "Voice-activity post-filter"; keep the line as profiles/vad_times.json):

    python scripts/vad_times.py [--rounds 7] [--iters 20] [--reference /path/to/reference]

A 10 s and a 60 s clip at 16 kHz (tests/golden/035.wav tiled) through the three kernels of csrc/vad.hip, each launched alone, event-timed,
warm; per kernel the median of the rounds and their min .. max:
    frontend     everything in front of the LSTM for all windows of the clip (one block per window)
    scan         the 2-layer LSTM and the decoder, one block, W serial steps
    mask         the 32 kHz waveform zeroed outside two spans
    forward      SileroVad.audio_forward end to end (upload of the geometry, both launches, the probabilities back on the host)
Where the reference's model file is present (``--reference``, or ./vad/assets/silero_vad.jit), the scripted model's CPU time for the same
windows is printed next to them.  Prints one JSON line.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

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
    from svcmi.vad.utils import SileroVad
    from workload.stamp import csrc_sha
    ops = Ops()
    z = np.load(os.path.join(ROOT, "tests", "golden", "silero_vad.npz"))
    vad = SileroVad.from_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}, "cuda", ops=ops)
    clip = wavfile.read(os.path.join(ROOT, "tests", "golden", "035.wav"))[1].astype(np.float32) / 32768.0
    res = {"what": "vad_times", "csrc": csrc_sha(), "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds}
    jit = os.path.join(args.reference, "vad", "assets", "silero_vad.jit") if args.reference else os.path.join("vad", "assets", "silero_vad.jit")
    ref_model = torch.jit.load(jit, map_location="cpu").eval() if os.path.exists(jit) else None
    for seconds in (10, 60):
        n = seconds * 16000
        x = torch.from_numpy(np.tile(clip, -(-n // clip.shape[0]))[:n].copy()).cuda()
        W = -(-n // 512)
        off, ln = torch.zeros(1, dtype=torch.int64).cuda(), torch.tensor([n], dtype=torch.int64).cuda()
        _, gates = ops.vad_frontend(vad.cmodel, x, off, ln, W)
        svc = torch.randn(2 * n, device="cuda")
        spans = torch.tensor([[n // 10, n // 2], [n // 2 + 4000, n - 3000]], dtype=torch.int32).cuda()
        variants = {"frontend": lambda: ops.vad_frontend(vad.cmodel, x, off, ln, W), "scan": lambda: ops.vad_lstm_scan(vad.cmodel, gates, ln),
                    "mask": lambda: ops.mask_spans(svc, spans, n, 2), "forward": lambda: vad.audio_forward(x, 16000)}
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(time_events(fn, args.iters))
        r = {"windows": W}
        for k, v in times.items():
            r[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        if ref_model is not None:
            xc = torch.nn.functional.pad(x.cpu(), (0, W * 512 - n)).reshape(W, 512)
            with torch.no_grad():
                cpu = []
                for _ in range(3):
                    ref_model.reset_states()
                    t0 = time.perf_counter()
                    for w in range(W):
                        ref_model(xc[w], 16000)
                    cpu.append((time.perf_counter() - t0) * 1000.0)
            r["reference_cpu_ms"] = round(min(cpu), 1)
        res[f"clip_{seconds}s"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reference", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vad_times.py needs the GPU")
    main(a)
