"""Key sweep timings on one MI355X (profiles/key_sweep.md): base.yaml sizes, a 10 s clip (T = 1000), fp32, warm, event-timed, medians.

  (a) the loop a caller had to write before: 25 x svc_infer(..., write_pit_wav=False, return_tensor=True) on pre-shifted tracks
  (b) svc_infer_sweep over the same 25 keys at key_batch 8, 16 and 25
  plus the shared front (two convolutions at batch 1), the two sweep kernels, and the workspace of 16 keys x 2520 frames.

    python scripts/sweep_times.py [--reps 20] [--frames 1000] [--out key_sweep.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "whisper-vits-svc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from svcmi import Ops, SynthesizerInfer, svc_infer
    from svcmi._lib import TraceRecord
    from svcmi.svc_inference import svc_infer_sweep
    from workload import config as C, inputs as I, weights as W
    ops, dev, T = Ops(), "cuda", a.frames
    hp = C.base_hp()
    m = SynthesizerInfer(hp.data.filter_length // 2 + 1, hp.data.segment_size // hp.data.hop_length, hp, ops=ops)
    m.load_state_dict(W.make_vits_state(hp, seed=1234))
    m.eval()
    m.to(dev)
    d = I.synth_clip(T=T, hp=hp, seed=3, B=1)
    spk, ppg, vec = d["spk"][0].to(dev), d["ppg"][0].to(dev), d["vec"][0].to(dev)
    pit = torch.floor(d["pit"][0])                                        # integers, as the CSV gives them
    shifts = list(range(-12, 13))
    tracks = [torch.FloatTensor(np.asarray(pit, np.float64) * 2 ** (s / 12)) for s in shifts]
    res = {"frames": T, "keys": len(shifts), "precision": "f32", "device": torch.cuda.get_device_name(0)}

    def loop():
        return [svc_infer(m, None, spk, t, ppg, vec, hp, dev, write_pit_wav=False, return_tensor=True) for t in tracks]
    res["loop_of_svc_infer"] = timed(loop, a.reps)
    for kb in (8, 16, 25):
        res[f"sweep_key_batch_{kb}"] = timed(lambda: svc_infer_sweep(m, None, spk, pit, ppg, vec, hp, dev, shifts, key_batch=kb, return_tensor=True), a.reps)
    base = res["loop_of_svc_infer"]["median_ms"]
    for kb in (8, 16, 25):
        res[f"sweep_key_batch_{kb}"]["ratio_to_loop"] = res[f"sweep_key_batch_{kb}"]["median_ms"] / base
    # the pieces: the two sweep kernels on their own, and the shared front read from the stage's per-launch trace
    cm = m._cmodel()
    pit_d, length = pit.to(dev), torch.tensor([T], dtype=torch.int32, device=dev)
    factors = [2 ** (s / 12) for s in shifts[:16]]
    xs = torch.randn(T, hp.vits.hidden_channels, device=dev)
    emb = torch.randn(256, hp.vits.hidden_channels, device=dev)
    pit_k = ops.sweep_pitch(pit_d, factors)
    res["sweep_pitch_16_keys"] = timed(lambda: ops.sweep_pitch(pit_d, factors), a.reps, warm=5)
    res["sweep_embed_16_keys"] = timed(lambda: ops.sweep_embed(xs, pit_k, emb, length), a.reps, warm=5)
    # the front: trace one sweep call; its first two convolution launches are pre and hub at batch 1
    src = m.pitch2source(pit_k[:1])
    noise = torch.randn(1, hp.vits.inter_channels, T, device=dev)
    front = []
    for _ in range(max(a.reps, 5)):
        ops.lib.svcmi_trace_begin(8192)
        ops.synth_sweep_fwd(cm, ppg, vec, pit_d, spk, length, src.view(1, -1), noise, [1.0])
        recs = (TraceRecord * 8192)()
        n = min(ops.lib.svcmi_trace_end(recs, 8192), 8192)
        names = [ops.lib.svcmi_trace_op_name(recs[i].op).decode() for i in range(n)]
        first = [i for i, nm in enumerate(names) if nm.startswith("svcmi_conv_gemm")][:2]
        front.append(sum(recs[i].ms for i in first))
    res["shared_front_two_convolutions"] = {"median_ms": statistics.median(front), "min_ms": min(front), "max_ms": max(front), "reps": len(front)}
    res["workspace_bytes_16_keys_2520_frames"] = ops.synth_sweep_workspace_bytes(cm, 16, 2520)
    res["workspace_bytes_solo_2520_frames"] = int(ops.lib.svcmi_synth_workspace_bytes(ctypes.byref(cm.struct), 1, 2520, 0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
