"""Singer sweep timings on one MI355X (profiles/singer_sweep.md): base.yaml sizes, a 10 s clip (T = 1000), fp32, seeded random weights,
inputs and speaker embeddings, warm, event-timed, medians.

  (a) the loop a caller had to write before: S x svc_infer(..., write_pit_wav=False, return_tensor=True), one call per speaker row
  (b) svc_infer_singers over the same S rows at singer_batch 8, 16 and 32
  for S = 16 and S = 56 (the number of embeddings the reference ships).  (a) and (b) alternate inside every repetition, so that a drift
  of the device's clocks lands on both.  Plus the fan-out kernel on its own and the workspace of 16 singers x 2520 frames.

    python scripts/singers_times.py [--reps 10] [--frames 1000] [--out singer_sweep.json]
    python scripts/singers_times.py --kernel-only 50        # the kernel alone, for a kernel trace of its own
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

import torch  # noqa: E402


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def alternated(fns, reps, warm=2):
    """{name: [ms]}: every repetition runs each function once, in the given order."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(once(fn))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--singers", type=int, nargs="+", default=[16, 56])
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N", help="launch the fan-out kernel N times (16 rows) and exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from svcmi import Ops, SynthesizerInfer, svc_infer
    from svcmi.svc_inference import svc_infer_singers
    from workload import config as C, inputs as I, weights as W
    ops, dev, T = Ops(), "cuda", a.frames
    hp = C.base_hp()
    Ic = hp.vits.inter_channels
    g = torch.Generator().manual_seed(2)
    stats = torch.randn(T, 2 * Ic, generator=g).to(dev)
    noise16 = torch.randn(16, Ic, T, generator=g).to(dev)
    length = torch.tensor([T], dtype=torch.int32, device=dev)
    if a.kernel_only:
        for _ in range(a.kernel_only):
            ops.sweep_sample_prior(stats, noise16, length)
        torch.cuda.synchronize()
        return
    m = SynthesizerInfer(hp.data.filter_length // 2 + 1, hp.data.segment_size // hp.data.hop_length, hp, ops=ops)
    m.load_state_dict(W.make_vits_state(hp, seed=1234))
    m.eval()
    m.to(dev)
    d = I.synth_clip(T=T, hp=hp, seed=3, B=1)
    ppg, vec, pit = d["ppg"][0].to(dev), d["vec"][0].to(dev), torch.floor(d["pit"][0]).to(dev)
    res = {"frames": T, "precision": "f32", "device": torch.cuda.get_device_name(0)}
    for S in a.singers:
        spks = torch.stack([I.synth_spk(hp.vits.spk_dim, seed=100 + s) for s in range(S)]).to(dev)
        fns = {"loop_of_svc_infer": lambda: [svc_infer(m, None, spks[s], pit, ppg, vec, hp, dev, write_pit_wav=False, return_tensor=True) for s in range(S)]}
        for sb in (8, 16, 32):
            fns[f"singer_batch_{sb}"] = lambda sb=sb: svc_infer_singers(m, None, spks, pit, ppg, vec, hp, dev, singer_batch=sb, return_tensor=True)
        ms = alternated(fns, a.reps)
        row = {k: summary(v) for k, v in ms.items()}
        for sb in (8, 16, 32):
            ratios = [x / y for x, y in zip(ms[f"singer_batch_{sb}"], ms["loop_of_svc_infer"])]      # per repetition: neighbours in time
            row[f"singer_batch_{sb}"].update(ratio_to_loop=row[f"singer_batch_{sb}"]["median_ms"] / row["loop_of_svc_infer"]["median_ms"],
                                             ratio_min=min(ratios), ratio_max=max(ratios))
        res[f"singers_{S}"] = row
    # the fan-out kernel on its own, against the solo kernel on 16 copies of the statistics
    copies = stats.unsqueeze(0).repeat(16, 1, 1).contiguous()
    len16 = length.repeat(16)
    ks = alternated({"sweep_sample_prior_16_rows": lambda: ops.sweep_sample_prior(stats, noise16, length),
                     "sample_prior_batch_16": lambda: ops.sample_prior(copies, noise16, len16)}, max(a.reps, 20), warm=5)
    res.update({k: summary(v) for k, v in ks.items()})
    cm = m._cmodel()
    res["workspace_bytes_16_singers_2520_frames"] = ops.synth_singers_workspace_bytes(cm, 16, 2520)
    res["workspace_bytes_batch_16_2520_frames"] = int(ops.lib.svcmi_synth_workspace_bytes(ctypes.byref(cm.struct), 16, 2520, 0))
    res["workspace_bytes_solo_2520_frames"] = int(ops.lib.svcmi_synth_workspace_bytes(ctypes.byref(cm.struct), 1, 2520, 0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
