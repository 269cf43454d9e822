"""Timing of the checkpoint scoring on the GPU (profiles/validate_times.json, DESIGN.md "Scoring checkpoints"):

    python scripts/validate_times.py [--n 320000] [--rounds 7] [--iters 20]

One 10 s pair at 32 kHz through the mel L1 and the four configured STFT resolutions, two ways on the same device, same process,
alternating, event-timed, warm; per variant the median of the rounds and their min .. max:
    fused        the entry points of csrc/spectral_loss.hip (svcmi.svc_validate.Scorer: 2 spectrograms + 2 mel projections + 1 |a - b| sum +
                 4 pair distances, 13 launches), and per resolution the pair distance alone
    torch_stft   the reference recipe (vits_extend/stft.py, stft_loss.py) written with torch.stft / matmul / torch.norm
Prints one JSON line.  Needs the GPU: there is no CPU path.
"""
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

RESOLUTIONS = [(1024, 120, 600), (2048, 240, 1200), (4096, 480, 2400), (512, 50, 240)]      # configs/base.yaml: mrd.resolutions
DATA = dict(sampling_rate=32000, filter_length=1024, hop_length=320, win_length=1024, mel_channels=100, mel_fmin=50.0, mel_fmax=16000.0)


def time_events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters          # us per call


def signal(n, freq, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    x = 0.5 * np.sin(2 * np.pi * freq * np.arange(n) / 32000.0) + 0.05 * rng.standard_normal(n)
    x[:n // 4] = 0.0
    return torch.from_numpy((scale * x).astype(np.float32)).cuda()[None]


def main(args):
    from svcmi import Ops
    from svcmi.svc_validate import Scorer
    from svcmi.vits.spectrogram import spectrogram_basis
    from svcmi.whisper.audio import slaney_mel_filterbank
    from workload.config import AttrDict
    from workload.stamp import csrc_sha
    ops = Ops()
    n = args.n
    x, y = signal(n, 233.0, 1, 0.8), signal(n, 220.0, 0)
    hp = AttrDict({"data": DATA, "mrd": {"resolutions": RESOLUTIONS}})
    scorer = Scorer(hp, "cuda", ops=ops)
    d = DATA
    mel_basis = torch.from_numpy(slaney_mel_filterbank(d["sampling_rate"], d["filter_length"], d["mel_channels"], d["mel_fmin"], d["mel_fmax"])).cuda()
    mel_window = torch.hann_window(d["win_length"], device="cuda")
    windows = {r: torch.hann_window(r[2], device="cuda") for r in RESOLUTIONS}

    def fused():
        return scorer(x[0], y[0])

    def torch_mel(w):
        pad = int((d["filter_length"] - d["hop_length"]) / 2)
        w = torch.nn.functional.pad(w.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
        s = torch.stft(w, d["filter_length"], hop_length=d["hop_length"], win_length=d["win_length"], window=mel_window, center=False,
                       pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        s = torch.sqrt(s.real ** 2 + s.imag ** 2 + 1e-9)
        return torch.log(torch.clamp(torch.matmul(mel_basis, s), min=1e-5))

    def torch_mag(w, r):
        s = torch.stft(w, r[0], r[1], r[2], windows[r], return_complex=True)
        return torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=1e-7)).transpose(2, 1)

    def torch_resolution(r):
        mx, my = torch_mag(x, r), torch_mag(y, r)
        return torch.norm(my - mx, p="fro") / torch.norm(my, p="fro"), torch.nn.functional.l1_loss(torch.log(my), torch.log(mx))

    def torch_stft():
        mel_l1 = torch.nn.functional.l1_loss(torch_mel(x), torch_mel(y))
        sc = mag = 0.0
        for r in RESOLUTIONS:
            s, m = torch_resolution(r)
            sc, mag = sc + s, mag + m
        return torch.stack([mel_l1, sc / len(RESOLUTIONS), mag / len(RESOLUTIONS)])

    variants = {"fused": fused, "torch_stft": torch_stft}
    for r in RESOLUTIONS:
        basis = spectrogram_basis(r[0], r[2], "cuda")
        variants["fused_%d_%d_%d" % r] = (lambda r=r, basis=basis: ops.stft_distance(x, y, basis, r[0], r[1]))
        variants["torch_stft_%d_%d_%d" % r] = (lambda r=r: torch_resolution(r))
    a, b = fused(), torch_stft()
    torch.cuda.synchronize()
    for fn in variants.values():                             # warm: code objects, FFT plans, allocator
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(time_events(fn, args.iters))
    gflop = sum(8e-9 * (1 + n // r[1]) * (r[0] // 2 + 1) * r[0] for r in RESOLUTIONS)
    res = {"what": "validate_scoring", "n": n, "resolutions": RESOLUTIONS, "csrc": csrc_sha(), "iters": args.iters, "rounds": args.rounds,
           "dft_gflop_of_the_four_pairs": round(gflop, 2), "fused_values": [float(v) for v in a], "torch_stft_values": [float(v) for v in b]}
    for k, v in times.items():
        res[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=320000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("validate_times.py needs the GPU")
    main(a)
