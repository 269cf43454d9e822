"""Timings of the training-set preparation on the GPU (profiles/preprocessing.md):

    python scripts/preprocess_times.py kernel [--n 320000] [--rounds 7] [--iters 200]
        the fused linear spectrogram (csrc/spectrogram.hip, one launch) against the same result composed from the building blocks the
        library had before it: reflect_pad + the implicit-GEMM convolution with the DFT table at stride hop + magnitude_spectrum
        (+ nlc_to_ncl for the [bins, frames] layout).  Same process, alternating, event-timed, warm; per variant the median of the
        rounds and their min .. max.
    python scripts/preprocess_times.py driver [--clips 32] [--seconds 10] [--precision f32]
        svcmi.svc_preprocessing's per-clip chain on a synthetic folder (44.1 kHz stereo int16) with full-size seeded models, loaded
        once and warmed with one clip: seconds of raw audio per second with the extractors in flight, and, in a second pass that
        synchronises after every stage, the share of every stage.
Prints one JSON line per measurement.  Needs the GPU: there is no CPU path.
"""
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
    return e0.elapsed_time(e1) * 1000.0 / iters          # us per call


def kernel(args):
    from svcmi import Ops
    from svcmi.vits.spectrogram import spectrogram_basis
    from workload.stamp import csrc_sha
    ops = Ops()
    n_fft, hop, win, n = 1024, 320, 1024, args.n
    pad, bins = (n_fft - hop) // 2, n_fft // 2 + 1
    half = (bins + 3) // 4 * 4
    rng = np.random.default_rng(0)
    x = torch.from_numpy((0.5 * np.sin(2 * np.pi * 220.0 * np.arange(n) / 32000.0) + 0.05 * rng.standard_normal(n)).astype(np.float32)).cuda()[None]
    basis = spectrogram_basis(n_fft, win, "cuda")
    frames = 1 + (n + 2 * pad - n_fft) // hop
    # the composition's operand: [2 * half, n_fft] rows = table columns (cos block | sin block, zero rows as padding)
    w = torch.zeros(2 * half, n_fft, device="cuda")
    w[:bins] = basis[:, 0::2].t()
    w[half:half + bins] = basis[:, 1::2].t()
    w = w.contiguous()

    def fused():
        return ops.linear_spectrogram(x, basis, n_fft, hop, pad, 1e-6)

    def composed(transpose=True):
        xp = ops.reflect_pad(x, pad)
        ri = ops.conv(xp, w, None, ksize=n_fft, stride=hop, pad=0, c_in=1, ldx=1, t_in=xp.shape[1], t_out=frames, x_bstride=xp.stride(0))
        m = ops.magnitude_spectrum(ri, bins, half)
        return ops.nlc_to_ncl(m, bins) if transpose else m

    a, b = fused(), composed()
    torch.cuda.synchronize()
    ref = torch.sqrt(b[0, :bins].double() ** 2 + 1e-6)      # the composition has no eps under its root
    diff = float((a[0].double() - ref).abs().max())
    variants = {"fused": fused, "composed": composed, "composed_time_major": lambda: composed(False)}
    for fn in variants.values():                             # warm: code objects, workspaces, allocator
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(time_events(fn, args.iters))
    res = {"what": "linear_spectrogram", "shape": [n_fft, hop, win, n], "frames": frames, "csrc": csrc_sha(), "iters": args.iters,
           "rounds": args.rounds, "max_abs_diff_fused_vs_composed": diff, "gflop": 4e-9 * frames * bins * n_fft}
    for k, v in times.items():
        res[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    print(json.dumps(res))


def driver(args):
    import shutil
    import tempfile
    from scipy.io import wavfile
    from svcmi import svc_preprocessing as P
    from workload import config as C, speaker as WS, weights as W
    from workload.stamp import csrc_sha
    tmp = tempfile.mkdtemp(prefix="svcmi_prep_")
    try:
        # full-size seeded models: checkpoints as dicts (the loaders take them), the speaker encoder as the files its loader reads
        torch.save({"model": WS.make_speaker_state(**WS.FULL)}, os.path.join(tmp, "speaker.pth.tar"))
        with open(os.path.join(tmp, "speaker.json"), "w", encoding="utf-8") as f:
            json.dump({"audio": dict(num_mels=80, fft_size=1024, sample_rate=16000, win_length=1024, hop_length=256, preemphasis=0.98,
                                     min_level_db=-100, ref_level_db=20, signal_norm=True, symmetric_norm=True, max_norm=4.0, clip_norm=True,
                                     mel_fmin=0.0, mel_fmax=8000.0, do_trim_silence=True, trim_db=60),
                       "model": dict(WS.FULL, use_lstm_with_projection=True)}, f)
        with open(os.path.join(tmp, "cfg.yaml"), "w", encoding="utf-8") as f:
            f.write("data:\n  sampling_rate: 32000\n  filter_length: 1024\n  hop_length: 320\n  win_length: 1024\n  max_wav_value: 32768.0\n")
        raw = os.path.join(tmp, "dataset_raw", "singer0")
        os.makedirs(raw)
        rng = np.random.default_rng(1)
        n = int(args.seconds * 44100)
        t = np.arange(n) / 44100.0
        for i in range(args.clips):
            f0 = 150.0 + 10.0 * i
            s = 0.4 * np.sin(2 * np.pi * (f0 + 20 * np.sin(2 * np.pi * 1.5 * t)) * t) + 0.02 * rng.standard_normal(n)
            wavfile.write(os.path.join(raw, f"{i:03d}.wav"), 44100, np.round(np.stack([s, 0.8 * s], 1) * 32767).astype(np.int16))
        total = args.clips * args.seconds
        res = {"what": "svc_preprocessing", "clips": args.clips, "seconds_each": args.seconds, "precision": args.precision, "csrc": csrc_sha()}
        models = dict(whisper=W.make_whisper_state(C.WHISPER_LARGE_V2), hubert=W.make_hubert_state(), crepe=W.make_crepe_state("full"))
        for mode in ("in_flight", "stage_times"):
            out = os.path.join(tmp, "data_svc_" + mode)
            argv = ["--raw", os.path.join(tmp, "dataset_raw"), "--out", out, "--files", os.path.join(tmp, "files"), "--config",
                    os.path.join(tmp, "cfg.yaml"), "--speaker-model", os.path.join(tmp, "speaker.pth.tar"), "--speaker-config",
                    os.path.join(tmp, "speaker.json"), "--loader", "gpu", "--seed", "1234", "--precision", args.precision]
            pa = P.build_parser().parse_args(argv + (["--stage-times"] if mode == "stage_times" else []))
            pa.whisper, pa.hubert, pa.crepe = models["whisper"], models["hubert"], models["crepe"]
            pre = P.Preprocessor(pa)                         # models loaded once, outside the timed window
            os.makedirs(os.path.join(out, "warm"), exist_ok=True)
            for kind in ("waves-16k", "waves-32k", "pitch", "whisper", "hubert", "speaker", "specs"):
                os.makedirs(os.path.join(out, kind, "warm"), exist_ok=True)
                os.makedirs(os.path.join(out, kind, "singer0"), exist_ok=True)
            pre.clip("warm", "000", os.path.join(raw, "000.wav"))      # warm: code objects, weight images, workspaces
            pre.stage_seconds = {k: 0.0 for k in P.STAGES}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.clips):
                pre.clip("singer0", f"{i:03d}", os.path.join(raw, f"{i:03d}.wav"))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[mode] = {"wall_s": round(dt, 3), "audio_seconds_per_second": round(total / dt, 2)}
            if mode == "stage_times":
                st = {k: round(v, 3) for k, v in pre.stage_seconds.items()}
                res[mode]["stage_seconds"] = st
                res[mode]["stage_share"] = {k: round(v / max(sum(st.values()), 1e-9), 3) for k, v in st.items()}
            del pre
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--n", type=int, default=320000)
    k.add_argument("--rounds", type=int, default=7)
    k.add_argument("--iters", type=int, default=200)
    d = sub.add_parser("driver")
    d.add_argument("--clips", type=int, default=32)
    d.add_argument("--seconds", type=float, default=10.0)
    d.add_argument("--precision", default="f32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("preprocess_times.py needs the GPU")
    {"kernel": kernel, "driver": driver}[a.cmd](a)
