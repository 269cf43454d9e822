"""Timings of the speaker encoder on the GPU (profiles/speaker_encoder.md):

    python scripts/speaker_times.py [--no-torch] [--once]

  * the step kernel per launch at B = 10 and B = 64 (H = 768), HIP events around 250 launches;
  * the three launch kinds of a layer (input GEMM, 250 steps, projection GEMM) from the library's per-launch trace;
  * wall time wav -> embedding for a 10 s clip (load, trim, level, mel, ten 250-frame windows through the encoder);
  * the same model as a plain torch nn.LSTM / nn.Linear stack on the same device, for scale (--no-torch skips it).

--once: a single encoder call and nothing else (what a rocprofv3 --kernel-trace --stats run wraps)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "whisper-vits-svc_amd")):
    sys.path.insert(0, p)

from workload import speaker as WS      # noqa: E402


def ev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    from svcmi import Ops
    from svcmi import weights as PW
    from svcmi.speaker.models.lstm import LSTMSpeakerEncoder
    from svcmi.speaker.utils.audio import AudioProcessor
    ops = Ops()
    sd = WS.make_speaker_state(**WS.FULL)
    enc = LSTMSpeakerEncoder(80, 256, 768, 3, ops=ops)
    enc.load_checkpoint({"model": sd})
    g = torch.Generator().manual_seed(1)
    x10 = (2.0 * torch.randn(10, 250, 80, generator=g)).cuda()
    if args.once:
        enc.inference(x10)
        torch.cuda.synchronize()
        enc.inference(x10)
        torch.cuda.synchronize()
        return
    H, T = 768, 250
    whh = enc.w.layers[0]["whh"]
    for B in (10, 64):
        gx = torch.randn(B, T, 4 * H, device="cuda")
        hs = torch.zeros(B, T, H, device="cuda")
        c = torch.zeros(B, H, device="cuda")

        def layer():
            for t in range(T):
                ops.lstm_step(gx, whh, hs, c, t)
        print(f"step kernel  B={B:2d} H=768: {1000.0 * ev_ms(layer, 4) / T:7.2f} us per launch ({T} launches back to back)")
    for B, x in ((10, x10), (64, (2.0 * torch.randn(64, 250, 80, generator=g)).cuda())):
        print(f"encoder      B={B:2d} T=250:  {ev_ms(lambda: enc.inference(x), 5):7.3f} ms per call")
        enc.inference(x)
        torch.cuda.synchronize()
        ops.trace_begin(4096)
        enc.inference(x)
        rows = ops.trace_end()
        for name, r in rows.items():
            print(f"    {name:26s} {r['launches']:4d} launches  {r['ms']:8.3f} ms")
        ly0, ly1 = enc.w.layers[0], enc.w.layers[1]
        hseq = torch.randn(B, 250, 768, device="cuda")
        y = torch.randn(B, 250, 256, device="cuda")
        print(f"    GEMMs alone: input 80 -> 3072 {1000 * ev_ms(lambda: ops.conv(x, ly0['ih_w'], ly0['bias'], split_k=1), 10):.1f} us, "
              f"input 256 -> 3072 {1000 * ev_ms(lambda: ops.conv(y, ly1['ih_w'], ly1['bias'], split_k=1), 10):.1f} us, "
              f"projection 768 -> 256 {1000 * ev_ms(lambda: ops.conv(hseq, ly0['lin_w'], None, split_k=1), 10):.1f} us, "
              f"last-row projection {1000 * ev_ms(lambda: ops.conv(hseq[:, -1:], ly0['lin_w'], None, split_k=1, x_bstride=hseq.stride(0)), 10):.1f} us")
    # wav -> embedding, 10 s
    from scipy.io import wavfile
    from tests import speaker_cases as S
    proc = AudioProcessor(**dict(S.AUDIO_CFG, ops=ops, device="cuda"))
    proc.do_sound_norm = True
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "clip.wav")
        wavfile.write(path, 16000, S.voice_clip(10.0, seed=2))

        def chain():
            mel = proc.melspectrogram_device(proc.load_wav(path)).unsqueeze(0)
            return enc.compute_embedding(mel).cpu()
        chain()
        t0 = time.perf_counter()
        for _ in range(5):
            chain()
        print(f"wav -> embedding, 10 s clip (host loader, trim, mel, 10 x 250 frames): {(time.perf_counter() - t0) / 5 * 1000.0:.2f} ms wall")
        wav = proc.load_wav(path)
        t0 = time.perf_counter()
        for _ in range(5):
            enc.compute_embedding(proc.melspectrogram_device(wav).unsqueeze(0)).cpu()
        print(f"  of which mel + encoder (waveform in memory): {(time.perf_counter() - t0) / 5 * 1000.0:.2f} ms wall")
    if args.no_torch:
        return
    try:
        layers = [(lstm.cuda(), lin.cuda()) for lstm, lin in S.torch_encoder(sd, torch.float32)]

        @torch.no_grad()
        def torch_fwd(x):
            d = x
            for lstm, lin in layers:
                d = lin(lstm(d)[0])
            return torch.nn.functional.normalize(d[:, -1], p=2, dim=1)
        ref = torch_fwd(x10)
        print(f"torch nn.LSTM stack B=10 T=250: {ev_ms(lambda: torch_fwd(x10), 5):7.3f} ms per call; "
              f"max |svcmi - torch| = {float((enc.inference(x10) - ref).abs().max()):.2e}")
    except Exception as e:       # noqa: BLE001  (MIOpen may be unable to run here: reported, not worked around)
        print(f"torch nn.LSTM on this device failed: {type(e).__name__}: {e}")


if __name__ == "__main__":
    main()
