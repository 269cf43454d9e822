"""Drop-in for the reference's svc_inference_post.py: silence the converted waveform wherever the input recording has no voice.

    python -m svcmi.svc_inference_post --ref in.wav --svc svc_out.wav --out svc_out_post.wav [--vad vad/assets/silero_vad.jit]

The Silero detector runs over the 16 kHz input (svcmi.vad, two kernel launches), the speech spans at threshold 0.2 become a mask at
32 kHz (every 16 kHz sample twice), both signals are cut to the shorter length and the converted waveform is zeroed outside the
spans -- on the device, in one more launch.  The result is written as a float32 wav at 32 kHz, like the reference's."""
import os

import numpy as np
import torch

REF_RATE, SVC_RATE = 16000, 32000


@torch.no_grad()
def apply_vad_post(ref16k, svc32k, vad, threshold=0.2):
    """svc_inference_post.py:34-49.  ``ref16k``: the input recording at 16 kHz (numpy or tensor [n]); ``svc32k``: the converted waveform
    at 32 kHz (numpy, or a tensor that may already live on the device); ``vad``: a ``svcmi.vad.SileroVad``.  Returns
    min(len(svc32k), 2 n) samples, zero wherever the detector hears no voice: a device tensor for a tensor input, numpy for numpy."""
    from .vad.utils import get_speech_timestamps
    ref = torch.as_tensor(np.asarray(ref16k)) if not torch.is_tensor(ref16k) else ref16k
    ref = ref.reshape(-1)
    as_numpy = not torch.is_tensor(svc32k)
    svc = (torch.as_tensor(np.asarray(svc32k, dtype=np.float32)) if as_numpy else svc32k).reshape(-1).to(vad.device, torch.float32).contiguous()
    if ref.shape[0] < 1 or svc.shape[0] < 1:
        raise ValueError("apply_vad_post: empty input")
    tags = get_speech_timestamps(ref, vad, threshold=threshold, sampling_rate=REF_RATE)
    spans = torch.tensor([[t["start"], t["end"]] for t in tags], dtype=torch.int32).reshape(-1, 2).to(vad.device)
    out = vad.ops.mask_spans(svc, spans, int(ref.shape[0]), SVC_RATE // REF_RATE)
    return out.cpu().numpy() if as_numpy else out


def build_parser():
    import argparse
    p = argparse.ArgumentParser(description="svcmi drop-in for the reference's svc_inference_post.py")
    p.add_argument("--ref", type=str, required=True, help="Path of ref audio.")
    p.add_argument("--svc", type=str, required=True, help="Path of svc audio.")
    p.add_argument("--out", type=str, required=True, help="Path of out audio.")
    p.add_argument("--vad", type=str, default=os.path.join("vad", "assets", "silero_vad.jit"), help="Path of the Silero VAD TorchScript archive.")
    return p


def main(args, vad=None):
    from scipy.io.wavfile import write
    from .vad.utils import init_jit_model
    from .whisper.audio import load_audio
    print("svc in wave :", args.ref)
    print("svc out wave :", args.svc)
    print("svc post wave :", args.out)
    vad = vad if vad is not None else init_jit_model(args.vad, "cuda")
    out = apply_vad_post(load_audio(args.ref, sr=REF_RATE), load_audio(args.svc, sr=SVC_RATE), vad, threshold=0.2)
    write(args.out, SVC_RATE, out)
    return out


if __name__ == "__main__":
    main(build_parser().parse_args())
