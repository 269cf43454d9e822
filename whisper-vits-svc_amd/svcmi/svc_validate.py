"""Score checkpoints on a validation list: which of these models converts the held-out items best?

    python -m svcmi.svc_validate --config configs/base.yaml --model A.pth [B.pth ...] --files files/valid.txt
                                 [--out report.json] [--seed 1234] [--limit N] [--max-frames F]

The figure is the one the reference's trainer reports after every epoch (vits_extend/validation.py): every item of ``files/valid.txt``
(``wave|spec|pitch|hubert|whisper|spk``, written by svc_preprocessing) is converted from its own features and compared with its recording
by the L1 distance of log-mel spectrograms (``hp.data``'s mel parameters, vits_extend/stft.py).  Beside it the trainer's two other
reconstruction figures, spectral convergence and log-STFT-magnitude at ``hp.mrd.resolutions`` (vits_extend/stft_loss.py).  All of it runs
on the GPU: csrc/spectral_loss.hip never writes the four STFT pairs it sums.

Items are aligned as the reference's loader does (vits/data_utils.py:80-106): hubert and whisper features repeated x2,
``len_min = min(len(pit), len(vec) - 2, len(ppg) - 2)``, the wave cut to ``len_min * hop_length`` and divided by ``max_wav_value``.
An item with a missing file, or too short for the largest resolution (``n <= n_fft / 2``: torch.stft's reflect padding would raise) or for
the mel's padding, is skipped AND LISTED in the report.  Conversion is the engine's inference path, ``load_svc_model`` and the chunked
``svc_infer``: what the user will hear.  Its noise is drawn on the host from a ``torch.Generator`` seeded from ``--seed`` and the item's
line number, so every checkpoint sees identical noise and a rerun reproduces the report bit for bit.  The predicted wave (``svc_infer``
drops the last sample) and the recording are cut to the shorter of the two.

Two divergences from the reference's validation step, on purpose:
  * The reference validates the TRAINING model, whose decoder adds unit-variance noise to z (vits_decoder/generator.py:116), on items
    randomly cropped to 4 s, and divides the sum of per-batch means by the dataset size.  This tool scores the INFERENCE model on whole
    items (or their first ``--max-frames`` frames) and averages per-item values.
  * A training checkpoint must first go through ``python -m svcmi.tools export``: the models given here are inference checkpoints.
Sharding the list over several GPUs is out of scope.  Exit status: 0, or 1 if no item could be scored.
"""
import ast
import json
import os
import sys

import numpy as np
import torch

from .svc_inference import chunk_schedule, load_config, load_svc_model, svc_infer
from .vits import consts as K
from .vits_extend.stft import TacotronSTFT
from .vits_extend.stft_loss import resolution_sums, sc_mag_from_sums

FIELDS = ("wave", "spec", "pitch", "hubert", "whisper", "spk")


def read_items(path, limit=None):
    """files/valid.txt -> [(line number, {field: path})]; blank lines are not items."""
    items = []
    with open(path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f):
            parts = line.strip().split("|")
            if parts == [""]:
                continue
            if len(parts) != len(FIELDS):
                raise ValueError(f"{path}:{no + 1}: expected {'|'.join(FIELDS)}, got {len(parts)} fields")
            items.append((no, dict(zip(FIELDS, parts))))
    return items if limit is None else items[:limit]


def resolutions_of(hp):
    """``hp.mrd.resolutions``: a list, or the string the reference's yaml holds (it eval()s it: mrd.py; here ast.literal_eval)."""
    r = hp.mrd.resolutions
    return [tuple(int(v) for v in t) for t in (ast.literal_eval(r) if isinstance(r, str) else r)]


def load_item(paths, hp, resolutions, max_frames=None):
    """vits/data_utils.py:80-106 without the random crop -> dict of tensors, or a string: why the item is skipped."""
    from scipy.io import wavfile
    for k in ("wave", "pitch", "hubert", "whisper", "spk"):
        if not os.path.isfile(paths[k]):
            return f"missing {k} file {paths[k]}"
    sr, data = wavfile.read(paths["wave"])
    if sr != hp.data.sampling_rate:
        return f"sampling rate {sr} is not {hp.data.sampling_rate}"
    wav = torch.from_numpy(data.astype(np.float32)) / float(hp.data.max_wav_value)
    pit = torch.FloatTensor(np.load(paths["pitch"]))
    vec = torch.FloatTensor(np.repeat(np.load(paths["hubert"]), 2, 0))          # 320 PPG -> 160 * 2
    ppg = torch.FloatTensor(np.repeat(np.load(paths["whisper"]), 2, 0))
    spk = torch.FloatTensor(np.load(paths["spk"]))
    len_min = min(pit.shape[0], vec.shape[0] - 2, ppg.shape[0] - 2)              # "for safe"
    if max_frames is not None:
        len_min = min(len_min, int(max_frames))
    if len_min < 1:
        return "no frames"
    wav = wav[:len_min * hp.data.hop_length]
    n = min(wav.shape[0], len_min * hp.data.hop_length - 1)                     # svc_infer drops the last sample
    need = max(max(r[0] for r in resolutions) // 2, int((hp.data.filter_length - hp.data.hop_length) / 2))
    if n <= need:
        return f"too short: {n} samples, the reflect padding needs more than {need}"
    return {"wav": wav, "pit": pit[:len_min], "vec": vec[:len_min], "ppg": ppg[:len_min], "spk": spk, "frames": len_min}


def item_noise(seed, line_no, frames, hp):
    """The three host draws of one conversion (svc_infer's ``noise``) from a generator seeded by (seed, line number): the same for every
    checkpoint and every run."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(line_no)) % (2 ** 63 - 1))
    hop = hp.data.hop_length
    return {"rand_ini": torch.rand(1, K.NSF_HARMONICS, generator=g),
            "src_noise": torch.randn(1, frames * hop, K.NSF_HARMONICS, generator=g),
            "enc_noises": [torch.randn(1, hp.vits.inter_channels, ce - cs, generator=g) for (cs, ce, _, _) in chunk_schedule(frames, hop)]}


class Scorer:
    """mel L1, spectral convergence and log-STFT-magnitude of (predicted, recorded) waves on ``device``: float64 device scalars."""

    def __init__(self, hp, device, ops=None):
        d = hp.data
        self.stft = TacotronSTFT(d.filter_length, d.hop_length, d.win_length, d.mel_channels, d.sampling_rate, d.mel_fmin, d.mel_fmax, center=False,
                                 device=device, ops=ops)
        self.resolutions = resolutions_of(hp)
        self.ops = ops

    @torch.no_grad()
    def __call__(self, fake, real):
        """fake, real: float32 [n] on the device -> float64 device tensor (mel_l1, sc, mag)."""
        from .vits_extend import stft as _stft
        ops = self.ops if self.ops is not None else _stft._default_ops()
        x, y = fake.view(1, -1), real.view(1, -1)
        mel_x, mel_y = self.stft.mel_spectrogram(x), self.stft.mel_spectrogram(y)
        mel_l1 = ops.abs_diff_sum(mel_x, mel_y)[0] / mel_x[0].numel()            # F.l1_loss (validation.py:31)
        sc = torch.zeros((), dtype=torch.float64, device=x.device)
        mag = torch.zeros((), dtype=torch.float64, device=x.device)
        for fs, ss, wl in self.resolutions:
            s, m = sc_mag_from_sums(resolution_sums(ops, x, y, fs, ss, wl), fs, ss, x.shape[1])
            sc += s
            mag += m
        return torch.stack([mel_l1, sc / len(self.resolutions), mag / len(self.resolutions)])


@torch.no_grad()
def validate(model, items, hp, device, seed, ops=None, max_frames=None, keep_waves=None):
    """Convert and score ``items`` ([(line number, paths)], read_items) with one loaded model.  Returns
    ``{"items": [{line, wave, frames, samples, mel_l1, sc, mag}], "skipped": [{line, wave, reason}], "mean": {mel_l1, sc, mag} | None}``.
    ``keep_waves``: a dict that receives line -> (predicted, recorded) CPU tensors (tests)."""
    scorer = Scorer(hp, device, ops=ops)
    scored, skipped, pending = [], [], []
    for line_no, paths in items:
        it = load_item(paths, hp, scorer.resolutions, max_frames)
        if isinstance(it, str):
            skipped.append({"line": line_no + 1, "wave": paths["wave"], "reason": it})
            continue
        fake = svc_infer(model, None, it["spk"], it["pit"], it["ppg"], it["vec"], hp, device, noise=item_noise(seed, line_no, it["frames"], hp),
                         write_pit_wav=False, return_tensor=True)
        n = min(fake.shape[0], it["wav"].shape[0])
        fake, real = fake[:n].contiguous(), it["wav"][:n].to(fake.device).contiguous()
        if keep_waves is not None:
            keep_waves[line_no + 1] = (fake.cpu(), real.cpu())
        pending.append(scorer(fake, real))                                      # stays on the device: one copy for the whole list below
        scored.append({"line": line_no + 1, "wave": paths["wave"], "frames": it["frames"], "samples": n})
    if pending:
        values = torch.stack(pending).cpu().tolist()
        for rec, (mel_l1, sc, mag) in zip(scored, values):
            rec.update(mel_l1=mel_l1, sc=sc, mag=mag)
    mean = {k: float(np.mean([r[k] for r in scored])) for k in ("mel_l1", "sc", "mag")} if scored else None
    return {"items": scored, "skipped": skipped, "mean": mean}


def rank(checkpoints):
    """Model paths by ascending mean mel L1 (ties: the order given); checkpoints without a scored item last."""
    order = sorted(range(len(checkpoints)), key=lambda i: (checkpoints[i]["mean"] is None, (checkpoints[i]["mean"] or {}).get("mel_l1", 0.0), i))
    return [checkpoints[i]["model"] for i in order]


def main(argv=None, ops=None, device="cuda"):
    from .vits.models import SynthesizerInfer
    args = build_parser().parse_args(argv)
    hp = load_config(args.config)
    items = read_items(args.files, args.limit)
    checkpoints = []
    for path in args.model:
        model = SynthesizerInfer(hp.data.filter_length // 2 + 1, hp.data.segment_size // hp.data.hop_length, hp, ops=ops)
        load_svc_model(path, model)
        model.eval()
        model.to(device)
        res = validate(model, items, hp, device, args.seed, ops=ops, max_frames=args.max_frames)
        checkpoints.append({"model": path, "mean": res["mean"], "items": res["items"]})
        skipped = res["skipped"]                                                # a property of the list, the same for every checkpoint
        m = res["mean"]
        print(f"{path}: " + (f"mel_l1 {m['mel_l1']:.6f}  sc {m['sc']:.6f}  mag {m['mag']:.6f}  ({len(res['items'])} items, {len(skipped)} skipped)"
                             if m else f"no item scored ({len(skipped)} skipped)"))
    report = {"config": args.config, "files": args.files, "seed": args.seed, "max_frames": args.max_frames, "checkpoints": checkpoints,
              "ranking": rank(checkpoints), "skipped": skipped if checkpoints else []}
    text = json.dumps(report, indent=1, sort_keys=True) + "\n"
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0 if any(c["mean"] is not None for c in checkpoints) else 1


def build_parser():
    import argparse
    p = argparse.ArgumentParser(description="score inference checkpoints on a validation list: mel L1, spectral convergence, log-STFT magnitude")
    p.add_argument("--config", type=str, required=True, help="yaml file for config.")
    p.add_argument("--model", type=str, required=True, nargs="+", help="inference checkpoints (svcmi.tools export of a training checkpoint)")
    p.add_argument("--files", type=str, required=True, help="the validation list: wave|spec|pitch|hubert|whisper|spk per line (files/valid.txt)")
    p.add_argument("--out", type=str, help="write the JSON report here instead of standard output")
    p.add_argument("--seed", type=int, default=1234, help="seed of the per-item noise: the same for every checkpoint")
    p.add_argument("--limit", type=int, help="score the first N lines only")
    p.add_argument("--max-frames", type=int, help="score the first F frames of every item")
    return p


if __name__ == "__main__":
    from svcmi.lanes import want_hw_queues
    want_hw_queues()                      # before the first HIP call, like svc_inference
    sys.exit(main())
