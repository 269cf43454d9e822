"""Drop-in for the reference's speaker/infer.py: one wav -> the 256-float timbre embedding ``--spk`` takes.

    python -m svcmi.speaker.infer MODEL CONFIG -s in.wav -t out.spk.npy
    python -m svcmi.speaker.infer MODEL CONFIG --folder DIR --mean singer.spk.npy

Same positional arguments, flags and commented-JSON config as the reference; the output is a float32 [proj_dim] ``.npy``.  The
reference's script also re-saves the model as ``model_small.pth`` in the working directory on every run; this one does not.
``--folder`` does what prepare/preprocess_speaker.py + preprocess_speaker_ave.py do for one singer: every wav of the folder is embedded
(the windows of several files share encoder calls of up to 64 rows) and the mean over files is written.
"""
import argparse
import json
import os
import re

import numpy as np
import torch

from .models.lstm import MAX_BATCH, LSTMSpeakerEncoder
from .utils.audio import AudioProcessor


def read_json_with_comments(json_path):
    """speaker/infer.py:27-36: ``//`` comments and backslash line continuations removed."""
    with open(json_path, "r", encoding="utf-8") as f:
        input_str = f.read()
    input_str = re.sub(r"\\\n", "", input_str)
    input_str = re.sub(r"//.*\n", "\n", input_str)
    return json.loads(input_str)


def read_json(json_path):
    try:
        with open(json_path, "r", encoding="utf-8") as f:
            return dict(json.load(f))
    except json.decoder.JSONDecodeError:
        return dict(read_json_with_comments(json_path))


def build_parser():
    parser = argparse.ArgumentParser(description="Compute the speaker embedding of a wav file (or the mean over a folder of them).",
                                     formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument("model_path", type=str, help="Path to model checkpoint file.")
    parser.add_argument("config_path", type=str, help="Path to model config file.")
    parser.add_argument("-s", "--source", help="input wave", dest="source")
    parser.add_argument("-t", "--target", help="output 256d speaker embeddimg", dest="target")
    parser.add_argument("--use_cuda", type=bool, help="accepted for compatibility: svcmi always runs on the GPU", default=True)
    parser.add_argument("--eval", type=bool, help="accepted for compatibility", default=True)
    parser.add_argument("--folder", help="embed every .wav of this folder (with --mean)")
    parser.add_argument("--mean", help="output: the mean embedding of the folder's files")
    parser.add_argument("--loader", choices=("host", "gpu"), default="host", help="wav decode + resampling on the host (default) or on the GPU")
    return parser


def load(model_path, config_path, loader="host", ops=None, device=None):
    """(encoder, audio processor) as speaker/infer.py:67-88 builds them."""
    config = read_json(config_path)
    mp = config.get("model_params", config.get("model"))
    enc = LSTMSpeakerEncoder(mp["input_dim"], mp["proj_dim"], mp["lstm_dim"], mp["num_lstm_layers"],
                             use_lstm_with_projection=mp.get("use_lstm_with_projection", True), ops=ops, device=device)
    enc.load_checkpoint(model_path, eval=True, use_cuda=True)
    ap = AudioProcessor(**dict(config["audio"], ops=enc.ops, device=enc.device, loader=loader))
    ap.do_sound_norm = True
    ap.do_trim_silence = True
    return enc, ap


@torch.no_grad()
def embed_file(enc, ap, path):
    """speaker/infer.py:91-101: float32 numpy [proj_dim]."""
    waveform = ap.load_wav(path, sr=ap.sample_rate)
    spec = ap.melspectrogram_device(waveform).unsqueeze(0)
    return enc.compute_embedding(spec).cpu().numpy().squeeze()


@torch.no_grad()
def embed_folder(enc, ap, folder, num_frames=250, num_eval=10):
    """Mean over the folder's wav files (sorted by name) of their embeddings, float32 numpy [proj_dim].  Windows of equal length from
    several files are stacked into encoder calls of up to 64 rows."""
    files = sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.endswith(".wav"))
    if not files:
        raise FileNotFoundError(f"no .wav files in {folder}")
    windows = []                                            # (file index, [nf, D] view), ten per file, in file order
    for fi, path in enumerate(files):
        mel = ap.melspectrogram_device(ap.load_wav(path, sr=ap.sample_rate))
        nf, offsets = enc.window_offsets(mel.shape[0], num_frames, num_eval)
        windows += [(fi, mel[o:o + nf]) for o in offsets]
    emb = torch.empty(len(windows), enc.proj_dim, dtype=torch.float32, device=enc.device)
    by_len = {}
    for i, (_, w) in enumerate(windows):
        by_len.setdefault(w.shape[0], []).append(i)
    for idx in by_len.values():
        for s in range(0, len(idx), MAX_BATCH):
            part = idx[s:s + MAX_BATCH]
            emb[part] = enc.inference(torch.stack([windows[i][1] for i in part]))
    per_file = enc.ops.group_mean(emb, num_eval)            # [files, P]
    return enc.ops.group_mean(per_file, len(files)).cpu().numpy().squeeze()


def main(argv=None):
    args = build_parser().parse_args(argv)
    if bool(args.folder) != bool(args.mean) or bool(args.folder) == bool(args.source) or bool(args.source) != bool(args.target):
        raise SystemExit("give either -s IN.wav -t OUT.npy, or --folder DIR --mean OUT.npy")
    enc, ap = load(args.model_path, args.config_path, loader=args.loader)
    if args.folder:
        np.save(args.mean, embed_folder(enc, ap, args.folder).astype(np.float32), allow_pickle=False)
    else:
        np.save(args.target, embed_file(enc, ap, args.source).astype(np.float32), allow_pickle=False)


if __name__ == "__main__":
    main()
