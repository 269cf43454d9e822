"""One clip rendered in many timbres: the other half of an audition next to ``svc_inference_shift`` (which key?) -- which voice?

    python -m svcmi.svc_inference_singers --config configs/base.yaml --model sovits5.0.pth --wave in.wav --spk configs/singers
    python -m svcmi.svc_inference_singers ... --spk singer0047.npy singer0051.npy --blend-steps 4

The reference ships 56 singer embeddings (configs/singers/) and ``svc_eva.py`` to blend them; the only way to hear them on one input is a
loop of whole ``svc_inference.py`` runs.  Here the singers are a batch (``svc_inference.svc_infer_singers``): nothing up to the prior
statistics reads the speaker, so per chunk the retrieval blend and the prior encoder run once and only the reverse flow and the generator
run at batch ``--singer-batch``; the harmonic source is made once.  ``--spk`` takes one or more embedding files; a directory stands for
its ``*.npy`` files in sorted order.  Each voice is written as ``./_svc_out/svc_out_{stem}.wav`` (the file name without ``.spk.npy`` /
``.npy``).  ``--blend-steps N`` (exactly two embeddings) renders the N + 1 voices ``svc_eva.py`` would save for the weights
(1 - i/N, i/N), as ``svc_out_blend_{i:02d}of{N:02d}.wav``.  The pitch goes through the CSV's ``int()`` quantisation and ``--shift`` exactly
as in ``svc_inference.py``; missing features are extracted in process with its flags (--f0, --loader, --precision, ...).

One deliberate difference from a loop of ``svc_inference.py`` runs: all voices hear the same NSF excitation (one rand_ini, one noise),
which is a valid draw for each of them and the fairer comparison; the prior noise stays independent per voice."""
import glob
import os

import numpy as np
import torch

from . import svc_inference as SI
from .svc_inference_shift import OUT_DIR, ensure_features
from .tools import mix_speaker_rows


def expand_spk(paths):
    """The embedding files of ``--spk``: a directory stands for its *.npy files in sorted order."""
    files = []
    for p in paths:
        if os.path.isdir(p):
            found = sorted(glob.glob(os.path.join(p, "*.npy")))
            if not found:
                raise ValueError(f"--spk: no *.npy file in {p}")
            files += found
        else:
            files.append(p)
    return files


def stem(path):
    name = os.path.basename(path)
    for ext in (".spk.npy", ".npy"):
        if name.endswith(ext):
            return name[: -len(ext)]
    return name


def blend_weights(steps):
    """(1 - i/N, i/N) for i = 0 .. N."""
    return [(1 - i / steps, i / steps) for i in range(steps + 1)]


def plan_voices(args):
    """[(output stem, embedding file(s), weights or None)] from --spk / --blend-steps, checked before any work is done."""
    files = expand_spk(args.spk)
    steps = getattr(args, "blend_steps", None)
    if steps is not None:
        if steps < 1:
            raise ValueError(f"--blend-steps must be at least 1, got {steps}")
        if len(files) != 2:
            raise ValueError(f"--blend-steps blends exactly two --spk embeddings, got {len(files)}")
        return [(f"blend_{i:02d}of{steps:02d}", files, w) for i, w in enumerate(blend_weights(steps))]
    stems = [stem(f) for f in files]
    for s in stems:
        if stems.count(s) > 1:
            raise ValueError(f"--spk: two embeddings would be written as svc_out_{s}.wav")
    return [(s, [f], None) for s, f in zip(stems, files)]


def load_voices(plan):
    """-> [S, spk_dim] float32.  A blend is rounded as ``torch.FloatTensor(np.load("eva.spk.npy"))`` rounds svc_eva.py's float64 result."""
    cache = {}

    def load(f):
        if f not in cache:
            cache[f] = np.load(f)
        return cache[f]
    rows = []
    for _, files, weights in plan:
        if weights is None:
            rows.append(torch.FloatTensor(load(files[0])))
        else:
            rows.append(torch.FloatTensor(mix_speaker_rows([load(f) for f in files], weights)))
    return torch.stack(rows)


def load_model(args, hp, device, ops=None):
    from .vits.models import SynthesizerInfer
    model = SynthesizerInfer(hp.data.filter_length // 2 + 1, hp.data.segment_size // hp.data.hop_length, hp, ops=ops)
    SI.load_svc_model(args.model, model)
    model.eval()
    model.to(device)
    model.precision = None if getattr(args, "precision", "f32") == "f32" else args.precision
    return model


def main(args, device="cuda", ops=None):
    """Returns {output stem: waveform}."""
    from scipy.io.wavfile import write
    from .feature_retrieval import create_retrival
    from .pitch import inference as pitch_inf
    plan = plan_voices(args)
    os.makedirs(OUT_DIR, exist_ok=True)
    ensure_features(args, device, ops)
    hp = SI.load_config(args.config)
    model = load_model(args, hp, device, ops)
    retrieval = create_retrival(args, device)
    spks = load_voices(plan)
    ppg = torch.FloatTensor(np.repeat(np.load(args.ppg), 2, 0))
    vec = torch.FloatTensor(np.repeat(np.load(args.vec), 2, 0))
    print("pitch shift: ", args.shift)
    pit = torch.FloatTensor(SI.shift_pitch(pitch_inf.load_csv_pitch(args.pit), args.shift))
    outs = SI.svc_infer_singers(model, retrieval, spks, pit, ppg, vec, hp, device, singer_batch=getattr(args, "singer_batch", SI.SINGER_BATCH))
    names = [name for name, _, _ in plan]
    for name, out_audio in zip(names, outs):
        print(name)
        write(os.path.join(OUT_DIR, f"svc_out_{name}.wav"), hp.data.sampling_rate, out_audio)
    return dict(zip(names, outs))


def build_parser():
    import argparse
    base = SI.build_parser()
    p = argparse.ArgumentParser(description="one clip in many timbres: svc_inference.py over a set of speaker embeddings, singers batched")
    p.add_argument("--config", type=str, required=True, help="yaml file for config.")
    p.add_argument("--model", type=str, required=True, help="path of model for evaluation")
    p.add_argument("--wave", type=str, required=True, help="Path of raw audio.")
    p.add_argument("--spk", type=str, required=True, nargs="+",
                   help="Paths of speaker embeddings; a directory stands for its *.npy files in sorted order.")
    p.add_argument("--ppg", type=str, help="Path of content vector.")
    p.add_argument("--vec", type=str, help="Path of hubert vector.")
    p.add_argument("--pit", type=str, help="Path of pitch csv file.")
    p.add_argument("--shift", type=int, default=0, help="Pitch shift key.")
    p.add_argument("--singer-batch", type=int, default=SI.SINGER_BATCH,
                   help="singers rendered per synthesizer call (1..32): the prior encoder runs once per group of this size")
    p.add_argument("--blend-steps", type=int, default=None, metavar="N",
                   help="with exactly two --spk embeddings: render the N + 1 blends of weights (1 - i/N, i/N), as svc_eva.py would mix them")
    # the engine's own flags, with the help texts and defaults of svc_inference.py
    shared = ("--enable-retrieval", "--retrieval-index-prefix", "--retrieval-ratio", "--n-retrieval-vectors", "--hubert-index-path",
              "--whisper-index-path", "--whisper", "--hubert", "--crepe", "--f0", "--swipe-threshold", "--loader", "--precision", "--f0-precision")
    for a in base._actions:
        if a.option_strings and a.option_strings[0] in shared:
            kw = dict(default=a.default, help=a.help)
            if a.nargs == 0:
                kw["action"] = "store_true"
            else:
                kw.update(type=a.type, choices=a.choices, metavar=a.metavar, required=a.required)
            p.add_argument(*a.option_strings, **kw)
    return p


if __name__ == "__main__":
    from svcmi.lanes import want_hw_queues
    want_hw_queues()
    main(build_parser().parse_args())      # (the --spk checks and ./_svc_out: first thing in main)
