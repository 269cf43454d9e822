"""Drop-in for the reference's svc_inference_shift.py: one clip rendered at every transposition from ``--shift_l`` to ``--shift_r``
(up to 25 keys, -12 .. +12), written as ``./_svc_out/svc_out_{shift}.wav`` so that the singer can pick the key that suits the target voice.

    python -m svcmi.svc_inference_shift --config configs/base.yaml --model sovits5.0.pth --wave in.wav --spk singer.spk.npy --shift_l -6 --shift_r 6

The reference extracts the features once and then calls ``svc_infer`` per key (:60-70; its copy is stale: it passes no ``retrieval`` and
raises).  Here the keys are a batch (``svc_inference.svc_infer_sweep``): across keys only the pitch changes, so the feature copies, the
retrieval blend and the prior encoder's front convolutions happen once per chunk and the rest of the synthesizer runs at batch
``--key-batch``.  Same flags, same four range assertions, same printed lines and file names; the pitch goes through the CSV's ``int()``
quantisation and ``np.array(pit) * 2 ** (shift / 12)`` in float64 as there.  Missing features are extracted in process with the flags of
``svc_inference.py`` (--f0, --loader, --precision, ...).  The reference's per-call ``svc_out_pit.wav`` (overwritten once per key) is
not written."""
import os

import numpy as np
import torch

from . import svc_inference as SI

OUT_DIR = "./_svc_out"


def check_range(args):
    """The four assertions of svc_inference_shift.py:97-101."""
    assert args.shift_l >= -12
    assert args.shift_r >= -12
    assert args.shift_l <= 12
    assert args.shift_r <= 12
    assert args.shift_l <= args.shift_r


def ensure_features(args, device="cuda", ops=None):
    """svc_tmp.ppg.npy / svc_tmp.vec.npy / svc_tmp.pit.csv for whichever of --ppg / --vec / --pit is missing, through the extractor entry
    points ``svc_inference.main`` uses (``extract_features`` in flight when all three are missing, else ``pred_ppg`` / ``pred_vec`` /
    ``compute_f0_*``) with the same precision policy; sets the three paths on ``args``.  Returns the 16 kHz audio if it was loaded."""
    from .hubert import inference as hubert_inf
    from .pitch import inference as pitch_inf
    from .whisper import inference as whisper_inf
    f0_method = getattr(args, "f0", "crepe")
    f0_prec = None if getattr(args, "f0_precision", "f32") == "f32" else args.f0_precision
    prec = None if getattr(args, "precision", "f32") == "f32" else args.precision
    enc_prec = "f16" if prec == "mixed" else prec
    swipe_thr = float(getattr(args, "swipe_threshold", 0.0))

    def with_prec(m):
        (m.encoder if hasattr(m, "encoder") else m).precision = enc_prec
        return m

    def crepe():
        if f0_method != "crepe":
            return None
        m = pitch_inf.load_crepe(args.crepe, device, ops=ops)
        m.precision = f0_prec
        return m
    audio = None
    if args.ppg is None and args.vec is None and args.pit is None:
        from .whisper.audio import load_audio, load_audio_device
        audio = load_audio_device(args.wave, device=device) if getattr(args, "loader", "host") == "gpu" else load_audio(args.wave)
        ppg_d, vec_d, f0 = SI.extract_features(audio, with_prec(whisper_inf.load_model(args.whisper, device, ops=ops)),
                                               with_prec(hubert_inf.load_model(args.hubert, device, ops=ops)), crepe(), device, f0=f0_method,
                                               ops=ops, swipe_threshold=swipe_thr)
        args.ppg, args.vec, args.pit = "svc_tmp.ppg.npy", "svc_tmp.vec.npy", "svc_tmp.pit.csv"
        np.save(args.ppg, ppg_d.cpu().numpy(), allow_pickle=False)
        np.save(args.vec, vec_d.cpu().numpy(), allow_pickle=False)
        pitch_inf.save_csv_pitch(f0, args.pit)
    if args.ppg is None:
        args.ppg = "svc_tmp.ppg.npy"
        whisper_inf.pred_ppg(with_prec(whisper_inf.load_model(args.whisper, device, ops=ops)), args.wave, args.ppg, device)
    if args.vec is None:
        args.vec = "svc_tmp.vec.npy"
        hubert_inf.pred_vec(with_prec(hubert_inf.load_model(args.hubert, device, ops=ops)), args.wave, args.vec, device)
    if args.pit is None:
        args.pit = "svc_tmp.pit.csv"
        if f0_method == "salience":
            f0 = pitch_inf.compute_f0_salience(args.wave, device, ops=ops)
        elif f0_method == "pyin":
            f0 = pitch_inf.compute_f0_pyin(args.wave, device, ops=ops)
        elif f0_method == "swipe":
            f0 = pitch_inf.compute_f0_swipe(args.wave, device, strength_threshold=swipe_thr, ops=ops)
        else:
            f0 = pitch_inf.compute_f0_sing(args.wave, device, model=crepe())
        pitch_inf.save_csv_pitch(f0, args.pit)
    return audio


def main(args, device="cuda", ops=None):
    """svc_inference_shift.py:14-70.  Returns {shift: waveform}."""
    from scipy.io.wavfile import write
    from .feature_retrieval import create_retrival
    from .pitch import inference as pitch_inf
    from .vits.models import SynthesizerInfer
    check_range(args)
    os.makedirs(OUT_DIR, exist_ok=True)
    ensure_features(args, device, ops)
    hp = SI.load_config(args.config)
    model = SynthesizerInfer(hp.data.filter_length // 2 + 1, hp.data.segment_size // hp.data.hop_length, hp, ops=ops)
    SI.load_svc_model(args.model, model)
    retrieval = create_retrival(args, device)
    model.eval()
    model.to(device)
    model.precision = None if getattr(args, "precision", "f32") == "f32" else args.precision
    spk = torch.FloatTensor(np.load(args.spk))
    ppg = torch.FloatTensor(np.repeat(np.load(args.ppg), 2, 0))
    vec = torch.FloatTensor(np.repeat(np.load(args.vec), 2, 0))
    pit = torch.FloatTensor(np.array(pitch_inf.load_csv_pitch(args.pit)))        # integers (the CSV's int()): exact in fp32
    shift_l, shift_r = args.shift_l, args.shift_r
    print(f"pitch shift: [{shift_l}, {shift_r}]")
    shifts = list(range(shift_l, shift_r + 1))
    outs = SI.svc_infer_sweep(model, retrieval, spk, pit, ppg, vec, hp, device, shifts, key_batch=getattr(args, "key_batch", SI.SWEEP_KEY_BATCH))
    for shift, out_audio in zip(shifts, outs):
        print(shift)
        write(os.path.join(OUT_DIR, f"svc_out_{shift}.wav"), hp.data.sampling_rate, out_audio)
    return dict(zip(shifts, outs))


def build_parser():
    import argparse
    base = SI.build_parser()
    p = argparse.ArgumentParser(description="svcmi drop-in for the reference's svc_inference_shift.py")
    p.add_argument("--config", type=str, required=True, help="yaml file for config.")
    p.add_argument("--model", type=str, required=True, help="path of model for evaluation")
    p.add_argument("--wave", type=str, required=True, help="Path of raw audio.")
    p.add_argument("--spk", type=str, required=True, help="Path of speaker.")
    p.add_argument("--ppg", type=str, help="Path of content vector.")
    p.add_argument("--vec", type=str, help="Path of hubert vector.")
    p.add_argument("--pit", type=str, help="Path of pitch csv file.")
    p.add_argument("--shift_l", type=int, default=0, help="Pitch shift key for [shift_l, shift_r]")
    p.add_argument("--shift_r", type=int, default=0, help="Pitch shift key for [shift_l, shift_r]")
    p.add_argument("--key-batch", type=int, default=SI.SWEEP_KEY_BATCH,
                   help="keys rendered per synthesizer call (1..32): the shared front of the prior encoder runs once per group of this size")
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
    main(build_parser().parse_args())      # (the range assertions and ./_svc_out: first thing in main)
