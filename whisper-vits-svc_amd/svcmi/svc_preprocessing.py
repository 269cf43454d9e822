"""Drop-in for the reference's svc_preprocessing.py chain (prepare/preprocess_a / _crepe / _ppg / _hubert / _speaker / _speaker_ave /
_spec / _train): ``dataset_raw/<singer>/*.wav`` -> the ``data_svc/`` tree and ``files/{train,valid}.txt``, in ONE process.

    python -m svcmi.svc_preprocessing --raw dataset_raw --out data_svc --files files --config configs/base.yaml \\
        --whisper whisper_pretrain/large-v2.pt --hubert hubert_pretrain/hubert-soft-0d54a1f4.pt --crepe crepe/assets/full.pth \\
        --speaker-model speaker_pretrain/best_model.pth.tar --speaker-config speaker_pretrain/config.json [--loader gpu]

The reference runs ten child processes that each reload their model and re-read the wavs the first two wrote.  Here every model is
loaded once and a clip stays on the device from its PCM to the written features:

    waves-16k/<s>/<f>.wav, waves-32k/<s>/<f>.wav   int16: peak normalisation to 0.6 and truncation (preprocess_a.py:12-14)
    pitch/<s>/<f>.pit.npy      float32 [1 + n16 // 160]     CREPE at hop 160, periodicity gate (pitch.inference.compute_f0_train)
    whisper/<s>/<f>.ppg.npy    float32 [n16 // 320, state]  30 s pad-or-trim, no mel noise (whisper.inference.pred_ppg_train); kept when present
    hubert/<s>/<f>.vec.npy     float32 [T, proj]            the whole clip (hubert.inference.pred_vec_train)
    speaker/<s>/<f>.spk.npy    float32 [proj_dim]           speaker.infer's chain;   singer/<s>.spk.npy: the float32 mean over the folder
    specs/<s>/<f>.pt           float32 [bins, n32 // hop]   the fused linear spectrogram (vits.spectrogram.spectrogram_torch)

The features are computed from the QUANTISED samples (int16 / 32768, what the reference's later steps read back from the files just
written) without re-reading those files; the three extractors of a clip are in flight together on side streams like
``svc_inference.extract_features``.  A file that fails is reported as (path, error) and the folder goes on; the file lists are still
written (only items whose six files exist, as preprocess_train.py:23-54 checks) and the exit status is non-zero.  Singers and files
are taken in sorted order (the reference: ``os.listdir`` order), so ``--seed`` reproduces the F0 draws and the train / valid split.
Not covered: preprocess_zzz.py (a DataLoader dry run of the trainer), preprocess_trim.py, the parselmouth / salience F0 variants.
"""
import argparse
import contextlib
import os
import random
import sys
import time

import numpy as np
import torch

STAGES = ("load", "waves", "pitch", "whisper", "hubert", "speaker", "spec")
VALID_ITEMS = 10


def build_parser():
    p = argparse.ArgumentParser(description="dataset_raw -> data_svc + files/*.txt on the GPU, one process.")
    p.add_argument("--raw", default="dataset_raw", help="input: <raw>/<singer>/*.wav at any rate")
    p.add_argument("--out", default="data_svc", help="output tree")
    p.add_argument("--files", default="files", help="folder of train.txt / valid.txt")
    p.add_argument("--config", required=True, help="yaml config (data.sampling_rate / filter_length / hop_length / win_length / max_wav_value)")
    p.add_argument("--whisper", default=os.path.join("whisper_pretrain", "large-v2.pt"))
    p.add_argument("--hubert", default=os.path.join("hubert_pretrain", "hubert-soft-0d54a1f4.pt"))
    p.add_argument("--crepe", default=os.path.join("crepe", "assets", "full.pth"))
    p.add_argument("--speaker-model", default=os.path.join("speaker_pretrain", "best_model.pth.tar"))
    p.add_argument("--speaker-config", default=os.path.join("speaker_pretrain", "config.json"))
    p.add_argument("--loader", choices=("host", "gpu"), default="host", help="wav decode + resampling on the host (default) or on the GPU")
    p.add_argument("--precision", default="f32", choices=["f32", "bf16x3", "bf16", "f16"],
                   help="GEMM operand precision of the Whisper / HuBERT / CREPE networks (the reference's own preprocessing runs them in fp16)")
    p.add_argument("--index-by-singer", action="store_true", help="file lists name singer/<s>.spk.npy instead of the per-file embedding")
    p.add_argument("--seed", type=int, default=None, help="seeds the F0 noise / dither draws and the train / valid shuffle")
    p.add_argument("--stage-times", action="store_true", help="synchronise after every stage and report seconds per stage (no overlap)")
    return p


# ------------------------------------------------------------------------------------------------ preprocess_a.py:12-14
def normalize_wave_int16(x, name=""):
    """``wav = wav / |wav|.max() * 0.6;  wav = wav / max(0.01, |wav|.max()) * 32767 * 0.6;  wav.astype(np.int16)`` in float32 on the
    tensor's device -> (int16 tensor for the wav file, ``int16 / 32768`` float32: what every later step of the reference reads back).
    The reference turns an all-zero clip into NaNs (0 / 0); here it raises ValueError with ``name``."""
    x = x.to(torch.float32)
    peak = x.abs().max()                              # 0-dim tensors on the device: true divisions, not multiplications by a reciprocal
    if not bool(peak > 0):
        raise ValueError(f"{name}: all-zero (or empty / non-finite) clip, the reference's peak normalisation gives NaNs")
    w = x / peak * 0.6
    peak2 = torch.maximum(w.abs().max(), torch.tensor(0.01, dtype=torch.float32, device=x.device))
    w = w / peak2 * 32767 * 0.6
    i16 = w.to(torch.int16)                           # truncation towards zero, like astype(np.int16); |w| <= 0.6 * 32767
    return i16, i16.to(torch.float32) / 32768.0


# ------------------------------------------------------------------------------------------------ preprocess_train.py
def collect_items(out, index_by_singer=False, log=print):
    """preprocess_train.py:13-54: one ``wave|spec|pitch|hubert|whisper|spk`` line per wav of ``<out>/waves-32k`` whose six files exist."""
    root = os.path.join(out, "waves-32k")
    items = []
    for spks in sorted(os.listdir(root)) if os.path.isdir(root) else ():
        if not os.path.isdir(os.path.join(root, spks)):
            continue
        for file in sorted(os.listdir(os.path.join(root, spks))):
            if not file.endswith(".wav"):
                continue
            file = file[:-4]
            path_spk = f"{out}/singer/{spks}.spk.npy" if index_by_singer else f"{out}/speaker/{spks}/{file}.spk.npy"
            paths = [f"{out}/waves-32k/{spks}/{file}.wav", f"{out}/specs/{spks}/{file}.pt", f"{out}/pitch/{spks}/{file}.pit.npy",
                     f"{out}/hubert/{spks}/{file}.vec.npy", f"{out}/whisper/{spks}/{file}.ppg.npy", path_spk]
            missing = [p for p in paths if not os.path.isfile(p)]
            for p in missing:
                log(f"\033[31m File isn't existed: {p}\033[0m")
            if not missing:
                items.append("|".join(paths))
    return items


def write_file_lists(out, files_dir, index_by_singer=False, seed=None, log=print):
    """preprocess_train.py:56-68: shuffle, the first 10 items sorted -> valid.txt, the rest -> train.txt.  Returns (valid, train)."""
    items = collect_items(out, index_by_singer, log)
    (random.Random(seed) if seed is not None else random).shuffle(items)
    valids, trains = sorted(items[:VALID_ITEMS]), items[VALID_ITEMS:]
    os.makedirs(files_dir, exist_ok=True)
    for name, lines in (("valid.txt", valids), ("train.txt", trains)):
        with open(os.path.join(files_dir, name), "w", encoding="utf-8") as fw:
            for line in lines:
                print(line, file=fw)
    return valids, trains


# ------------------------------------------------------------------------------------------------ preprocess_speaker_ave.py
def write_singer_mean(speaker_dir, singer_path):
    """The float32 mean of the folder's ``.npy`` embeddings, summed in sorted file order; nothing is written for an empty folder."""
    files = sorted(f for f in os.listdir(speaker_dir) if f.endswith(".npy")) if os.path.isdir(speaker_dir) else []
    if not files:
        return None
    ave = 0
    for f in files:
        ave = ave + np.load(os.path.join(speaker_dir, f)).astype(np.float32)
    ave = ave / len(files)
    os.makedirs(os.path.dirname(singer_path), exist_ok=True)
    np.save(singer_path, ave, allow_pickle=False)
    return ave


def embed_wave(enc, ap, wave, name=""):
    """speaker/infer.py:91-101 from the loaded 16 kHz waveform (numpy float32): ``AudioProcessor.load_wav``'s trim + level normalisation,
    mel front-end, ``compute_embedding`` -> float32 numpy [proj_dim]."""
    x = np.asarray(wave, dtype=np.float32)
    if ap.do_trim_silence:
        try:
            x = ap.trim_silence(x)
        except ValueError:
            print(f" [!] File cannot be trimmed for silence - {name}")
    if ap.do_sound_norm:
        x = ap.sound_norm(x)
    spec = ap.melspectrogram_device(x).unsqueeze(0)
    return enc.compute_embedding(spec).cpu().numpy().squeeze()


class Preprocessor:
    """The models, loaded once, and the per-clip chain."""

    def __init__(self, args, ops=None, device=None):
        from .hubert import inference as hubert_inf
        from .ops import Ops
        from .pitch import inference as pitch_inf
        from .speaker import infer as speaker_inf
        from .svc_inference import load_config
        from .whisper import inference as whisper_inf
        self.ops = ops if ops is not None else Ops()
        self.args, self.device = args, device if device is not None else ("cuda" if self.ops.on_gpu else "cpu")
        self.gpu = torch.device(self.device).type == "cuda"          # (a CPU device: the emulator library of the unit tests, no streams)
        self.hp = load_config(args.config).data
        prec = None if args.precision == "f32" else args.precision
        self.whisper = whisper_inf.load_model(args.whisper, self.device, ops=self.ops)
        self.whisper.encoder.precision = prec
        self.hubert = hubert_inf.load_model(args.hubert, self.device, ops=self.ops)
        self.hubert.precision = prec
        self.crepe = pitch_inf.load_crepe(args.crepe, self.device, ops=self.ops)
        self.crepe.precision = prec
        self.enc, self.ap = speaker_inf.load(args.speaker_model, args.speaker_config, loader=args.loader, ops=self.ops, device=self.device)
        self.side = [torch.cuda.Stream(device=self.device) for _ in range(2)] if self.gpu else []
        self.stage_seconds = {k: 0.0 for k in STAGES}

    @contextlib.contextmanager
    def _stage(self, name):
        if not self.args.stage_times:
            yield
            return
        if self.gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            yield
        finally:
            if self.gpu:
                torch.cuda.synchronize()
            self.stage_seconds[name] += time.perf_counter() - t0

    def load(self, path, sr):
        from .whisper.audio import load_audio, load_audio_device
        if self.args.loader == "gpu":
            return load_audio_device(path, sr=sr, device=self.device, ops=self.ops)
        return torch.from_numpy(load_audio(path, sr=sr)).to(self.device)

    @torch.no_grad()
    def clip(self, singer, name, path):
        """One wav of ``dataset_raw/<singer>`` -> its eight files."""
        from scipy.io import wavfile
        from .hubert.inference import pred_vec_train
        from .pitch.inference import compute_f0_train_begin
        from .vits.spectrogram import spectrogram_torch
        from .whisper.inference import pred_ppg_train
        out, hp = self.args.out, self.hp

        def dst(kind, ext):
            return os.path.join(out, kind, singer, name + ext)
        with self._stage("load"):
            raw16, raw32 = self.load(path, 16000), self.load(path, hp.sampling_rate)
        with self._stage("waves"):
            i16, w16 = normalize_wave_int16(raw16, path)
            i32, w32 = normalize_wave_int16(raw32, path)
            wavfile.write(dst("waves-16k", ".wav"), 16000, i16.cpu().numpy())
            wavfile.write(dst("waves-32k", ".wav"), hp.sampling_rate, i32.cpu().numpy())
        cur = torch.cuda.current_stream() if self.gpu else None
        overlap = self.gpu and not self.args.stage_times
        want_ppg = not os.path.isfile(dst("whisper", ".ppg.npy"))           # preprocess_ppg.py:69-70
        ppg = vec = None
        try:
            for s in self.side:
                s.wait_stream(cur)
                w16.record_stream(s)
            with self._stage("pitch"):
                f0_finish = compute_f0_train_begin(w16, self.device, model=self.crepe)      # the longest of the three first
                if not overlap:
                    f0 = f0_finish()
            with self._stage("whisper"), (torch.cuda.stream(self.side[0]) if overlap else contextlib.nullcontext()):
                if want_ppg:
                    ppg = pred_ppg_train(self.whisper, w16)
            with self._stage("hubert"), (torch.cuda.stream(self.side[1]) if overlap else contextlib.nullcontext()):
                vec = pred_vec_train(self.hubert, w16)
            with self._stage("spec"):
                audio_norm = i32.to(torch.float32) / float(getattr(hp, "max_wav_value", 32768.0))      # preprocess_spec.py:16
                spec = spectrogram_torch(audio_norm.unsqueeze(0), hp.filter_length, hp.sampling_rate, hp.hop_length, hp.win_length, center=False,
                                         ops=self.ops)[0]
            with self._stage("speaker"):
                spk = embed_wave(self.enc, self.ap, w16.cpu().numpy(), path)
            if overlap:
                f0 = f0_finish()
        finally:
            for s, t in zip(self.side, (ppg, vec)):
                cur.wait_stream(s)
                if t is not None:
                    t.record_stream(cur)
        np.save(dst("pitch", ".pit.npy"), f0, allow_pickle=False)
        if want_ppg:
            np.save(dst("whisper", ".ppg.npy"), ppg.cpu().numpy(), allow_pickle=False)
        np.save(dst("hubert", ".vec.npy"), vec.cpu().numpy(), allow_pickle=False)
        np.save(dst("speaker", ".spk.npy"), spk.astype(np.float32), allow_pickle=False)
        torch.save(spec.cpu(), dst("specs", ".pt"))


def main(args, ops=None, limit=None, device=None):
    """Runs the chain; returns {"failed": [(path, error), ...], "clips": n, "valid": [...], "train": [...], "stage_seconds": {...},
    "returncode": 0 | 1}.  ``limit``: stop after that many clips (warm-up runs of the timing script)."""
    if args.seed is not None:
        torch.manual_seed(args.seed)
        np.random.seed(args.seed % (2 ** 32))
    pre = Preprocessor(args, ops=ops, device=device)
    failed, done = [], 0
    singers = sorted(s for s in os.listdir(args.raw) if os.path.isdir(os.path.join(args.raw, s)))
    for singer in singers:
        for kind in ("waves-16k", "waves-32k", "pitch", "whisper", "hubert", "speaker", "specs"):
            os.makedirs(os.path.join(args.out, kind, singer), exist_ok=True)
        for file in sorted(f for f in os.listdir(os.path.join(args.raw, singer)) if f.endswith(".wav")):
            if limit is not None and done >= limit:
                break
            path = os.path.join(args.raw, singer, file)
            try:
                pre.clip(singer, file[:-4], path)
                done += 1
            except Exception as e:          # noqa: BLE001  (per-item isolation: report, go on with the folder)
                failed.append((path, f"{type(e).__name__}: {e}"))
                print(f"\033[31m failed: {path}: {type(e).__name__}: {e}\033[0m", file=sys.stderr)
        write_singer_mean(os.path.join(args.out, "speaker", singer), os.path.join(args.out, "singer", f"{singer}.spk.npy"))
    valid, train = write_file_lists(args.out, args.files, args.index_by_singer, args.seed)
    for path, err in failed:
        print(f"failed: {path}: {err}")
    print(f"{done} clips, {len(failed)} failed, {len(valid)} valid + {len(train)} train items")
    return {"failed": failed, "clips": done, "valid": valid, "train": train, "stage_seconds": dict(pre.stage_seconds),
            "returncode": 1 if failed else 0}


def cli(argv=None):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")          # before HIP initialises: the side streams need their own hardware queues
    return main(build_parser().parse_args(argv))["returncode"]


if __name__ == "__main__":
    sys.exit(cli())
