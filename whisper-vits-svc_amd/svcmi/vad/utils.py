"""The reference's vad/utils.py surface that svc_inference_post.py uses: ``init_jit_model`` and ``get_speech_timestamps``.

The 16 kHz Silero network runs in two kernel launches per call (csrc/vad.hip): the convolutional part of every 512-sample window at
once, then one serial scan of the 2-layer LSTM per recording.  ``init_jit_model`` only takes the tensors out of the TorchScript archive
(``state_dict()``); the archive's code is never executed.  The span logic of ``get_speech_timestamps`` runs on the host over the
probabilities, a few hundred scalars.

Supported: 16 kHz input (or a multiple of it, decimated by plain striding as the reference does) and windows of 512 samples; anything
else raises ValueError.  Out of scope: VADIterator, probability plots, the progress callback, the ONNX wrapper."""
import warnings

import numpy as np
import torch

WINDOW = 512
RATE = 16000


class SileroVad:
    """The 16 kHz model with the reference model's call surface: ``model(chunk, sr)`` for one window with the LSTM state kept between
    calls, ``reset_states()``, ``audio_forward(x, sr)`` for whole recordings."""

    sample_rates = [RATE]

    def __init__(self, weights, device="cuda", ops=None):
        from ..cmodel import vad_cmodel
        from ..ops import Ops
        self.ops = ops if ops is not None else Ops()
        self.device = torch.device(device)
        self.weights = weights
        self.cmodel = vad_cmodel(weights)
        self.reset_states()

    @classmethod
    def from_state_dict(cls, sd, device="cuda", ops=None):
        """``sd``: the archive's ``state_dict()`` (keys ``_model.*``; the 8 kHz twin ``_model_8k.*`` is ignored) or the same tensors
        without the prefix.  ValueError for a tensor of another shape, KeyError for a missing one."""
        from ..weights import VadWeights
        if any(k.startswith("_model.") for k in sd):
            sd = {k[len("_model."):]: v for k, v in sd.items() if k.startswith("_model.")}
        sd = {k: (torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v) for k, v in sd.items()}
        return cls(VadWeights(sd, device), device, ops)

    def eval(self):
        return self

    def reset_states(self, batch_size=1):
        self._state = None
        self._last_sr = 0
        self._last_batch_size = 0

    def _validate_input(self, x, sr):
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x))
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() > 2:
            raise ValueError(f"Too many dimensions for input audio chunk {x.dim()}")
        sr = int(sr)
        if sr != RATE and sr % RATE == 0:
            x = x[:, ::sr // RATE]
            sr = RATE
        if sr != RATE:
            raise ValueError(f"Supported sampling rates: {self.sample_rates} (or a multiple of 16000); the 8 kHz model is not built, got {sr}")
        return x.to(self.device, torch.float32), sr

    def _run(self, flat, offsets, lengths, wmax, state=None):
        dev = self.device
        return self.ops.vad_probs_fwd(self.cmodel, flat.contiguous(), torch.tensor(offsets, dtype=torch.int64).to(dev),
                                      torch.tensor(lengths, dtype=torch.int64).to(dev), wmax, state)

    @torch.no_grad()
    def __call__(self, x, sr):
        """One window [512] or [B, 512] -> probabilities [B, 1] on the device; h and c of both LSTM layers carry over to the next call."""
        x, sr = self._validate_input(x, sr)
        B, n = x.shape
        if n != WINDOW:
            raise ValueError(f"only windows of {WINDOW} samples at 16 kHz are supported, got {n}")
        if not self._last_batch_size or self._last_sr != sr or self._last_batch_size != B or self._state is None:
            self._state = torch.zeros(B, 4, 64, dtype=torch.float32, device=self.device)
        self._last_sr, self._last_batch_size = sr, B
        return self._run(x.reshape(-1), [b * WINDOW for b in range(B)], [WINDOW] * B, 1, self._state)

    @torch.no_grad()
    def audio_forward(self, x, sr, num_samples=WINDOW):
        """Every window's probability of one recording [n], of equally long recordings [B, n] -> CPU tensor [B, ceil(n / 512)]; or of a
        list of recordings of any lengths -> a list of CPU tensors [W_b].  The state starts from zero for every recording; two launches
        whatever the batch."""
        if int(num_samples) != WINDOW:
            raise ValueError(f"only windows of {WINDOW} samples at 16 kHz are supported, got num_samples={num_samples}")
        self.reset_states()
        if isinstance(x, (list, tuple)):
            items = [self._validate_input(t, sr)[0].reshape(-1) for t in x]
            lengths = [int(t.shape[0]) for t in items]
            if not items or min(lengths) < 1:
                raise ValueError("audio_forward: every recording needs at least one sample")
            offsets = [int(o) for o in np.cumsum([0] + lengths[:-1])]
            nw = [-(-n // WINDOW) for n in lengths]
            probs = self._run(torch.cat(items), offsets, lengths, max(nw)).cpu()
            return [probs[b, :w].clone() for b, w in enumerate(nw)]
        x, sr = self._validate_input(x, sr)
        B, n = x.shape
        if n < 1:
            raise ValueError("audio_forward: empty audio")
        return self._run(x.reshape(-1), [b * n for b in range(B)], [n] * B, -(-n // WINDOW)).cpu()


def init_jit_model(model_path, device="cuda", ops=None):
    """vad/utils.py init_jit_model: the model of ``silero_vad.jit``.  Only the archive's tensors are read (``state_dict()`` of the loaded
    module, on the CPU); its TorchScript code is never run.  A ``.npz`` file of the same tensors (names with or without a ``sd/`` or
    ``_model.`` prefix) is accepted too."""
    if str(model_path).endswith(".npz"):
        with np.load(model_path) as z:
            sd = {(k[3:] if k.startswith("sd/") else k): torch.from_numpy(z[k]) for k in z.files if k.startswith(("sd/", "_model.")) or "." in k}
    else:
        sd = torch.jit.load(model_path, map_location="cpu").state_dict()
    return SileroVad.from_state_dict(sd, device, ops)


def _speech_runs(probs, n_samples, win, on_level, off_level, min_speech, min_silence, max_speech, split_silence):
    """The hysteresis pass over the window probabilities -> [[start, end]] in samples, before padding.

    A run opens at the first window at or above ``on_level``.  Inside a run, a window below ``off_level`` starts a quiet stretch (it
    is forgotten when a window reaches ``on_level`` again); once the stretch is ``min_silence`` long the run closes where the stretch
    began, and is kept if longer than ``min_speech``.  A run that outgrows ``max_speech`` is cut: at the last quiet stretch longer
    than ``split_silence`` if there was one -- the next run then opens where speech resumed, if it did -- else right here."""
    runs = []
    start = None          # first sample of the open run
    quiet_from = 0        # first sample of the current quiet stretch (0: none; a stretch never begins at sample 0)
    cut_at = 0            # a quiet stretch long enough to cut an over-long run at
    resume_at = 0         # where speech came back after `cut_at`
    for i, p in enumerate(probs):
        pos = win * i
        loud = p >= on_level
        if loud and quiet_from:
            quiet_from = 0
            if resume_at < cut_at:
                resume_at = pos
        if loud and start is None:
            start = pos
            continue
        if start is not None and pos - start > max_speech:
            if cut_at:
                runs.append([start, cut_at])
                start = resume_at if resume_at >= cut_at else None
                quiet_from = cut_at = resume_at = 0
            else:
                runs.append([start, pos])
                start = None
                quiet_from = cut_at = resume_at = 0
                continue
        if start is not None and p < off_level:
            if not quiet_from:
                quiet_from = pos
            if pos - quiet_from > split_silence:
                cut_at = quiet_from
            if pos - quiet_from >= min_silence:
                if quiet_from - start > min_speech:
                    runs.append([start, quiet_from])
                start = None
                quiet_from = cut_at = resume_at = 0
    if start is not None and n_samples - start > min_speech:
        runs.append([start, n_samples])
    return runs


def _pad_runs(runs, n_samples, pad):
    """Widen every run by ``pad`` samples on both sides, clipped to the recording; neighbours closer than 2 pad share the gap in halves."""
    for k, run in enumerate(runs):
        if k == 0:
            run[0] = int(max(0, run[0] - pad))
        if k + 1 < len(runs):
            nxt = runs[k + 1]
            gap = nxt[0] - run[1]
            if gap < 2 * pad:
                run[1] += int(gap // 2)
                nxt[0] = int(max(0, nxt[0] - gap // 2))
            else:
                run[1] = int(min(n_samples, run[1] + pad))
                nxt[0] = int(max(0, nxt[0] - pad))
        else:
            run[1] = int(min(n_samples, run[1] + pad))
    return runs


def get_speech_timestamps(audio, model, threshold=0.5, sampling_rate=16000, min_speech_duration_ms=250, max_speech_duration_s=float("inf"),
                          min_silence_duration_ms=100, window_size_samples=512, speech_pad_ms=30, return_seconds=False):
    """vad/utils.py get_speech_timestamps: ``[{'start': s, 'end': e}]`` in samples of the input rate (seconds, rounded to 0.1, with
    ``return_seconds``).  The probabilities come from ``model.audio_forward``; windows at or above ``threshold`` open a span, windows
    below ``threshold - 0.15`` close it after ``min_silence_duration_ms``."""
    if int(window_size_samples) != WINDOW:
        raise ValueError(f"window_size_samples={window_size_samples}: only {WINDOW}-sample windows (at 16 kHz) are supported")
    if not torch.is_tensor(audio):
        try:
            audio = torch.as_tensor(np.asarray(audio, dtype=np.float32))
        except Exception as e:       # noqa: BLE001
            raise TypeError("Audio cannot be casted to tensor. Cast it manually") from e
    while audio.dim() > 1 and audio.shape[0] == 1:
        audio = audio.squeeze(0)
    if audio.dim() > 1:
        raise ValueError("More than one dimension in audio. Are you trying to process audio with 2 channels?")
    sampling_rate = int(sampling_rate)
    step = 1
    if sampling_rate > RATE and sampling_rate % RATE == 0:
        step = sampling_rate // RATE
        sampling_rate = RATE
        audio = audio[::step]
        warnings.warn("Sampling rate is a multiply of 16000, casting to 16000 manually!")
    if sampling_rate != RATE:
        raise ValueError(f"sampling_rate={sampling_rate}: only 16000 Hz (or a multiple of it) is supported; the 8 kHz model is not built")
    n = int(audio.shape[0])
    if n == 0:
        return []
    probs = torch.as_tensor(model.audio_forward(audio, sampling_rate, num_samples=WINDOW)).reshape(-1).double().tolist()
    pad = sampling_rate * speech_pad_ms / 1000
    runs = _speech_runs(probs, n, WINDOW, threshold, threshold - 0.15,
                        min_speech=sampling_rate * min_speech_duration_ms / 1000,
                        min_silence=sampling_rate * min_silence_duration_ms / 1000,
                        max_speech=sampling_rate * max_speech_duration_s - WINDOW - 2 * pad,
                        split_silence=sampling_rate * 98 / 1000)
    runs = _pad_runs(runs, n, pad)
    if return_seconds:
        return [{"start": round(a / sampling_rate, 1), "end": round(b / sampling_rate, 1)} for a, b in runs]
    return [{"start": a * step, "end": b * step} for a, b in runs]
