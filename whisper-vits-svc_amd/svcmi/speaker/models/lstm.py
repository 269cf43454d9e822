"""Drop-in for the reference's speaker/models/lstm.py ``LSTMSpeakerEncoder`` (inference side) on the svcmi kernels.

    enc = LSTMSpeakerEncoder(80, 256, 768, 3)
    enc.load_checkpoint("speaker_pretrain/best_model.pth.tar", eval=True, use_cuda=True)
    emb = enc.compute_embedding(mel[1, T, 80])                     # [1, 256]: the mean of ten 250-frame windows

Per layer the input projections of all time steps and the output projection are launches of the implicit GEMM; the recurrence is one
launch of csrc/lstm.hip per time step (svcmi_speaker_encoder_fwd composes them on the caller's stream).  fp32 only: the encoder does not
honour ``Ops.use_precision``.  Only the projection architecture of the pretrained model exists (``use_lstm_with_projection=True``).
"""
import numpy as np
import torch

from ... import weights as PW
from ..._lib import SvcmiError
from ...cmodel import speaker_cmodel
from ...ops import Ops

MAX_BATCH = 64            # rows per svcmi_speaker_encoder_fwd call


class LSTMSpeakerEncoder:
    def __init__(self, input_dim, proj_dim=256, lstm_dim=768, num_lstm_layers=3, use_lstm_with_projection=True, device=None, ops=None):
        if not use_lstm_with_projection:
            raise SvcmiError("LSTMSpeakerEncoder: use_lstm_with_projection=False (LSTMWithoutProjection) is not implemented; the pretrained "
                             "speaker encoder uses the projection layers")
        self.input_dim, self.proj_dim, self.lstm_dim, self.num_lstm_layers = input_dim, proj_dim, lstm_dim, num_lstm_layers
        self.use_lstm_with_projection = True
        self.ops = ops if ops is not None else Ops()
        self.device = torch.device(device if device is not None else ("cuda" if self.ops.on_gpu else "cpu"))
        self.w = self.cm = None
        self.training = False

    # -- nn.Module look-alikes the reference's callers use
    def eval(self):
        return self

    def cuda(self):
        return self

    def to(self, device):
        if torch.device(device).type != self.device.type:
            raise NotImplementedError("construct the encoder on its device (LSTMSpeakerEncoder(..., device=...))")
        return self

    def load_state_dict(self, sd):
        w = PW.SpeakerWeights(sd, self.device)
        got = (w.input_dim, w.proj_dim, w.lstm_dim, len(w.layers))
        want = (self.input_dim, self.proj_dim, self.lstm_dim, self.num_lstm_layers)
        if got != want:
            raise SvcmiError(f"speaker encoder checkpoint has (input, proj, lstm, layers) = {got}, the model was built for {want}")
        self.w, self.cm = w, speaker_cmodel(w, self.ops)
        return self

    def load_checkpoint(self, checkpoint_path, eval=False, use_cuda=False):      # noqa: A002  (the reference's argument names)
        """speaker/models/lstm.py:125-131: the ``{"model": state_dict}`` file (or an already loaded dict of that form)."""
        state = torch.load(checkpoint_path, map_location="cpu") if isinstance(checkpoint_path, (str, bytes)) or hasattr(checkpoint_path, "__fspath__") \
            else checkpoint_path
        self.load_state_dict(state["model"])

    @torch.no_grad()
    def inference(self, x):
        """x [B, T, input_dim] -> L2-normalised embeddings [B, proj_dim] (the last time step of the last layer)."""
        if self.cm is None:
            raise SvcmiError("LSTMSpeakerEncoder: no weights loaded (load_checkpoint / load_state_dict)")
        x = x.to(self.device, torch.float32)
        if x.dim() != 3 or x.shape[2] != self.input_dim or x.shape[1] < 1:
            raise ValueError(f"expected [B, T >= 1, {self.input_dim}], got {tuple(x.shape)}")
        out = [self.ops.speaker_encoder_fwd(self.cm, x[i:i + MAX_BATCH]) for i in range(0, x.shape[0], MAX_BATCH)]
        return out[0] if len(out) == 1 else torch.cat(out, 0)

    forward = inference
    __call__ = inference

    @staticmethod
    def window_offsets(max_len, num_frames=250, num_eval=10):
        """speaker/models/lstm.py:79-91: (window length, start offsets).  A clip shorter than ``num_frames`` is taken whole, ``num_eval``
        times (every offset is 0)."""
        if max_len < num_frames:
            num_frames = max_len
        return num_frames, [int(o) for o in np.linspace(0, max_len - num_frames, num=num_eval)]

    @torch.no_grad()
    def compute_embedding(self, x, num_frames=250, num_eval=10, return_mean=True):
        """x [1, T, D] -> [1, proj_dim] (or the ``num_eval`` window embeddings): speaker/models/lstm.py:73-100."""
        x = x.to(self.device, torch.float32)
        num_frames, offsets = self.window_offsets(x.shape[1], num_frames, num_eval)
        frames_batch = torch.cat([x[:, o:o + num_frames] for o in offsets], dim=0)
        embeddings = self.inference(frames_batch)
        if return_mean:
            embeddings = self.ops.group_mean(embeddings.contiguous(), embeddings.shape[0])
        return embeddings
