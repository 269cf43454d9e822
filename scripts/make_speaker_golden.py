"""Regenerate tests/golden/speaker_lstm_tiny.npz from the reference's own class:

    python scripts/make_speaker_golden.py /path/to/reference/checkout

Imports ``speaker.models.lstm.LSTMSpeakerEncoder`` from the reference checkout (only here, at generation time), builds it at tiny
dimensions, loads seeded weights with NON-ZERO biases (workload.speaker), and records ``compute_embedding`` (ten windows of 40 frames out of 100: short, so that the emulator test stays quick) on a seeded mel input: the
state dict, the input, the reference's embedding and per-window embeddings in fp32, and the same from the same class in float64 --
the fixture's own fp32-against-fp64 gap is the ``a`` of the test's bound."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from workload import speaker as WS      # noqa: E402


def main(ref_root):
    sys.path.insert(0, ref_root)
    from speaker.models.lstm import LSTMSpeakerEncoder
    d = WS.TINY
    T, NF = 100, 40
    sd = WS.make_speaker_state(seed=31415, **d)
    model = LSTMSpeakerEncoder(d["input_dim"], d["proj_dim"], d["lstm_dim"], d["num_lstm_layers"])
    model.load_state_dict(sd)
    model.eval()
    mel = 2.0 * torch.randn(1, T, d["input_dim"], generator=torch.Generator().manual_seed(27))
    with torch.no_grad():
        w32 = model.compute_embedding(mel, num_frames=NF, return_mean=False)
        e32 = model.compute_embedding(mel, num_frames=NF)
        model.double()
        w64 = model.compute_embedding(mel.double(), num_frames=NF, return_mean=False)
        e64 = model.compute_embedding(mel.double(), num_frames=NF)
    out = {"sd/" + k: v.numpy() for k, v in sd.items()}
    out.update(dims=np.array([d["input_dim"], d["proj_dim"], d["lstm_dim"], d["num_lstm_layers"]], dtype=np.int32), num_frames=np.int32(NF), mel=mel.numpy(),
               windows32=w32.numpy(), embedding32=e32.numpy(), windows64=w64.numpy(), embedding64=e64.numpy())
    path = os.path.join(ROOT, "tests", "golden", "speaker_lstm_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; fp32 against fp64:", float((e32.double() - e64).abs().max()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SVCMI_REFERENCE", ""))
