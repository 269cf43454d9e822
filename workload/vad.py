"""Seeded Silero-VAD-shaped state dicts (the 16 kHz model's key names and shapes) for tests and timing scripts.

The real weights are a fixture (tests/golden/silero_vad.npz); these are for the checks that need weights of a chosen size: a wrong
shape for the loader, and small recurrent matrices under saturated gates for the scan kernel."""
import math

import torch

HIDDEN = 64
BLOCKS = (("first_layer.0", 258, 16), ("encoder.3.0", 16, 32), ("encoder.7.0", 32, 32), ("encoder.11.0", 32, 64))
DOWNS = (("encoder.0", "encoder.1", 16), ("encoder.4", "encoder.5", 32), ("encoder.8", "encoder.9", 32), ("encoder.12", "encoder.13", 64))


def make_vad_state(seed=1618, rnn_scale=None):
    """Every tensor of the 16 kHz model.  The STFT basis is the real construction (a Hann-windowed DFT of 256 taps: rows 0..128 cosine,
    129..257 sine), the smoothing filter a normalised 7-tap bell; convolutions are He-normal, BatchNorm statistics are away from the
    identity, LSTM weights are xavier-normal (times ``rnn_scale`` if given) with N(0, 0.5) biases."""
    g = torch.Generator().manual_seed(seed)

    def he(*shape, fan):
        return torch.randn(*shape, generator=g) * math.sqrt(2.0 / fan)

    sd = {}
    n = torch.arange(256, dtype=torch.float64)
    win = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / 256)
    k = torch.arange(129, dtype=torch.float64)[:, None]
    ang = 2.0 * math.pi * k * n[None, :] / 256
    sd["feature_extractor.forward_basis_buffer"] = torch.cat([torch.cos(ang) * win, -torch.sin(ang) * win]).float().unsqueeze(1)
    f = torch.tensor([1.0, 3.0, 6.0, 7.0, 6.0, 3.0, 1.0])
    sd["adaptive_normalization.filter_"] = (f / f.sum()).view(1, 1, 7)
    for name, cin, cout in BLOCKS:
        sd[f"{name}.dw_conv.0.weight"] = he(cin, 1, 5, fan=5)
        sd[f"{name}.dw_conv.0.bias"] = torch.randn(cin, generator=g) * 0.1
        sd[f"{name}.pw_conv.0.weight"] = he(cout, cin, 1, fan=cin)
        sd[f"{name}.pw_conv.0.bias"] = torch.randn(cout, generator=g) * 0.1
        if cin != cout:
            sd[f"{name}.proj.weight"] = he(cout, cin, 1, fan=cin)
            sd[f"{name}.proj.bias"] = torch.randn(cout, generator=g) * 0.1
    for conv, bn, c in DOWNS:
        sd[f"{conv}.weight"] = he(c, c, 1, fan=c)
        sd[f"{conv}.bias"] = torch.randn(c, generator=g) * 0.1
        sd[f"{bn}.weight"] = 1.0 + 0.2 * torch.randn(c, generator=g)
        sd[f"{bn}.bias"] = 0.1 * torch.randn(c, generator=g)
        sd[f"{bn}.running_mean"] = 0.2 * torch.randn(c, generator=g)
        sd[f"{bn}.running_var"] = 0.5 + torch.rand(c, generator=g)
        sd[f"{bn}.num_batches_tracked"] = torch.tensor(1000)
    s = 1.0 if rnn_scale is None else float(rnn_scale)
    for layer in (0, 1):
        sd[f"decoder.rnn.weight_ih_l{layer}"] = torch.randn(4 * HIDDEN, HIDDEN, generator=g) * math.sqrt(2.0 / (5 * HIDDEN)) * s
        sd[f"decoder.rnn.weight_hh_l{layer}"] = torch.randn(4 * HIDDEN, HIDDEN, generator=g) * math.sqrt(2.0 / (5 * HIDDEN)) * s
        sd[f"decoder.rnn.bias_ih_l{layer}"] = torch.randn(4 * HIDDEN, generator=g) * 0.5
        sd[f"decoder.rnn.bias_hh_l{layer}"] = torch.randn(4 * HIDDEN, generator=g) * 0.5
    sd["decoder.decoder.1.weight"] = torch.randn(1, HIDDEN, 1, generator=g) * 0.3
    sd["decoder.decoder.1.bias"] = torch.randn(1, generator=g) * 0.1
    return sd
