"""Seeded ``LSTMSpeakerEncoder`` state dicts (speaker/models/lstm.py key names) for tests and timing scripts.

Weights are xavier-normal like the reference's ``_init_layers``; biases are N(0, 0.5) instead of the reference's zeros, so that a
missing ``b_hh`` (or a bias applied to the wrong gate) changes the result."""
import math

import torch

TINY = dict(input_dim=12, proj_dim=20, lstm_dim=40, num_lstm_layers=3)
FULL = dict(input_dim=80, proj_dim=256, lstm_dim=768, num_lstm_layers=3)      # speaker_pretrain/config.json "model"


def make_speaker_state(input_dim=80, proj_dim=256, lstm_dim=768, num_lstm_layers=3, seed=2718):
    g = torch.Generator().manual_seed(seed)

    def xavier(rows, cols):
        return torch.randn(rows, cols, generator=g) * math.sqrt(2.0 / (rows + cols))

    sd = {}
    for i in range(num_lstm_layers):
        d_in = input_dim if i == 0 else proj_dim
        sd[f"layers.{i}.lstm.weight_ih_l0"] = xavier(4 * lstm_dim, d_in)
        sd[f"layers.{i}.lstm.weight_hh_l0"] = xavier(4 * lstm_dim, lstm_dim)
        sd[f"layers.{i}.lstm.bias_ih_l0"] = torch.randn(4 * lstm_dim, generator=g) * 0.5
        sd[f"layers.{i}.lstm.bias_hh_l0"] = torch.randn(4 * lstm_dim, generator=g) * 0.5
        sd[f"layers.{i}.linear.weight"] = xavier(proj_dim, lstm_dim)
    return sd
