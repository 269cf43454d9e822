"""Checks of the training-set preparation recipes shared by the CPU (emulator) and the GPU tests: every function takes ``ops`` and
``device`` like tests/spectrogram_cases.py."""
import numpy as np
import torch

from tests import engine_cases as E
from workload import weights as W

F0_N = 16000 + 37              # 1 s + 37 samples at 16 kHz -> 101 frames at hop 160
BIAS_SHIFT = 1.85             # see crepe_state_with_gate: 94 of the 101 filtered periodicities fall below 0.5, 7 above, the nearest 9e-3 away


def preprocess_a_numpy(wav):
    """prepare/preprocess_a.py:12-14 on the loaded float32 waveform, verbatim -> int16."""
    wav = wav / np.abs(wav).max() * 0.6
    wav = wav / max(0.01, np.max(np.abs(wav))) * 32767 * 0.6
    return wav.astype(np.int16)


def crepe_state_with_gate():
    """The seeded tiny CREPE with ``classifier.bias`` lowered by a constant: as seeded, every periodicity lies in 0.75 .. 0.94 and the
    gate ``periodicity < 0.5`` never fires; shifted by 1.85 in the logit they spread over both sides of 0.5."""
    sd = dict(W.make_crepe_state("tiny"))
    sd["classifier.bias"] = sd["classifier.bias"] - BIAS_SHIFT
    return sd


def f0_oracle(sd, audio, noise, dither):
    """oracle/crepe_oracle.py's preprocess / network / decode composed at hop 160 like crepe.predict(..., return_periodicity=True):
    (bins int64 [F], periodicity float32 [F], Hz float32 [F]), decoding restarted every 512 frames."""
    from oracle import crepe_oracle as CO
    with torch.no_grad():
        prob = CO.network(sd, CO.preprocess((audio + noise * 0.001)[None], 160))
        bins, hz = [], []
        for i in range(0, prob.shape[0], 512):
            p = prob[i:i + 512]
            flat = CO.decode(p, 50.0, 1000.0, "viterbi", np.zeros(p.shape[0]))                  # no dither: Hz <-> bin is exact to invert
            b = torch.round((1200.0 * torch.log2(flat.double() / 10.0) - 1997.3794084376191) / 20.0).long()
            assert float((10 * 2 ** ((20.0 * b + 1997.3794084376191) / 1200) - flat).abs().max()) < 1e-2       # a bin apart is >= 0.5 Hz
            bins.append(b)
            hz.append(CO.decode(p, 50.0, 1000.0, "viterbi", dither[i:i + 512]))
        bins = torch.cat(bins)
        per = prob.gather(1, bins[:, None])[:, 0]
    return bins.numpy(), per.numpy(), torch.cat(hz).float().numpy()


def check_f0_train(ops, device):
    """compute_f0_train end to end against the oracle: bins equal, periodicity within 1e-5, the final track equal (NaN positions
    included).  First, on the oracle alone: both sides of the 0.5 gate occur and no median-filtered periodicity lies within 1e-3 of
    it -- so a 1e-5 difference cannot move a frame across the gate and no frame needs to be excused."""
    from svcmi.pitch import load_crepe
    from svcmi.pitch.inference import _median_filter_np, compute_f0_train_begin, f0_train_postfilter
    sd = crepe_state_with_gate()
    audio = E.crepe_test_audio(F0_N, 5)
    g = torch.Generator().manual_seed(9)
    noise = torch.randn(F0_N, generator=g)
    frames = 1 + F0_N // 160
    dither = (torch.rand(frames, generator=g) * 2 - 1).numpy() * 20.0
    bins_ref, per_ref, hz_ref = f0_oracle(sd, audio, noise, dither)
    med = _median_filter_np(per_ref, 7)
    assert (med < 0.5).any() and (med >= 0.5).any(), (float(med.min()), float(med.max()))
    assert float(np.abs(med - 0.5).min()) > 1e-3, float(np.abs(med - 0.5).min())
    want = f0_train_postfilter(hz_ref, per_ref)
    assert (want == 0).any() and (want > 0).any()

    m = load_crepe(sd, device, ops=ops)
    f0, bins, per = compute_f0_train_begin(audio, device, model=m, noise=noise)(dither, parts=True)
    assert f0.dtype == np.float32 and f0.shape == (frames,)
    assert np.array_equal(bins, bins_ref)
    assert float(np.abs(per - per_ref).max()) <= 1e-5, float(np.abs(per - per_ref).max())
    assert np.array_equal(np.isnan(f0), np.isnan(want)) and np.array_equal(f0[np.isfinite(f0)], want[np.isfinite(want)])
    return float(np.abs(per - per_ref).max())
