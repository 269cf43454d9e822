"""Checks of the speaker encoder (csrc/lstm.hip, svcmi_speaker_encoder_fwd, svcmi.speaker), shared by the emulator tests (CPU) and the
GPU tests like tests/kernel_cases.py: every function takes ``ops`` and ``device``.

Reference for every numeric check: the operation's plain formula in float64 on the same fp32 inputs (``want64``), under the project's
Rule A (tests/kernel_cases.py ``_close64``): |got - want64| <= 8 (2^-24 |want64| + a) per element, where ``a`` is the error against
``want64`` of torch's own CPU fp32 ``nn.LSTM`` / ``nn.Linear`` (or, for the mel path, of an fp32 numpy restatement built on
``np.fft.rfft``) on the same inputs -- computed here, never from the code under test."""
import functools
import json
import math
import os

import numpy as np
import torch

from tests.kernel_cases import _close64
from workload import speaker as WS

STEP_H = (4, 20, 40)
STEP_B = (1, 3, 16, 17)
STEP_T = (1, 2, 7)
POISON = 1234.5


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ references
def lstm_layer64(gx, w_hh):
    """The recurrence in float64, written out: gx [B, T, 4H] (gate-major i | f | g | o, biases included), w_hh [4H, H] ->
    (h sequence [B, T, H], every step's cell state [B, T, H])."""
    gx, w_hh = gx.double(), w_hh.double()
    B, T, H4 = gx.shape
    H = H4 // 4
    h, c = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
    hs, cs = [], []
    for t in range(T):
        pre = gx[:, t] + h @ w_hh.t()
        i, f, g, o = (pre[:, k * H:(k + 1) * H] for k in range(4))
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
        cs.append(c)
    return torch.stack(hs, 1), torch.stack(cs, 1)


def lstm_layer32(gx, w_hh):
    """torch's own CPU fp32 ``nn.LSTM`` on the same pre-activations: input size 4H with W_ih = I and zero biases, so that its input
    projection reproduces ``gx`` exactly (x * 1 plus exact zeros)."""
    B, T, H4 = gx.shape
    H = H4 // 4
    m = torch.nn.LSTM(H4, H, batch_first=True)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.eye(H4))
        m.weight_hh_l0.copy_(w_hh)
        m.bias_ih_l0.zero_()
        m.bias_hh_l0.zero_()
        out, (_, c) = m(gx)
    return out, c[0]


def torch_encoder(sd, dtype):
    """The reference architecture from torch's own modules: [(nn.LSTM, nn.Linear)] per layer."""
    layers, i = [], 0
    while f"layers.{i}.lstm.weight_ih_l0" in sd:
        w_ih, w_hh = sd[f"layers.{i}.lstm.weight_ih_l0"], sd[f"layers.{i}.lstm.weight_hh_l0"]
        lstm = torch.nn.LSTM(w_ih.shape[1], w_hh.shape[1], batch_first=True)
        lin = torch.nn.Linear(w_hh.shape[1], sd[f"layers.{i}.linear.weight"].shape[0], bias=False)
        with torch.no_grad():
            lstm.weight_ih_l0.copy_(w_ih)
            lstm.weight_hh_l0.copy_(w_hh)
            lstm.bias_ih_l0.copy_(sd[f"layers.{i}.lstm.bias_ih_l0"])
            lstm.bias_hh_l0.copy_(sd[f"layers.{i}.lstm.bias_hh_l0"])
            lin.weight.copy_(sd[f"layers.{i}.linear.weight"])
        layers.append((lstm.to(dtype), lin.to(dtype)))
        i += 1
    return layers


@torch.no_grad()
def encoder_ref(sd, x, dtype):
    """LSTMSpeakerEncoder.inference with torch's modules in ``dtype``: x [B, T, D] -> normalised [B, P]."""
    d = x.to(dtype)
    for lstm, lin in torch_encoder(sd, dtype):
        d = lin(lstm(d)[0])
    return torch.nn.functional.normalize(d[:, -1], p=2, dim=1)


@torch.no_grad()
def encoder_formula64(sd, x):
    """The same in float64 from the written-out recurrence (pins ``encoder_ref`` to the plain formula: tests/test_speaker_abi.py)."""
    d, i = x.double(), 0
    while f"layers.{i}.lstm.weight_ih_l0" in sd:
        p = f"layers.{i}"
        gx = d @ sd[p + ".lstm.weight_ih_l0"].double().t() + sd[p + ".lstm.bias_ih_l0"].double() + sd[p + ".lstm.bias_hh_l0"].double()
        d = lstm_layer64(gx, sd[p + ".lstm.weight_hh_l0"])[0] @ sd[p + ".linear.weight"].double().t()
        i += 1
    v = d[:, -1]
    return v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)


# ------------------------------------------------------------------------------------------------ step kernel
def run_steps(ops, device, gx, w_hh, margin=True, want_c_steps=False):
    """T launches of the step kernel on padded, poisoned buffers.  gx [B, T, 4H] / w_hh [4H, H] in torch's gate-major order (permuted
    here as svcmi.weights does).  Returns (hseq [B, T, H], c [B, H], (c after every step)) on the CPU; asserts the margins untouched."""
    from svcmi import weights as PW
    B, T, H4 = gx.shape
    H = H4 // 4
    perm = PW.lstm_tile_order(H)
    gxp = gx[:, :, perm].contiguous().to(device)
    whh = w_hh[perm].contiguous().to(device)
    rb, rc = (2, 4) if margin else (0, 0)
    hbuf = torch.full((B + rb, T, H + rc), POISON, dtype=torch.float32, device=device)
    cbuf = torch.full((B + rb, H + rc), POISON, dtype=torch.float32, device=device)
    hseq, c = hbuf[:B, :, :H], cbuf[:B, :H]
    steps = []
    for t in range(T):
        ops.lstm_step(gxp, whh, hseq, c, t)
        if want_c_steps:
            steps.append(c.cpu().clone())
    hb, cb = hbuf.cpu(), cbuf.cpu()
    assert bool((hb[B:] == POISON).all()) and bool((hb[:, :, H:] == POISON).all()), "rows >= B or columns >= H of the sequence buffer were written"
    assert bool((cb[B:] == POISON).all()) and bool((cb[:, H:] == POISON).all()), "rows >= B or columns >= H of the cell buffer were written"
    return hb[:B, :, :H].contiguous(), cb[:B, :H].contiguous(), steps


def step_inputs(B, T, H, seed):
    g = _g(seed)
    gx = 2.0 * torch.randn(B, T, 4 * H, generator=g)
    w_hh = torch.randn(4 * H, H, generator=g) * math.sqrt(2.0 / (5 * H))
    return gx, w_hh


def check_step_shape(ops, device, B, T, H, seed=0):
    gx, w_hh = step_inputs(B, T, H, seed + 1000 * H + 10 * B + T)
    h, c, _ = run_steps(ops, device, gx, w_hh)
    h64, c64 = lstm_layer64(gx, w_hh)
    h32, c32 = lstm_layer32(gx, w_hh)
    _close64(h, h64, h32, f"lstm step h  B={B} T={T} H={H}")
    _close64(c, c64[:, -1], c32, f"lstm step c  B={B} T={T} H={H}")


def check_step_shapes(ops, device, H):
    for B in STEP_B:
        for T in STEP_T:
            check_step_shape(ops, device, B, T, H)


def check_saturation(ops, device):
    """Pre-activations of +-30 and +-100 (W_hh = 0, so the gate inputs are exactly the values in gx, where the biases live): sigmoid
    and tanh give what float64 rounds to -- exactly 0 / 1 at +-100, exactly 1 at +30, exactly +-1 for tanh at +-30 and +-100 -- and
    nothing is NaN or inf."""
    H, T = 4, 1
    vals = [30.0, -30.0, 100.0, -100.0]
    w_hh = torch.zeros(4 * H, H)
    sig = lambda v: 1.0 if v >= 30.0 else (0.0 if v <= -100.0 else None)       # (sigmoid(-30) = 9.4e-14: small, not zero)
    for i in vals:                                                             # 4 calls of 64 rows: every combination of the four gates
        rows = [(i, f, g, o) for f in vals for g in vals for o in vals]
        B = len(rows)
        gx = torch.zeros(B, T, 4 * H)
        for b, r in enumerate(rows):
            for q in range(4):
                gx[b, 0, q * H:(q + 1) * H] = r[q]
        h, c, _ = run_steps(ops, device, gx, w_hh)
        assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(c).all())
        for b, (_, f, g, o) in enumerate(rows):
            si, so, tg = sig(i), sig(o), math.copysign(1.0, g)
            if si is not None:
                assert bool((c[b] == si * tg).all()), (b, rows[b], c[b])          # c = sigmoid(i) tanh(g): exactly +-1 or 0
                if so is not None:
                    want = so * math.tanh(si * tg)                                 # h = sigmoid(o) tanh(c): 0, or tanh(+-1) to fp32 rounding
                    assert bool(((h[b].double() - want).abs() <= 2.0 ** -23 * abs(want)).all()), (b, rows[b], h[b])
        h64, c64 = lstm_layer64(gx, w_hh)
        h32, c32 = lstm_layer32(gx, w_hh)
        _close64(h, h64, h32, f"lstm saturation h, i = {i}")
        _close64(c, c64[:, -1], c32, f"lstm saturation c, i = {i}")
    # two steps with a saturated cell: tanh(c) is exactly +-1
    gx2 = torch.zeros(2, 12, 4 * H)
    gx2[:, :, 0 * H:1 * H], gx2[:, :, 1 * H:2 * H], gx2[:, :, 3 * H:] = 100.0, 100.0, 100.0
    gx2[0, :, 2 * H:3 * H], gx2[1, :, 2 * H:3 * H] = 100.0, -100.0
    h2, c2, _ = run_steps(ops, device, gx2, w_hh)
    assert bool((c2[0] == 12.0).all()) and bool((c2[1] == -12.0).all())
    assert bool((h2[0, -1] == 1.0).all()) and bool((h2[1, -1] == -1.0).all())


def check_exact_cell_growth(ops, device, T=40):
    """Forget gate exactly 1 and i * g exactly 1 at every step: c after t steps is exactly t, and h = sigmoid(o) * tanh(t)."""
    H, B = 20, 3
    g = _g(5)
    gx = torch.zeros(B, T, 4 * H)
    gx[:, :, :3 * H] = 100.0
    gx[:, :, 3 * H:] = torch.randn(B, T, H, generator=g)
    w_hh = torch.randn(4 * H, H, generator=g) * 0.05                 # |h W| < 1: the saturated gates stay saturated
    h, c, steps = run_steps(ops, device, gx, w_hh, want_c_steps=True)
    for t, ct in enumerate(steps):
        assert bool((ct == float(t + 1)).all()), (t, ct)
    h64, _ = lstm_layer64(gx, w_hh)
    h32, _ = lstm_layer32(gx, w_hh)
    _close64(h, h64, h32, "lstm exact cell growth h")


def check_batch_independence(ops, device):
    """Row b of a B = 10 run is bit-equal to its solo run, and to the same row inside a B = 17 run (second M tile present); a repeated
    run gives identical bits."""
    H, T = 40, 7
    gx, w_hh = step_inputs(10, T, H, seed=77)
    h, c, _ = run_steps(ops, device, gx, w_hh)
    h_again, c_again, _ = run_steps(ops, device, gx, w_hh)
    assert torch.equal(h, h_again) and torch.equal(c, c_again)
    for b in (0, 4, 9):
        hb, cb, _ = run_steps(ops, device, gx[b:b + 1], w_hh)
        assert torch.equal(hb[0], h[b]) and torch.equal(cb[0], c[b]), b
    gx17 = torch.cat([gx, step_inputs(7, T, H, seed=78)[0]], 0)
    h17, c17, _ = run_steps(ops, device, gx17, w_hh)
    assert torch.equal(h17[:10], h) and torch.equal(c17[:10], c)


# ------------------------------------------------------------------------------------------------ encoder
def make_encoder(ops, device, dims, seed=2718):
    from svcmi.speaker.models.lstm import LSTMSpeakerEncoder
    sd = WS.make_speaker_state(seed=seed, **dims)
    enc = LSTMSpeakerEncoder(dims["input_dim"], dims["proj_dim"], dims["lstm_dim"], dims["num_lstm_layers"], device=device, ops=ops)
    enc.load_checkpoint({"model": sd})
    return enc, sd


def check_encoder(ops, device, dims, B, T, seed=3):
    enc, sd = make_encoder(ops, device, dims)
    x = 2.0 * torch.randn(B, T, dims["input_dim"], generator=_g(seed))
    got = enc.inference(x.to(device))
    assert tuple(got.shape) == (B, dims["proj_dim"])
    return _close64(got, encoder_ref(sd, x, torch.float64), encoder_ref(sd, x, torch.float32), f"speaker encoder {dims['lstm_dim']} B={B} T={T}")


def embedding64(sd, x, num_frames, num_eval, dtype=torch.float64):
    """compute_embedding restated: the reference's np.linspace offsets; a clip shorter than num_frames is taken whole, num_eval times."""
    max_len = x.shape[1]
    nf = min(num_frames, max_len)
    offsets = [int(o) for o in np.linspace(0, max_len - nf, num=num_eval)]
    e = encoder_ref(sd, torch.cat([x[:, o:o + nf] for o in offsets], 0), dtype)
    return e, e.mean(dim=0, keepdim=True)


def check_compute_embedding(ops, device):
    dims = WS.TINY
    enc, sd = make_encoder(ops, device, dims)
    for (T, nf) in ((61, 25), (9, 25)):          # offsets 0, 4, 8, ..., 36; and the short clip: ten copies of the whole of it
        x = 2.0 * torch.randn(1, T, dims["input_dim"], generator=_g(T))
        per64, mean64 = embedding64(sd, x, nf, 10)
        per32, mean32 = embedding64(sd, x, nf, 10, torch.float32)
        got_per = enc.compute_embedding(x.to(device), num_frames=nf, num_eval=10, return_mean=False)
        got = enc.compute_embedding(x.to(device), num_frames=nf, num_eval=10)
        assert tuple(got_per.shape) == (10, dims["proj_dim"]) and tuple(got.shape) == (1, dims["proj_dim"])
        _close64(got_per, per64, per32, f"compute_embedding windows T={T}")
        _close64(got, mean64, mean32, f"compute_embedding mean T={T}")
        if T < nf:
            assert all(torch.equal(got_per[0], got_per[i]) for i in range(10))
    assert enc.window_offsets(300)[1] == [int(o) for o in np.linspace(0, 50, num=10)]
    assert enc.window_offsets(100) == (100, [0] * 10)


def check_golden(ops, device, golden_dir, tmp_path):
    """The fixture made by the reference's own class (scripts/make_speaker_golden.py), loaded through load_checkpoint's file and key
    path; a = the fixture's own fp32 against fp64 gap."""
    from svcmi.speaker.models.lstm import LSTMSpeakerEncoder
    z = np.load(os.path.join(golden_dir, "speaker_lstm_tiny.npz"))
    sd = {k[len("sd/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    path = os.path.join(str(tmp_path), "speaker_tiny.pth.tar")
    torch.save({"model": sd}, path)
    d = {k: int(z["dims"][i]) for i, k in enumerate(("input_dim", "proj_dim", "lstm_dim", "num_lstm_layers"))}
    enc = LSTMSpeakerEncoder(d["input_dim"], d["proj_dim"], d["lstm_dim"], d["num_lstm_layers"], device=device, ops=ops)
    enc.load_checkpoint(path, eval=True, use_cuda=True)
    mel = torch.from_numpy(z["mel"]).to(device)
    nf = int(z["num_frames"])
    _close64(enc.compute_embedding(mel, num_frames=nf, return_mean=False), torch.from_numpy(z["windows64"]), torch.from_numpy(z["windows32"]),
             "golden windows")
    _close64(enc.compute_embedding(mel, num_frames=nf), torch.from_numpy(z["embedding64"]), torch.from_numpy(z["embedding32"]), "golden embedding")


# ------------------------------------------------------------------------------------------------ front-end
AUDIO_CFG = dict(num_mels=80, fft_size=1024, sample_rate=16000, win_length=1024, hop_length=256, frame_length_ms=None, frame_shift_ms=None,
                 preemphasis=0.98, min_level_db=-100, ref_level_db=20, power=1.5, griffin_lim_iters=60, signal_norm=True,
                 symmetric_norm=True, max_norm=4.0, clip_norm=True, mel_fmin=0.0, mel_fmax=8000.0, do_trim_silence=True, trim_db=60)


def make_ap(ops, device, **over):
    from svcmi.speaker.utils.audio import AudioProcessor
    return AudioProcessor(**dict(AUDIO_CFG, ops=ops, device=device, **over))


@functools.lru_cache(maxsize=None)
def _mel_basis64():
    from svcmi.whisper.audio import slaney_mel_filterbank
    return slaney_mel_filterbank(16000, 1024, 80).astype(np.float64)          # the fp32 filterbank the kernels read, widened


def mel_restated(y, dtype):
    """AudioProcessor.melspectrogram (speaker/utils/audio.py:354-391, 480-489, 561-571) in numpy on np.fft.rfft, every step in ``dtype``:
    pre-emphasis, reflect pad by 512, frames of 1024 every 256, periodic Hann, |rfft|, mel projection, 20 log10(max(1e-5, .)), - 20,
    (S + 100) / 100, * 8 - 4, clip to +-4.  Returns [frames, 80]."""
    y = np.asarray(y, dtype=np.float32).astype(dtype)
    p = np.empty_like(y)
    p[0] = y[0]
    p[1:] = y[1:] - dtype(0.98) * y[:-1]
    if p.shape[0] <= 512:
        raise ValueError("reflect pad of 512 needs more than 512 samples")
    p = np.pad(p, 512, mode="reflect")
    frames = 1 + (p.shape[0] - 1024) // 256
    k = np.arange(1024, dtype=np.float64)
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * k / 1024)).astype(dtype)
    fr = np.stack([p[i * 256:i * 256 + 1024] for i in range(frames)]) * win
    mag = np.abs(np.fft.rfft(fr, axis=1)).astype(dtype)
    mel = mag @ _mel_basis64().astype(dtype).T
    s = dtype(20.0) * np.log10(np.maximum(dtype(1e-5), mel)) - dtype(20.0)
    s = (s + dtype(100.0)) / dtype(100.0)
    s = dtype(8.0) * s - dtype(4.0)
    return np.clip(s, dtype(-4.0), dtype(4.0)).astype(dtype)


def tone_noise(n, seed=1, amp=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (amp * np.sin(2 * np.pi * 440.0 * t) + 0.1 * amp * np.sin(2 * np.pi * 3100.0 * t + 0.5) + 0.05 * rng.standard_normal(n)).astype(np.float32)


def check_mel(ops, device, n):
    ap = make_ap(ops, device)
    y = tone_noise(n, seed=n)
    got = ap.melspectrogram_device(y)
    want64, ref32 = mel_restated(y, np.float64), mel_restated(y, np.float32)
    assert tuple(got.shape) == want64.shape == (1 + n // 256, 80)
    r = _close64(got, torch.from_numpy(want64), torch.from_numpy(ref32), f"speaker mel n={n}")
    m = ap.melspectrogram(y)
    assert m.dtype == np.float32 and m.shape == (80, 1 + n // 256) and np.array_equal(m.T, got.cpu().numpy())
    return r


def check_mel_edges(ops, device):
    import pytest
    ap = make_ap(ops, device)
    for n in (512, 100):
        with pytest.raises(ValueError):
            ap.melspectrogram_device(np.zeros(n, dtype=np.float32))
    z = ap.melspectrogram_device(np.zeros(1024, dtype=np.float32)).cpu()
    assert tuple(z.shape) == (5, 80) and bool((z == -4.0).all())
    # The upper clip.  With |x| <= 1 no mel band can reach it (a band is below sqrt(sum w^2) * sqrt(frame energy) ~ 10.6 by
    # Cauchy-Schwarz, and +4 starts at 10): the full scale that does is the int16 one, an un-normalised PCM clip -- every band of it
    # sits on the clip.  At 60x the unit scale the tones clip and the noise bands do not: the kink is checked against float64 there.
    loud = np.clip(np.round(32767.0 * tone_noise(4000, seed=6, amp=0.9)), -32767.0, 32767.0).astype(np.float32)
    assert bool((ap.melspectrogram_device(loud) == 4.0).all()) and bool((mel_restated(loud, np.float64) == 4.0).all())
    mid = (60.0 * tone_noise(4000, seed=6, amp=0.9)).astype(np.float32)
    got = ap.melspectrogram_device(mid)
    want64, ref32 = mel_restated(mid, np.float64), mel_restated(mid, np.float32)
    on_clip = float((want64 == 4.0).mean())
    assert 0.02 < on_clip < 0.9 and float(got.max()) == 4.0 and float(got.min()) >= -4.0, on_clip
    _close64(got, torch.from_numpy(want64), torch.from_numpy(ref32), "speaker mel across the upper clip")


def check_preemphasis(ops, device):
    """y[0] = x[0] exactly, y[n] = x[n] - 0.98 x[n - 1], reflect padding without an edge repeat; two rows, an odd length."""
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, (2, 777)).astype(np.float32)
    pad = 512
    got = ops.preemph_pad(torch.from_numpy(x).to(device), pad, 0.98).cpu()
    assert tuple(got.shape) == (2, 777 + 2 * pad)
    assert bool((got[:, pad] == torch.from_numpy(x[:, 0])).all())

    def ref(dtype):
        xx = x.astype(dtype)
        p = np.concatenate([xx[:, :1], xx[:, 1:] - dtype(np.float32(0.98)) * xx[:, :-1]], axis=1)
        return np.pad(p, ((0, 0), (pad, pad)), mode="reflect")
    _close64(got, torch.from_numpy(ref(np.float64)), torch.from_numpy(ref(np.float32)), "preemph + reflect pad")


def check_trim_and_norm(ops, device):
    """silence | tone | silence.  After the 160-sample margins the clip is 16384 samples with the tone on [4096, 12288).  Frames of
    1024 are centred on multiples of 256: frame k covers [256 k - 512, 256 k + 512).  Frame 14 ends at 4096 (no tone), frame 15 holds
    256 tone samples (-6 dB of a full frame: far above -60 dB); frame 49 starts at 12032 (256 tone samples), frame 50 at 12288 (none).
    So the sound frames are 15 .. 49 and the cut is [15 * 256, 50 * 256) = [3840, 12800)."""
    ap = make_ap(ops, device)
    t = np.arange(8192) / 16000.0
    tone = (0.5 * np.cos(2 * np.pi * 440.0 * t)).astype(np.float32)
    core = np.concatenate([np.zeros(4096, np.float32), tone, np.zeros(4096, np.float32)])
    wav = np.concatenate([np.full(160, 0.25, np.float32), core, np.full(160, 0.25, np.float32)])       # the margins are dropped, loud or not
    assert ap.trim_bounds(core) == (3840, 12800)
    out = ap.trim_silence(wav)
    assert np.array_equal(out, core[3840:12800])
    assert ap.trim_bounds(np.zeros(5000, np.float32)) == (0, 5000)            # all frames equal the maximum: nothing is below it
    x = tone_noise(3000, seed=4)
    assert np.array_equal(ap.sound_norm(x), x / np.float32(np.abs(x).max()) * np.float32(0.95))
    assert ap.sound_norm(x).dtype == np.float32


# ------------------------------------------------------------------------------------------------ end to end
CONFIG_TEXT = """{
    "model_name": "lstm",   // a commented JSON file like speaker_pretrain/config.json
    "audio":{
        // Audio processing parameters
        "num_mels": %(input_dim)d,         // size of the mel spec frame.
        "fft_size": 1024, "sample_rate": 16000, "win_length": 1024, "hop_length": 256,
        "frame_length_ms": null,  // stft window length in ms.If null, 'win_length' is used.
        "frame_shift_ms": null,
        "preemphasis": 0.98, "min_level_db": -100, "ref_level_db": 20, "power": 1.5, "griffin_lim_iters": 60,
        "signal_norm": true, "symmetric_norm": true, "max_norm": 4.0, "clip_norm": true,
        "mel_fmin": 0.0, "mel_fmax": 8000.0,
        "do_trim_silence": true,  // enable trimming of slience of audio as you load it.
        "trim_db": 60          // threshold for timming silence.
    },
    "model": {
        "input_dim": %(input_dim)d, "proj_dim": %(proj_dim)d, "lstm_dim": %(lstm_dim)d, "num_lstm_layers": %(num_lstm_layers)d,
        "use_lstm_with_projection": %(proj)s
    }
}
"""
E2E_DIMS = dict(input_dim=80, proj_dim=20, lstm_dim=40, num_lstm_layers=3)       # the tiny model on the real 80-band front-end


def write_model(tmp_path, dims=E2E_DIMS, projection=True, seed=2718):
    sd = WS.make_speaker_state(seed=seed, **dims)
    model, config = os.path.join(str(tmp_path), "speaker.pth.tar"), os.path.join(str(tmp_path), "config.json")
    torch.save({"model": sd}, model)
    with open(config, "w", encoding="utf-8") as f:
        f.write(CONFIG_TEXT % dict(dims, proj="true" if projection else "false"))
    return sd, model, config


def voice_clip(seconds, seed):
    """int16 PCM at 16 kHz: quiet lead-in and tail around a vibrato tone with harmonics and noise."""
    rng = np.random.default_rng(seed)
    n = int(seconds * 16000)
    t = np.arange(n) / 16000.0
    f0 = 180.0 + 25.0 * seed
    v = sum(a * np.sin(2 * np.pi * k * (f0 + 4.0 * np.sin(2 * np.pi * 5.0 * t)) * t) for k, a in ((1, 0.3), (2, 0.15), (3, 0.08), (7, 0.03)))
    env = np.zeros(n)
    env[n // 8: n - n // 8] = 1.0
    x = v * env + 0.004 * rng.standard_normal(n)
    return np.round(x * 32767).astype(np.int16)


def chain_restated(sd, pcm, dtype):
    """wav -> embedding, restated: decode (/ 2^15), drop the 10 ms margins, trim (the frame arithmetic of librosa.effects.trim, float64
    RMS), level to 0.95 in fp32 (the reference's numpy expression), mel in ``dtype``, the ten-window embedding with torch in ``dtype``."""
    x = pcm.astype(np.float32) / np.float32(32768.0)
    x = x[160:-160]
    y = np.pad(x.astype(np.float64), 512)
    frames = 1 + (y.shape[0] - 1024) // 256
    power = np.array([np.mean(y[i * 256:i * 256 + 1024] ** 2) for i in range(frames)])
    db = 10.0 * np.log10(np.maximum(1e-10, power)) - 10.0 * np.log10(max(1e-10, power.max()))
    nz = np.flatnonzero(db > -60.0)
    x = x[nz[0] * 256:min(x.shape[0], (nz[-1] + 1) * 256)]
    x = x / np.float32(np.abs(x).max()) * np.float32(0.95)
    mel = mel_restated(x, np.float64 if dtype == torch.float64 else np.float32)
    return embedding64(sd, torch.from_numpy(mel)[None], 250, 10, dtype)[1][0]


def run_cli(args, cwd):
    """python -m svcmi.speaker.infer in a fresh child process."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "whisper-vits-svc_amd"), root] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    return subprocess.run([sys.executable, "-m", "svcmi.speaker.infer"] + list(args), cwd=str(cwd), env=env, capture_output=True, text=True, timeout=300)
