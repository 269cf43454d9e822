"""Checks of the voice-activity detector (csrc/vad.hip, svcmi_vad_probs_fwd, svcmi.vad, svcmi.svc_inference_post), shared by the emulator
tests (CPU) and the GPU tests: every function takes ``ops`` and ``device``.

The reference of every numeric check is ``VadRef``: the network restated in float64 from the state dict (the issue's description of
the scripted 16 kHz model, checked against the model itself when the fixture was made).  The fixture tests/golden/silero_vad.npz
(scripts/make_vad_golden.py) carries the real weights, the scripted model's fp32 probabilities and spans on two clips, ``ref_dev`` = the
largest deviation of those fp32 probabilities from this restatement, and the state-machine cases.

Bounds.  Probabilities: 8 x ref_dev of the clip, read from the fixture (the allowance for another summation order in the 256-tap and
258-channel sums and for the device's expf / tanhf / logf against torch's).  Front-end vectors and gate rows: Rule A of
tests/kernel_cases.py (``_close64``) with ``a`` = the error of torch's own CPU fp32 evaluation of the same restatement."""
import functools
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.kernel_cases import _close64
from workload import vad as WV

WIN = 512
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLIPS = {"035": "035.wav", "010": "vad_010.wav"}


# ------------------------------------------------------------------------------------------------ the restatement
class VadRef:
    """The 16 kHz network from its state dict in ``dtype`` (float64: the reference; float32: torch's own CPU arithmetic, the ``a`` of
    Rule A)."""

    def __init__(self, sd, dtype=torch.float64):
        self.sd = {k: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))) for k, v in sd.items()}
        self.dtype = dtype

    def p(self, name):
        return self.sd[name].to(self.dtype)

    def windows(self, x):
        """[n] -> [W, 512], the last window zero-padded on the right."""
        x = torch.as_tensor(x).to(self.dtype).reshape(-1)
        W = -(-x.shape[0] // WIN)
        return F.pad(x, (0, W * WIN - x.shape[0])).reshape(W, WIN)

    def conv_block(self, x, name):
        cin = x.shape[1]
        d = F.relu(F.conv1d(x, self.p(f"{name}.dw_conv.0.weight"), self.p(f"{name}.dw_conv.0.bias"), padding=2, groups=cin))
        y = F.conv1d(d, self.p(f"{name}.pw_conv.0.weight"), self.p(f"{name}.pw_conv.0.bias"))
        res = F.conv1d(x, self.p(f"{name}.proj.weight"), self.p(f"{name}.proj.bias")) if f"{name}.proj.weight" in self.sd else x
        return F.relu(y + res)

    def down(self, x, conv, bn, stride):
        y = F.conv1d(x, self.p(f"{conv}.weight"), self.p(f"{conv}.bias"), stride=stride)
        mean, var = self.p(f"{bn}.running_mean")[None, :, None], self.p(f"{bn}.running_var")[None, :, None]
        y = (y - mean) / torch.sqrt(var + 1e-5) * self.p(f"{bn}.weight")[None, :, None] + self.p(f"{bn}.bias")[None, :, None]
        return F.relu(y)

    @torch.no_grad()
    def frontend(self, x):
        """[n] -> (the 64-vector of every window [W, 64], the layer-0 gate rows [W, 256])."""
        w = self.windows(x)
        xp = F.pad(w[:, None], (96, 96), mode="reflect")
        st = F.conv1d(xp, self.p("feature_extractor.forward_basis_buffer"), stride=64)          # [W, 258, 8]
        mag = torch.sqrt(st[:, :129] ** 2 + st[:, 129:] ** 2)
        s = torch.log1p(mag * 2.0 ** 20)
        m = s.mean(dim=1)                                                                        # [W, 8]
        ext = torch.cat([m[:, [3, 2, 1]], m, m[:, [6, 5, 4]]], dim=1)
        mu = F.conv1d(ext[:, None], self.p("adaptive_normalization.filter_")).mean(dim=-1)      # [W, 1]
        h = torch.cat([mag, s - mu[:, :, None]], dim=1)
        h = self.conv_block(h, "first_layer.0")
        h = self.down(h, "encoder.0", "encoder.1", 2)
        h = self.conv_block(h, "encoder.3.0")
        h = self.down(h, "encoder.4", "encoder.5", 2)
        h = self.conv_block(h, "encoder.7.0")
        h = self.down(h, "encoder.8", "encoder.9", 2)
        h = self.conv_block(h, "encoder.11.0")
        h = self.down(h, "encoder.12", "encoder.13", 1)
        feat = h[:, :, 0]
        return feat, self.gates0(feat)

    def gates0(self, feat):
        r = "decoder.rnn."
        return feat.to(self.dtype) @ self.p(r + "weight_ih_l0").t() + self.p(r + "bias_ih_l0") + self.p(r + "bias_hh_l0")

    @torch.no_grad()
    def scan(self, gates, state=None, want_state=False):
        """gates [W, 256] (layer 0's pre-activations, biases included) -> probabilities [W]; ``state`` [4, 64] = h0, c0, h1, c1."""
        r = "decoder.rnn."
        g = gates.to(self.dtype)
        st = torch.zeros(4, 64, dtype=self.dtype) if state is None else state.to(self.dtype).clone()
        h0, c0, h1, c1 = st[0], st[1], st[2], st[3]
        whh0, wih1, whh1 = self.p(r + "weight_hh_l0"), self.p(r + "weight_ih_l1"), self.p(r + "weight_hh_l1")
        b1 = self.p(r + "bias_ih_l1") + self.p(r + "bias_hh_l1")
        wd, bd = self.p("decoder.decoder.1.weight").reshape(64), self.p("decoder.decoder.1.bias").reshape(())
        out = []

        def cell(pre, c):
            i, f, gg, o = pre[0:64], pre[64:128], pre[128:192], pre[192:256]
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            return torch.sigmoid(o) * torch.tanh(c), c
        for w in range(g.shape[0]):
            h0, c0 = cell(g[w] + whh0 @ h0, c0)
            h1, c1 = cell(b1 + wih1 @ h0 + whh1 @ h1, c1)
            out.append(torch.sigmoid(wd @ torch.relu(h1) + bd))
        probs = torch.stack(out) if out else torch.zeros(0, dtype=self.dtype)
        return (probs, torch.stack([h0, c0, h1, c1])) if want_state else probs

    def probs(self, x):
        return self.scan(self.frontend(x)[1])


# ------------------------------------------------------------------------------------------------ fixture
@functools.lru_cache(maxsize=1)
def golden():
    z = np.load(os.path.join(GOLDEN, "silero_vad.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def real_sd():
    return {k[len("sd/"):]: torch.from_numpy(v) for k, v in golden().items() if k.startswith("sd/")}


@functools.lru_cache(maxsize=None)
def clip(name):
    """The clip as float32 [n] at 16 kHz, decoded like librosa / the project's loader does (int16 / 32768)."""
    from scipy.io import wavfile
    rate, x = wavfile.read(os.path.join(GOLDEN, CLIPS[name]))
    assert rate == 16000 and x.dtype == np.int16 and x.ndim == 1
    return torch.from_numpy(x.astype(np.float32) / 32768.0)


@functools.lru_cache(maxsize=None)
def clip_ref(name):
    """(feat64, gates64, probs64) of a clip with the real weights: computed once, shared, never modified."""
    ref = VadRef(real_sd())
    feat, gates = ref.frontend(clip(name))
    return feat, gates, ref.scan(gates)


@functools.lru_cache(maxsize=None)
def clip_ref32(name):
    return VadRef(real_sd(), torch.float32).frontend(clip(name))


def fixture_spans(name, threshold):
    return [tuple(int(v) for v in r) for r in golden()[f"spans_{name}_{int(round(threshold * 100)):03d}"].reshape(-1, 2)]


@functools.lru_cache(maxsize=4)
def _model(ops, device, kind="real"):
    from svcmi.vad.utils import SileroVad
    sd = real_sd() if kind == "real" else WV.make_vad_state(rnn_scale=0.05)
    return SileroVad.from_state_dict(sd, device, ops=ops)


def model(ops, device, kind="real"):
    return _model(ops, str(device), kind)


def _i64(vals, device):
    return torch.tensor(list(vals), dtype=torch.int64).to(device)


# ------------------------------------------------------------------------------------------------ front-end
def run_frontend(ops, device, recs, vad=None):
    """recs: list of float32 [n_b] -> (feat [B, wmax, 64], gates [B, wmax, 256]) on the CPU; the recordings lie one after another in a
    buffer with poisoned gaps, so a read past a recording's end would show."""
    vad = vad or model(ops, device)
    gap = torch.full((37,), 1234.5)
    parts, offsets, off = [gap], [], 37
    for r in recs:
        offsets.append(off)
        parts += [r.float(), gap]
        off += r.shape[0] + 37
    flat = torch.cat(parts).to(device)
    lengths = [int(r.shape[0]) for r in recs]
    wmax = max(-(-n // WIN) for n in lengths)
    feat, gates = ops.vad_frontend(vad.cmodel, flat, _i64(offsets, device), _i64(lengths, device), wmax)
    return feat.cpu(), gates.cpu()


def check_frontend_windows(ops, device, W):
    """Real weights, the first W windows of 035 (W = 125: the whole clip, the last window 126 samples + zeros)."""
    x = clip("035")
    x = x if W == 125 else x[:W * WIN]
    feat, gates = run_frontend(ops, device, [x])
    f64, g64, _ = clip_ref("035")
    f32, g32 = clip_ref32("035")
    assert tuple(feat.shape) == (1, W, 64) and tuple(gates.shape) == (1, W, 256)
    if W < 125:
        _close64(feat[0], f64[:W], f32[:W], f"vad front-end 64-vector W={W}")
        return _close64(gates[0], g64[:W], g32[:W], f"vad front-end gate rows W={W}")
    # the last window of the whole clip is cut short there and full in the truncated runs: compare it apart
    _close64(feat[0], f64, f32, "vad front-end 64-vector, whole clip")
    return _close64(gates[0], g64, g32, "vad front-end gate rows, whole clip")


def edge_inputs():
    sq = torch.ones(WIN)
    sq[(torch.arange(WIN) // 16) % 2 == 1] = -1.0                     # full-scale +-1.0 square wave, period 32
    g = torch.Generator().manual_seed(5)
    return {"zeros": torch.zeros(WIN), "square": sq, "n513": 0.3 * torch.randn(513, generator=g), "n512": 0.3 * torch.randn(512, generator=g)}


def check_frontend_edges(ops, device):
    """A window of exact zeros (sqrt(0), log1p(0), BatchNorm of a constant), a full-scale square wave, 513 samples (the second window
    is one sample and 511 zeros), exactly 512 samples."""
    ref64, ref32 = VadRef(real_sd()), VadRef(real_sd(), torch.float32)
    for name, x in edge_inputs().items():
        feat, gates = run_frontend(ops, device, [x])
        W = -(-x.shape[0] // WIN)
        assert tuple(feat.shape) == (1, W, 64)
        assert bool(torch.isfinite(feat).all()) and bool(torch.isfinite(gates).all()), name
        f64, g64 = ref64.frontend(x)
        f32, g32 = ref32.frontend(x)
        _close64(feat[0], f64, f32, f"vad front-end 64-vector, {name}")
        _close64(gates[0], g64, g32, f"vad front-end gate rows, {name}")


def check_frontend_bits(ops, device):
    """Window 7 of 035: launched alone, as window 7 of 125, and inside a batch of three recordings -- the same bits; two runs too."""
    x = clip("035")
    solo_f, solo_g = run_frontend(ops, device, [x[7 * WIN:8 * WIN]])
    all_f, all_g = run_frontend(ops, device, [x])
    again_f, again_g = run_frontend(ops, device, [x])
    assert torch.equal(all_f, again_f) and torch.equal(all_g, again_g)
    assert torch.equal(solo_f[0, 0], all_f[0, 7]) and torch.equal(solo_g[0, 0], all_g[0, 7])
    b_f, b_g = run_frontend(ops, device, [x[:3 * WIN + 5], x[:9 * WIN], x[5 * WIN:8 * WIN]])
    assert tuple(b_f.shape) == (3, 9, 64)
    assert torch.equal(b_f[1, 7], all_f[0, 7]) and torch.equal(b_g[1, 7], all_g[0, 7])
    assert torch.equal(b_f[2, 2], all_f[0, 7]) and torch.equal(b_g[2, 2], all_g[0, 7])
    assert torch.equal(b_f[0, :3], all_f[0, :3]) and bool((b_f[0, 4:] == 0).all()) and bool((b_g[2, 3:] == 0).all())      # rows past W_b: untouched


# ------------------------------------------------------------------------------------------------ scan
def run_scan(ops, device, gates_list, vad=None, state=None):
    """gates_list: [W_b, 256] each -> (list of probabilities [W_b], the probs buffer, final state or None) through ONE launch."""
    vad = vad or model(ops, device)
    nw = [int(g.shape[0]) for g in gates_list]
    wmax = max(nw)
    buf = torch.full((len(nw), wmax, 256), 1234.5)
    for b, g in enumerate(gates_list):
        buf[b, :nw[b]] = g.float()
    st = None if state is None else state.clone().float().to(device)
    probs = ops.vad_lstm_scan(vad.cmodel, buf.to(device), _i64([WIN * w for w in nw], device), st).cpu()
    for b, w in enumerate(nw):
        assert bool((probs[b, w:] == 0).all()), "probabilities past a recording's last window were written"
    return [probs[b, :w] for b, w in enumerate(nw)], probs, (None if st is None else st.cpu())


def scan_bound(name):
    return 8.0 * float(golden()[f"ref_dev_{name}"])


def check_scan_lengths(ops, device, W):
    """W = 1 (no recurrence is read), 2 and 135 windows of 010 from the float64 front-end's gate rows (rounded once to fp32)."""
    _, g64, _ = clip_ref("010")
    g = g64[:W].float()
    got = run_scan(ops, device, [g])[0][0]
    want = VadRef(real_sd()).scan(g)
    err = float((got.double() - want).abs().max())
    print(f"vad scan W={W}: max |p - p64| = {err:.3e} (bound {scan_bound('010'):.3e})")
    assert err <= scan_bound("010"), (W, err)
    return err


def check_scan_ragged_and_repeat(ops, device):
    """Recordings of 3 and 17 windows in one launch are bit-equal to their solo runs; two runs give identical bits."""
    _, g64, _ = clip_ref("010")
    a, b = g64[40:43].float(), g64[60:77].float()
    both, raw, _ = run_scan(ops, device, [a, b])
    again, raw2, _ = run_scan(ops, device, [a, b])
    assert torch.equal(raw, raw2)
    assert torch.equal(both[0], run_scan(ops, device, [a])[0][0]) and torch.equal(both[1], run_scan(ops, device, [b])[0][0])
    assert float(both[1].max()) > 0.5 > float(both[1].min()) or float(both[1].std()) > 0       # a live track, not a constant


def check_scan_state_carry(ops, device):
    """Seven windows in one launch = the same windows one launch each with the state handed on: identical bits, and the state matches
    float64."""
    _, g64, _ = clip_ref("010")
    g = g64[50:57].float()
    whole, _, st_whole = run_scan(ops, device, [g], state=torch.zeros(1, 4, 64))
    st = torch.zeros(1, 4, 64)
    steps = []
    for w in range(7):
        p, _, st = run_scan(ops, device, [g[w:w + 1]], state=st)
        steps.append(p[0])
    assert torch.equal(torch.cat(steps), whole[0]) and torch.equal(st, st_whole)
    assert torch.equal(whole[0], run_scan(ops, device, [g])[0][0])                            # state = zeros is the NULL state
    _, want = VadRef(real_sd()).scan(g, want_state=True)
    assert float((st_whole[0].double() - want).abs().max()) <= 1e-4


def _scan_model_with(ops, device, edit):
    from svcmi.vad.utils import SileroVad
    sd = WV.make_vad_state(rnn_scale=0.05)
    edit(sd)
    return SileroVad.from_state_dict(sd, device, ops=ops), sd


def check_scan_saturation(ops, device):
    """Tiny recurrent weights, gate inputs of +-100: the sigmoids are exactly 0 / 1, nothing is NaN.  Layer 1 is made a pass-through of
    saturated gates as well (W_ih1 = W_hh1 = 0, biases +-100), the decoder reads relu(h1) with weight 1 / 64 and no bias:
        i = f = o = 1, g = +1:  c1 = w + 1 after window w, h1 = tanh(c1);   p = sigmoid(tanh(w + 1))
        o = 0:                  h1 = 0 exactly, p = sigmoid(0) = 0.5 exactly."""
    def edit(sd):
        for k in ("weight_ih_l1", "weight_hh_l1"):
            sd["decoder.rnn." + k].zero_()
        sd["decoder.rnn.bias_hh_l1"].zero_()
        sd["decoder.rnn.bias_ih_l1"].fill_(100.0)
        sd["decoder.decoder.1.weight"].fill_(1.0 / 64)
        sd["decoder.decoder.1.bias"].zero_()
    vad, sd = _scan_model_with(ops, device, edit)
    W = 6
    for gate_vals in ((100.0, 100.0, 100.0, 100.0), (-100.0, 100.0, -100.0, 100.0), (100.0, -100.0, 100.0, -100.0), (-100.0, -100.0, -100.0, -100.0)):
        g = torch.cat([torch.full((W, 64), v) for v in gate_vals], dim=1)
        got = run_scan(ops, device, [g], vad=vad)[0][0]
        assert bool(torch.isfinite(got).all())
        want = torch.tensor([1.0 / (1.0 + math.exp(-math.tanh(w + 1.0))) for w in range(W)], dtype=torch.float64)
        assert float((got.double() - want).abs().max()) <= 4 * 2.0 ** -24, (gate_vals, got)     # layer 0 cannot reach the output: W_ih1 = 0
        ref = VadRef(sd).scan(g)
        assert float((got.double() - ref).abs().max()) <= 4 * 2.0 ** -24

    def edit_o0(sd):
        edit(sd)
        sd["decoder.rnn.bias_ih_l1"][192:] = -100.0
    vad0, _ = _scan_model_with(ops, device, edit_o0)
    got = run_scan(ops, device, [torch.full((W, 256), 100.0)], vad=vad0)[0][0]
    assert bool((got == 0.5).all()), got


def check_scan_exact_cell_growth(ops, device, T=50):
    """Forget gate exactly 1 and i * tanh(g) exactly 1 for 50 steps in BOTH layers: c grows by exactly 1 per window (the state
    buffer shows c0 = c1 = t after t windows, to the bit), like tests/speaker_cases.py check_exact_cell_growth for the step kernel."""
    def edit(sd):
        r = "decoder.rnn."
        sd[r + "bias_hh_l1"].zero_()
        sd[r + "bias_ih_l1"][:192] = 100.0                 # i, f, g of layer 1 saturated; its o gate stays live
        sd[r + "weight_ih_l1"][:192].mul_(0.05)            # |W h| << 100: saturated whatever h is
    vad, sd = _scan_model_with(ops, device, edit)
    g = torch.full((T, 256), 100.0)
    g[:, 192:] = torch.randn(T, 64, generator=torch.Generator().manual_seed(5))
    state = torch.zeros(1, 4, 64)
    seen = []
    for t0 in (0, 20):                                      # 20 windows, then 30 more from the carried state
        n = 20 if t0 == 0 else T - 20
        p, _, state = run_scan(ops, device, [g[t0:t0 + n]], vad=vad, state=state)
        seen.append(p[0])
        assert bool((state[0, 1] == float(t0 + n)).all()) and bool((state[0, 3] == float(t0 + n)).all()), state[0, [1, 3]]
    ref = VadRef(sd).scan(g)
    assert float((torch.cat(seen).double() - ref).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ end to end
def check_probs_clip(ops, device, name):
    """|p - p64| <= 8 ref_dev of the clip (from the fixture), and that bound is below a twentieth of the clip's smallest distance between
    a reference probability and a decision level of threshold 0.2 (0.2 and 0.05): the spans cannot hinge on rounding."""
    z = golden()
    vad = model(ops, device)
    x = clip(name)
    got = vad.audio_forward(x, 16000)
    W = -(-x.shape[0] // WIN)
    assert tuple(got.shape) == (1, W) and got.dtype == torch.float32 and got.device.type == "cpu"
    p64 = clip_ref(name)[2]
    ref32 = torch.from_numpy(z[f"probs_{name}"]).double()
    assert ref32.shape[0] == W == {"035": 125, "010": 135}[name]
    bound = scan_bound(name)
    margin = float(torch.minimum((ref32 - 0.2).abs(), (ref32 - 0.05).abs()).min())
    err = float((got[0].double() - p64).abs().max())
    print(f"vad probabilities {name}: max |p - p64| = {err:.3e}, bound 8 x ref_dev = {bound:.3e}, decision margin {margin:.4f}")
    assert float((ref32 - p64).abs().max()) <= float(z[f"ref_dev_{name}"]) * (1 + 1e-6)          # the fixture's own figure, re-derived here
    assert bound < margin / 20.0, (bound, margin)
    assert err <= bound, (name, err, bound)
    return err


def check_batched_forward(ops, device):
    """Both clips in one call (two launches) = their solo runs, bit for bit; equal-length rows as a [B, n] tensor too."""
    vad = model(ops, device)
    a, b = clip("035"), clip("010")
    both = vad.audio_forward([a, b], 16000)
    assert torch.equal(both[0], vad.audio_forward(a, 16000)[0]) and torch.equal(both[1], vad.audio_forward(b, 16000)[0])
    two = vad.audio_forward(torch.stack([a[:5000], b[:5000]]), 16000)
    assert tuple(two.shape) == (2, 10) and torch.equal(two[0], vad.audio_forward(a[:5000], 16000)[0])
    # a 32 kHz input is decimated by striding, as the reference does
    up = torch.repeat_interleave(a[:4096], 2)
    assert torch.equal(vad.audio_forward(up, 32000), vad.audio_forward(a[:4096], 16000))


def check_call_keeps_state(ops, device):
    """model(chunk, sr) window by window, like the reference's loop, equals audio_forward; reset_states starts over."""
    vad = model(ops, device)
    x = clip("035")[:6 * WIN]
    whole = vad.audio_forward(x, 16000)[0]
    vad.reset_states()
    seq = torch.cat([vad(x[w * WIN:(w + 1) * WIN], 16000).cpu().reshape(-1) for w in range(6)])
    assert torch.equal(seq, whole)
    vad.reset_states()
    assert torch.equal(vad(x[:WIN], 16000).cpu().reshape(-1), whole[:1])


def check_spans(ops, device):
    from svcmi.vad.utils import get_speech_timestamps
    vad = model(ops, device)
    for name in CLIPS:
        for thr in (0.2, 0.5):
            got = get_speech_timestamps(clip(name), vad, threshold=thr, sampling_rate=16000)
            assert [(t["start"], t["end"]) for t in got] == fixture_spans(name, thr), (name, thr, got)
    assert fixture_spans("035", 0.2) == [(1568, 50144)] and fixture_spans("010", 0.2) == [(1056, 36320), (40480, 61408)]


# ------------------------------------------------------------------------------------------------ mask
def mask_ref(x, spans, n_ref, ratio=2):
    """svc_inference_post.py:39-49 in numpy."""
    m = np.zeros(n_ref, dtype=np.float32)
    for a, b in spans:
        m[a:b] = 1
    m = np.repeat(m, ratio, -1)
    n = min(len(m), len(x))
    out = x[:n].copy()
    out[m[:n] == 0] = 0
    return out


def check_mask(ops, device):
    rng = np.random.default_rng(3)
    n_ref = 1000
    two = [(100, 250), (400, 777)]
    for spans in ([], [(0, n_ref)], two):
        for n_in in (2 * n_ref, 2 * n_ref - 37, 2 * n_ref + 101, 1501):             # equal, shorter, longer, odd
            x = (rng.standard_normal(n_in) + 3.0).astype(np.float32)                # no zeros of its own
            sp = torch.tensor(spans, dtype=torch.int32).reshape(-1, 2).to(device)
            got = ops.mask_spans(torch.from_numpy(x).to(device), sp, n_ref, 2).cpu().numpy()
            want = mask_ref(x, spans, n_ref)
            assert got.shape == want.shape == (min(n_in, 2 * n_ref),)
            assert np.array_equal(got, want), (spans, n_in)
            if not spans:
                assert not got.any()
            if spans == two and n_in >= 2 * n_ref:
                for a, b in two:
                    assert got[2 * a - 1] == 0 and got[2 * a] == x[2 * a] and got[2 * b - 1] == x[2 * b - 1] and got[2 * b] == 0
    # more than one block per grid stride, spans at the very ends, ratio 3
    n_ref, n_in = 300000, 3 * 300000 - 5
    spans = [(0, 7), (9, 100000), (100001, 299999)]
    x = (rng.standard_normal(n_in) + 3.0).astype(np.float32)
    got = ops.mask_spans(torch.from_numpy(x).to(device), torch.tensor(spans, dtype=torch.int32).to(device), n_ref, 3).cpu().numpy()
    assert np.array_equal(got, mask_ref(x, spans, n_ref, 3))


# ------------------------------------------------------------------------------------------------ post-filter
def post_inputs():
    x = clip("035")
    svc = (torch.randn(2 * x.shape[0] - 37, generator=torch.Generator().manual_seed(11)) * 0.2 + 0.5).numpy()
    return x.numpy(), svc


def check_apply_vad_post(ops, device):
    from svcmi.svc_inference_post import apply_vad_post
    vad = model(ops, device)
    ref, svc = post_inputs()
    want = mask_ref(svc, fixture_spans("035", 0.2), ref.shape[0])
    got = apply_vad_post(ref, svc, vad, threshold=0.2)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want)
    assert not got[:3136].any() and not got[100288:].any() and got[3136:100288].all()
    got_t = apply_vad_post(torch.from_numpy(ref), torch.from_numpy(svc).to(device), vad)
    assert torch.is_tensor(got_t) and got_t.device.type == torch.device(device).type and np.array_equal(got_t.cpu().numpy(), want)


def check_post_cli(ops, device, tmp_path):
    """The command line with a resident model: a 32 kHz float wav with the masked content."""
    from scipy.io import wavfile
    from svcmi import svc_inference_post as P
    ref, svc = post_inputs()
    svc_path, out_path = os.path.join(str(tmp_path), "svc_out.wav"), os.path.join(str(tmp_path), "svc_out_post.wav")
    wavfile.write(svc_path, 32000, svc)
    args = P.build_parser().parse_args(["--ref", os.path.join(GOLDEN, "035.wav"), "--svc", svc_path, "--out", out_path])
    assert args.vad == os.path.join("vad", "assets", "silero_vad.jit")
    P.main(args, vad=model(ops, device))
    rate, y = wavfile.read(out_path)
    assert rate == 32000 and y.dtype == np.float32
    assert np.array_equal(y, mask_ref(svc, fixture_spans("035", 0.2), ref.shape[0]))


# ------------------------------------------------------------------------------------------------ state machine
class Replay:
    """Stand-in model: replays a stored probability track."""

    def __init__(self, track):
        self.track = torch.as_tensor(np.asarray(track, dtype=np.float64))

    def reset_states(self):
        pass

    def audio_forward(self, x, sr, num_samples=512):
        assert -(-int(torch.as_tensor(x).reshape(-1).shape[0]) // num_samples) == self.track.shape[0]
        return self.track[None]


def state_machine_cases():
    """Every stored case: (params dict, track float32 [W], audio length in samples, the reference's spans [[start, end]])."""
    z = golden()
    params = json.loads(str(z["sm_params"]))
    t_off = np.concatenate([[0], np.cumsum(z["sm_windows"])])
    s_off = np.concatenate([[0], np.cumsum(z["sm_nspans"])])
    spans = z["sm_spans"].reshape(-1, 2)
    for i in range(len(z["sm_windows"])):
        yield params[int(z["sm_pset"][i])], z["sm_tracks"][t_off[i]:t_off[i + 1]], int(z["sm_samples"][i]), spans[s_off[i]:s_off[i + 1]].tolist()
