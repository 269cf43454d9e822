"""Host-side checks of the voice-activity detector that need no GPU: the new symbols are there under the unchanged ABI number, the struct
layout matches the binding, the workspace query has its documented value, every entry point rejects bad arguments before it touches the
device, and the loader rejects what it does not support."""
import ctypes
import importlib.util
import os

import pytest
import torch

from workload import vad as WV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
NEW = ("svcmi_vad_model_bytes", "svcmi_vad_frontend_f32", "svcmi_vad_lstm_scan_f32", "svcmi_mask_spans_f32", "svcmi_vad_workspace_bytes",
       "svcmi_vad_probs_fwd")


@pytest.fixture(scope="module")
def lib():
    from svcmi import _lib
    spec = importlib.util.spec_from_file_location("svcmi_build", os.path.join(ROOT, "whisper-vits-svc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return _lib.load_library(mod.build_hip())


def test_new_symbols_under_the_same_abi_version(lib):
    from svcmi import _lib
    assert _lib.ABI_VERSION == 22 and lib.svcmi_abi_version() == 22
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_struct_sizes_match_ctypes(lib):
    from svcmi import _lib
    assert ctypes.sizeof(_lib.VadConvBlock) == 6 * 8 + 8 and ctypes.sizeof(_lib.VadDown) == 4 * 8 + 8
    assert lib.svcmi_vad_model_bytes() == ctypes.sizeof(_lib.VadModel) == 2 * 8 + 4 * 56 + 4 * 40 + 7 * 8 + 8


def test_workspace_bytes_documented_value(lib):
    f = lib.svcmi_vad_workspace_bytes
    assert f(1, 1) == 1280 * 1 * 1 + 256 == 1536
    assert f(3, 125) == 1280 * 3 * 125 + 256 == 480256
    assert f(0, 5) == EINVAL and f(2, 0) == EINVAL


def _aligned(nfloats):
    buf = (ctypes.c_float * (nfloats + 64))()
    return buf, (ctypes.addressof(buf) + 255) & ~255


def _model(p):
    """A struct whose pointers all aim at one host buffer: enough for the argument checks, nothing is launched."""
    from svcmi import _lib
    m = _lib.VadModel()
    for k in ("basis_t", "filt", "gate0_w", "gate0_b", "whh0_t", "wih1_t", "whh1_t", "gate1_b", "dec_w"):
        setattr(m, k, p)
    for i, (cin, cout, stride) in enumerate(((258, 16, 2), (16, 32, 2), (32, 32, 2), (32, 64, 1))):
        b, d = m.block[i], m.down[i]
        b.dw_w = b.dw_b = b.pw_w = b.pw_b = p
        if cin != cout:
            b.proj_w = b.proj_b = p
        b.c_in, b.c_out = cin, cout
        d.w = d.b = d.scale = d.shift = p
        d.c, d.stride = cout, stride
    return m


def test_kernel_entry_points_validate_without_a_gpu(lib):
    keep, p = _aligned(4096)
    m = _model(p)
    M = ctypes.byref(m)
    fe, sc = lib.svcmi_vad_frontend_f32, lib.svcmi_vad_lstm_scan_f32
    assert fe(None, p, p, p, 1, 1, p, p, None) == EINVAL
    for bad in range(1, 4):
        a = [p, p, p]
        a[bad - 1] = None
        assert fe(M, a[0], a[1], a[2], 1, 1, p, p, None) == EINVAL
    assert fe(M, p, p, p, 1, 1, None, p, None) == EINVAL and fe(M, p, p, p, 1, 1, p, None, None) == EINVAL
    assert fe(M, p, p, p, 0, 1, p, p, None) == EINVAL and fe(M, p, p, p, 1, 0, p, p, None) == EINVAL
    assert fe(M, p, p, p, 65536, 1, p, p, None) == EUNSUPPORTED
    assert fe(M, p + 2, p, p, 1, 1, p, p, None) == EALIGN and fe(M, p, p + 4, p, 1, 1, p, p, None) == EALIGN
    assert sc(None, p, p, 1, 1, None, p, None) == EINVAL and sc(M, None, p, 1, 1, None, p, None) == EINVAL
    assert sc(M, p, None, 1, 1, None, p, None) == EINVAL and sc(M, p, p, 1, 1, None, None, None) == EINVAL
    assert sc(M, p, p, 0, 1, None, p, None) == EINVAL and sc(M, p, p, 1, 0, None, p, None) == EINVAL
    assert sc(M, p, p, 1, 1, p + 1, p, None) == EALIGN
    # a model of another architecture, or with a hole in it
    m2 = _model(p)
    m2.block[1].c_out = 48
    assert fe(ctypes.byref(m2), p, p, p, 1, 1, p, p, None) == EUNSUPPORTED
    m3 = _model(p)
    m3.down[2].stride = 1
    assert sc(ctypes.byref(m3), p, p, 1, 1, None, p, None) == EUNSUPPORTED
    m4 = _model(p)
    m4.whh1_t = None
    assert sc(ctypes.byref(m4), p, p, 1, 1, None, p, None) == EINVAL
    m5 = _model(p)
    m5.block[0].proj_b = None
    assert fe(ctypes.byref(m5), p, p, p, 1, 1, p, p, None) == EINVAL


def test_mask_and_stage_validate_without_a_gpu(lib):
    keep, p = _aligned(4096)
    mk = lib.svcmi_mask_spans_f32
    assert mk(None, 10, p, 1, 10, 2, p, 10, None) == EINVAL and mk(p, 10, p, 1, 10, 2, None, 10, None) == EINVAL
    assert mk(p, 0, p, 1, 10, 2, p, 0, None) == EINVAL and mk(p, 10, p, 1, 0, 2, p, 0, None) == EINVAL and mk(p, 10, p, 1, 10, 0, p, 0, None) == EINVAL
    assert mk(p, 10, None, 1, 10, 2, p, 10, None) == EINVAL and mk(p, 10, p, -1, 10, 2, p, 10, None) == EINVAL
    assert mk(p, 30, p, 1, 10, 2, p, 30, None) == EINVAL and mk(p, 15, p, 1, 10, 2, p, 20, None) == EINVAL      # n_out is min(n_in, ratio n_ref)
    assert mk(p + 2, 10, p, 1, 10, 2, p, 10, None) == EALIGN
    m = _model(p)
    M = ctypes.byref(m)
    st = lib.svcmi_vad_probs_fwd
    need = lib.svcmi_vad_workspace_bytes(2, 3)
    big, ws = _aligned(need // 4 + 64)
    assert st(None, p, p, p, 2, 3, None, p, ws, need, None) == EINVAL and st(M, None, p, p, 2, 3, None, p, ws, need, None) == EINVAL
    assert st(M, p, p, p, 2, 3, None, None, ws, need, None) == EINVAL and st(M, p, p, p, 2, 3, None, p, None, need, None) == EINVAL
    assert st(M, p, p, p, 0, 3, None, p, ws, need, None) == EINVAL and st(M, p, p, p, 2, 0, None, p, ws, need, None) == EINVAL
    assert st(M, p, p, p, 2, 3, None, p, ws, need - 256, None) == EINVAL and st(M, p, p, p, 2, 3, None, p, ws + 16, need, None) == EINVAL


def test_weights_layout_and_wrong_shapes():
    from svcmi import weights as PW
    sd = WV.make_vad_state()
    w = PW.VadWeights(sd, "cpu")
    assert tuple(w.basis_t.shape) == (256, 260) and torch.equal(w.basis_t[:, :258].t(), sd["feature_extractor.forward_basis_buffer"][:, 0])
    assert bool((w.basis_t[:, 258:] == 0).all())
    r = "decoder.rnn."
    assert torch.equal(w.gate0_b, sd[r + "bias_ih_l0"] + sd[r + "bias_hh_l0"]) and torch.equal(w.gate1_b, sd[r + "bias_ih_l1"] + sd[r + "bias_hh_l1"])
    assert float(sd[r + "bias_hh_l1"].abs().max()) > 0.1                  # non-zero: a missing b_hh would show
    assert torch.equal(w.whh0_t, sd[r + "weight_hh_l0"].t()) and w.whh0_t.is_contiguous() and tuple(w.wih1_t.shape) == (64, 256)
    assert w.blocks[2]["proj_w"] is None and w.blocks[0]["proj_w"].shape == (16, 258) and [d["stride"] for d in w.downs] == [2, 2, 2, 1]
    bn = w.downs[1]
    scale = sd["encoder.5.weight"] / torch.sqrt(sd["encoder.5.running_var"] + 1e-5)
    assert torch.equal(bn["scale"], scale) and torch.equal(bn["shift"], sd["encoder.5.bias"] - sd["encoder.5.running_mean"] * scale)
    assert torch.equal(bn["w"], sd["encoder.4.weight"][:, :, 0])          # BatchNorm is not folded into the convolution
    bad = dict(sd)
    bad["decoder.rnn.weight_hh_l0"] = torch.zeros(256, 32)
    with pytest.raises(ValueError, match="weight_hh_l0"):
        PW.VadWeights(bad, "cpu")
    bad = dict(sd)
    bad["feature_extractor.forward_basis_buffer"] = torch.zeros(130, 1, 128)      # the 8 kHz model's basis
    with pytest.raises(ValueError, match="forward_basis_buffer"):
        PW.VadWeights(bad, "cpu")
    missing = {k: v for k, v in sd.items() if k != "encoder.11.0.proj.weight"}
    with pytest.raises(KeyError):
        PW.VadWeights(missing, "cpu")


def test_restatement_matches_torch_modules():
    """The float64 restatement's LSTM scan is torch's own nn.LSTM (2 layers, one step per window, state carried) + the decoder."""
    from tests import vad_cases as V
    sd = WV.make_vad_state()
    ref = V.VadRef(sd)
    x = 0.2 * torch.randn(5 * 512 + 100, generator=torch.Generator().manual_seed(1))
    feat, gates = ref.frontend(x)
    assert tuple(feat.shape) == (6, 64) and tuple(gates.shape) == (6, 256)
    lstm = torch.nn.LSTM(64, 64, num_layers=2).double()
    with torch.no_grad():
        for k, v in lstm.named_parameters():
            v.copy_(sd["decoder.rnn." + k].double())
        h = lstm(feat[:, None])[0][:, 0]
        want = torch.sigmoid(torch.relu(h) @ sd["decoder.decoder.1.weight"].double().reshape(64) + sd["decoder.decoder.1.bias"].double())
    assert float((ref.scan(gates) - want).abs().max()) <= 1e-14


def test_post_parser_matches_the_reference_flags():
    from svcmi import svc_inference_post as P
    a = P.build_parser().parse_args(["--ref", "a.wav", "--svc", "b.wav", "--out", "c.wav"])
    assert (a.ref, a.svc, a.out) == ("a.wav", "b.wav", "c.wav")
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(["--ref", "a.wav", "--svc", "b.wav"])
