"""Host-side checks of the speaker encoder that need no GPU: every entry point rejects bad arguments before it touches the device
(against the hipcc-built library, like tests/test_abi.py), the ABI number is unchanged by the addition, the weight packing is the
permutation the step kernel expects, and the references of tests/speaker_cases.py agree with each other."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from svcmi import _lib
    spec = importlib.util.spec_from_file_location("svcmi_build", os.path.join(ROOT, "whisper-vits-svc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return _lib.load_library(mod.build_hip())


def test_abi_version_unchanged(lib):
    from svcmi import _lib
    assert _lib.ABI_VERSION == 22 and lib.svcmi_abi_version() == 22
    for name in ("svcmi_lstm_step_f32", "svcmi_preemph_pad_f32", "svcmi_magnitude_spectrum_f32", "svcmi_speaker_mel_finish_f32",
                 "svcmi_l2norm_rows_f32", "svcmi_group_mean_f32", "svcmi_speaker_encoder_fwd", "svcmi_speaker_encoder_workspace_bytes"):
        assert name in _lib.SIGNATURES


def _aligned(nfloats):
    buf = (ctypes.c_float * (nfloats + 64))()
    base = (ctypes.addressof(buf) + 255) & ~255
    return buf, base


def test_step_kernel_validation_needs_no_gpu(lib):
    keep, p = _aligned(65536)
    f = lib.svcmi_lstm_step_f32
    H, T, B = 8, 3, 2
    ok = dict(gx=p, gx_bs=T * 4 * H, whh=p, hseq=p, h_bs=T * H, ldh=H, c=p, ldc=H, batch=B, hidden=H, t=1, t_total=T)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["gx"], a["gx_bs"], a["whh"], a["hseq"], a["h_bs"], a["ldh"], a["c"], a["ldc"], a["batch"], a["hidden"], a["t"], a["t_total"], None)
    for name in ("gx", "whh", "hseq", "c"):
        assert call(**{name: None}) == EINVAL
    assert call(batch=0) == EINVAL and call(t_total=0) == EINVAL and call(t=-1) == EINVAL and call(t=T) == EINVAL
    assert call(hidden=0) == EINVAL and call(ldh=H - 4) == EINVAL and call(ldc=H - 1) == EINVAL
    assert call(batch=65) == EUNSUPPORTED
    assert call(hidden=6, ldh=8, ldc=8) == EALIGN                         # not a multiple of the unit tile
    assert call(whh=p + 4) == EALIGN and call(hseq=p + 8) == EALIGN       # misaligned rows
    assert call(ldh=H + 2, h_bs=T * (H + 2)) == EALIGN


def test_small_kernel_validation_needs_no_gpu(lib):
    keep, p = _aligned(4096)
    assert lib.svcmi_preemph_pad_f32(None, p, 1, 1024, 512, 0.98, None) == EINVAL
    assert lib.svcmi_preemph_pad_f32(p, p, 1, 512, 512, 0.98, None) == EINVAL           # a reflect pad needs pad < n
    assert lib.svcmi_preemph_pad_f32(p, p, 0, 1024, 512, 0.98, None) == EINVAL
    assert lib.svcmi_magnitude_spectrum_f32(p, None, 5, 513, 516, 1032, 516, None) == EINVAL
    assert lib.svcmi_magnitude_spectrum_f32(p, p, 5, 513, 512, 1032, 516, None) == EINVAL
    assert lib.svcmi_speaker_mel_finish_f32(None, 10, 20.0, -100.0, 4.0, None) == EINVAL
    assert lib.svcmi_speaker_mel_finish_f32(p, 10, 20.0, 0.0, 4.0, None) == EINVAL
    assert lib.svcmi_l2norm_rows_f32(p, 4, 2, 8, p, 8, None) == EINVAL
    assert lib.svcmi_group_mean_f32(p, 0, 1, 8, p, None) == EINVAL


def _model(lib, H=8, D=4, P=4, L=2, whh_off=0):
    from svcmi import _lib
    keep, p = _aligned(65536)
    m = _lib.SpeakerModel()
    m.input_dim, m.lstm_dim, m.proj_dim, m.n_layers = D, H, P, L
    for i in range(L):
        ly = m.layers[i]
        ly.ih.w, ly.ih.bias, ly.ih.n, ly.ih.ldw = p, p, 4 * H, D if i == 0 else P
        ly.lin.w, ly.lin.bias, ly.lin.n, ly.lin.ldw = p, None, P, H
        ly.whh = p + whh_off
    return m, keep, p


def test_stage_validation_needs_no_gpu(lib):
    f, wsb = lib.svcmi_speaker_encoder_fwd, lib.svcmi_speaker_encoder_workspace_bytes
    m, keep, p = _model(lib)
    need = wsb(ctypes.byref(m), 2, 3)
    assert need > 0
    big, ws = _aligned(need // 4 + 64)
    assert f(None, p, 2, 3, p, ws, need, None) == EINVAL
    assert f(ctypes.byref(m), None, 2, 3, p, ws, need, None) == EINVAL
    assert f(ctypes.byref(m), p, 2, 3, None, ws, need, None) == EINVAL
    assert f(ctypes.byref(m), p, 2, 3, p, None, need, None) == EINVAL
    assert f(ctypes.byref(m), p, 0, 3, p, ws, need, None) == EINVAL and wsb(ctypes.byref(m), 0, 3) == EINVAL       # B < 1
    assert f(ctypes.byref(m), p, 2, 0, p, ws, need, None) == EINVAL and wsb(ctypes.byref(m), 2, 0) == EINVAL       # T < 1
    assert f(ctypes.byref(m), p, 65, 3, p, ws, need, None) == EUNSUPPORTED and wsb(ctypes.byref(m), 65, 3) == EUNSUPPORTED
    assert f(ctypes.byref(m), p, 2, 3, p, ws, need - 1024, None) == EINVAL                                          # workspace too small
    assert f(ctypes.byref(m), p, 2, 3, p, ws + 16, need, None) == EINVAL
    m6, keep6, _ = _model(lib, H=6)
    assert f(ctypes.byref(m6), p, 2, 3, p, ws, need, None) == EALIGN and wsb(ctypes.byref(m6), 2, 3) == EALIGN      # H % unit tile
    mo, keepo, _ = _model(lib, whh_off=4)
    assert f(ctypes.byref(mo), p, 2, 3, p, ws, need, None) == EALIGN                                                # misaligned W_hh rows
    m0, keep0, _ = _model(lib, L=2)
    m0.n_layers = 0
    assert f(ctypes.byref(m0), p, 2, 3, p, ws, need, None) == EINVAL
    m0.n_layers = 9
    assert f(ctypes.byref(m0), p, 2, 3, p, ws, need, None) == EINVAL


def test_tile_order_and_packing():
    from svcmi import weights as PW
    from workload import speaker as WS
    perm = PW.lstm_tile_order(8)
    # unit tile 0 = units 0..3: gates i, f, g, o of those units, then the same for units 4..7
    assert perm.tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27, 4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 28, 29, 30, 31]
    with pytest.raises(ValueError):
        PW.lstm_tile_order(6)
    sd = WS.make_speaker_state(**WS.TINY)
    w = PW.SpeakerWeights(sd, "cpu")
    assert (w.input_dim, w.proj_dim, w.lstm_dim, len(w.layers)) == (12, 20, 40, 3)
    p40 = PW.lstm_tile_order(40)
    for i, ly in enumerate(w.layers):
        assert torch.equal(ly["whh"], sd[f"layers.{i}.lstm.weight_hh_l0"][p40])
        assert torch.equal(ly["ih_w"], sd[f"layers.{i}.lstm.weight_ih_l0"][p40])
        assert torch.equal(ly["bias"], (sd[f"layers.{i}.lstm.bias_ih_l0"] + sd[f"layers.{i}.lstm.bias_hh_l0"])[p40])
        assert ly["whh"].data_ptr() % 16 == 0
    assert float(sd["layers.0.lstm.bias_hh_l0"].abs().max()) > 0.1          # non-zero biases: a missing b_hh would show


def test_references_agree():
    """torch's float64 nn.LSTM / nn.Linear chain is the written-out formula; torch's fp32 chain is close to it (the path is well
    conditioned: the bound of the numeric checks is tight)."""
    from tests import speaker_cases as S
    from workload import speaker as WS
    sd = WS.make_speaker_state(**WS.TINY)
    x = 2.0 * torch.randn(3, 7, 12, generator=torch.Generator().manual_seed(3))
    a, b = S.encoder_ref(sd, x, torch.float64), S.encoder_formula64(sd, x)
    assert float((a - b).abs().max()) <= 1e-14
    assert float((S.encoder_ref(sd, x, torch.float32).double() - a).abs().max()) <= 1e-6
    gx, w_hh = S.step_inputs(3, 7, 20, seed=1)
    h64, c64 = S.lstm_layer64(gx, w_hh)
    h32, c32 = S.lstm_layer32(gx, w_hh)
    assert float((h32.double() - h64).abs().max()) <= 1e-6 and float((c32.double() - c64[:, -1]).abs().max()) <= 2e-6


def test_cli_parser_and_commented_config(tmp_path):
    from svcmi.speaker import infer
    from tests import speaker_cases as S
    a = infer.build_parser().parse_args(["m.pth", "c.json", "-s", "in.wav", "-t", "out.npy"])
    assert (a.model_path, a.config_path, a.source, a.target, a.loader) == ("m.pth", "c.json", "in.wav", "out.npy", "host")
    a = infer.build_parser().parse_args(["m.pth", "c.json", "--folder", "d", "--mean", "o.npy", "--loader", "gpu"])
    assert (a.folder, a.mean, a.loader) == ("d", "o.npy", "gpu")
    _, _, config = S.write_model(tmp_path)
    cfg = infer.read_json(config)
    assert cfg["audio"]["trim_db"] == 60 and cfg["audio"]["preemphasis"] == 0.98 and cfg["model"]["lstm_dim"] == 40
    with pytest.raises(SystemExit):
        infer.main(["m.pth", "c.json", "-s", "in.wav"])
