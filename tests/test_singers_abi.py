"""Host-side checks of the singer sweep that need no GPU: the new symbols are there under the unchanged ABI number, the io struct's layout
matches the binding, and every entry point rejects bad arguments before it touches the device or any buffer."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
NEW = ("svcmi_sweep_sample_prior_f32", "svcmi_singers_io_bytes", "svcmi_synth_singers_workspace_bytes", "svcmi_synth_singers_fwd")
FILL = 0xA5


@pytest.fixture(scope="module")
def lib():
    from svcmi import _lib
    spec = importlib.util.spec_from_file_location("svcmi_build", os.path.join(ROOT, "whisper-vits-svc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return _lib.load_library(mod.build_hip())


@pytest.fixture(scope="module")
def cmodel():
    """A filled svcmi_synth_model (tiny configuration, host pointers of the emulator build): the planning pass and the argument checks
    read its sizes only."""
    from tests import engine_cases as E
    from tests.emu import emu_ops
    from workload import config as C
    m, _ = E.make_model(C.tiny_hp(), emu_ops(), "cpu")
    return m._cmodel()


def test_new_symbols_under_the_same_abi_version(lib):
    from svcmi import _lib
    assert _lib.ABI_VERSION == 22 and lib.svcmi_abi_version() == 22
    header = open(os.path.join(ROOT, "include", "svcmi.h")).read()
    assert "#define SVCMI_ABI_VERSION 22" in header
    assert "#define SVCMI_SINGERS_MAX 32" in header and _lib.SINGERS_MAX == 32
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    # the ctypes rows have the header's argument counts
    for name in NEW:
        proto = re.search(name + r"\(([^)]*)\)", header).group(1)
        n_args = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    from svcmi.ops import Ops
    for name in ("sweep_sample_prior", "synth_singers_fwd", "synth_singers_workspace_bytes"):
        assert callable(getattr(Ops, name))


def test_io_struct_size_matches_ctypes(lib):
    from svcmi import _lib
    assert lib.svcmi_singers_io_bytes() == ctypes.sizeof(_lib.SingersIO) == 7 * 8 + 4 * 4 + 2 * 8
    assert _lib.SingersIO.spk.offset == 40 and _lib.SingersIO.ppg_row_shift.offset == 56 and _lib.SingersIO.wave.offset == 72
    assert [f[0] for f in _lib.SingersIO._fields_] == ["ppg", "vec", "pit", "length", "source", "spk", "noise", "ppg_row_shift", "t", "n_singers",
                                                       "stream_frames", "wave", "z_p"]


def test_the_kernel_has_a_row_in_the_trace_table_and_no_name_is_lost(lib):
    from svcmi import _lib
    names = []
    while lib.svcmi_trace_op_name(len(names)):
        names.append(lib.svcmi_trace_op_name(len(names)).decode())
    assert names.count("svcmi_sweep_sample_prior_f32") == 1 and len(set(names)) == len(names)
    assert names[names.index("svcmi_sweep_sample_prior_f32") - 1] == "svcmi_sample_prior_f32"       # beside the kernel whose arithmetic it shares
    for name in ("svcmi_embed_pitch_f32", "svcmi_copy2d_f32", "svcmi_sweep_pitch_f32", "svcmi_sweep_embed_f32", "svcmi_yin_aperiodicity_f64"):
        assert name in names
    sizes = (ctypes.c_int64 * 8)()
    assert lib.svcmi_struct_sizes(sizes, 8) == 7 and sizes[3] == ctypes.sizeof(_lib.SynthIO)          # svcmi_synth_io keeps its layout


class Buffers:
    """One host buffer filled with a pattern: every pointer the entry points get aims into it, and it must come back untouched."""

    def __init__(self, nbytes):
        self.raw = (ctypes.c_ubyte * (nbytes + 512))()
        ctypes.memset(self.raw, FILL, len(self.raw))
        self.p = (ctypes.addressof(self.raw) + 255) & ~255

    def untouched(self):
        return bytes(self.raw) == bytes([FILL]) * len(self.raw)


def test_kernel_entry_point_validates_without_a_gpu(lib):
    buf = Buffers(1 << 16)
    p = buf.p
    sp = lib.svcmi_sweep_sample_prior_f32
    call = lambda stats=p, lds=16, noise=p, ln=p, z=p, ldz=8, S=3, t=5, i=8: sp(stats, lds, noise, ln, z, ldz, S, t, i, None)
    for hole in ("stats", "noise", "z"):
        assert call(**{hole: None}) == EINVAL, hole
    for bad in (dict(S=0), dict(S=-1), dict(t=0), dict(i=0), dict(lds=15), dict(ldz=7)):
        assert call(**bad) == EINVAL, bad
    assert call(S=33) == EUNSUPPORTED
    for arg in ("stats", "noise", "ln", "z"):
        assert call(**{arg: p + 2}) == EALIGN, arg
    assert call(S=33, stats=None) == EINVAL                       # the order of svcmi_sweep_embed_f32: arguments, then the row limit
    assert buf.untouched()


def test_workspace_query_and_stage_validate_without_a_gpu(lib, cmodel):
    from svcmi import _lib
    M = ctypes.byref(cmodel.struct)
    wsb, st = lib.svcmi_synth_singers_workspace_bytes, lib.svcmi_synth_singers_fwd
    assert wsb(M, 0, 37, 0) == EINVAL and wsb(M, 33, 37, 0) == EUNSUPPORTED and wsb(M, 3, 0, 0) == EINVAL and wsb(None, 3, 37, 0) == EINVAL
    assert wsb(M, -1, 37, 0) < 0
    need1, need3 = wsb(M, 1, 37, 0), wsb(M, 3, 37, 0)
    assert 0 < need1 < need3
    assert need1 <= lib.svcmi_synth_workspace_bytes(M, 1, 37, 0)          # one singer needs no more than one clip through svcmi_synth_infer_fwd
    # three singers: one prior encoder, so less than the batch-3 stage, which runs three
    assert need3 <= lib.svcmi_synth_workspace_bytes(M, 3, 37, 0) + 3 * 37 * 320 * 4 + 1024
    buf = Buffers(4096)
    p = buf.p
    io = _lib.SingersIO()
    io.ppg = io.vec = io.pit = io.spk = io.length = io.source = io.noise = io.wave = p
    io.t, io.n_singers = 37, 3
    big = need3 + 4096
    assert st(M, ctypes.byref(io), p, need3 - 1, None) == EINVAL                  # a short workspace
    assert st(M, ctypes.byref(io), p, 0, None) == EINVAL
    assert st(None, ctypes.byref(io), p, big, None) == EINVAL and st(M, None, p, big, None) == EINVAL and st(M, ctypes.byref(io), None, big, None) == EINVAL
    assert st(M, ctypes.byref(io), p + 16, big, None) == EINVAL                   # the workspace wants 256-byte alignment
    for hole in ("ppg", "vec", "pit", "spk", "length", "source", "noise", "wave"):
        bad = _lib.SingersIO.from_buffer_copy(io)
        setattr(bad, hole, None)
        assert st(M, ctypes.byref(bad), p, big, None) == EINVAL, hole
    for k, want in ((0, EINVAL), (33, EUNSUPPORTED), (-2, EINVAL)):
        bad = _lib.SingersIO.from_buffer_copy(io)
        bad.n_singers = k
        assert st(M, ctypes.byref(bad), p, big, None) == want, k
    for field, v in (("t", 0), ("ppg_row_shift", 2)):
        bad = _lib.SingersIO.from_buffer_copy(io)
        setattr(bad, field, v)
        assert st(M, ctypes.byref(bad), p, big, None) == EINVAL, field
    assert buf.untouched()


def test_emulator_stage_refuses_a_short_workspace(cmodel):
    """The same refusal through the library that can launch: nothing is written."""
    from svcmi import _lib
    from tests.emu import emu_ops
    lib = emu_ops().lib
    M = ctypes.byref(cmodel.struct)
    need = lib.svcmi_synth_singers_workspace_bytes(M, 2, 5, 0)
    assert need > 0
    small = torch.full((need + 512,), FILL, dtype=torch.uint8)
    base = (small.data_ptr() + 255) & ~255
    io = _lib.SingersIO()
    io.ppg = io.vec = io.pit = io.spk = io.length = io.source = io.noise = io.wave = base
    io.t, io.n_singers = 5, 2
    assert lib.svcmi_synth_singers_fwd(M, ctypes.byref(io), base, need - 1, 0) == EINVAL
    assert bool((small == FILL).all())
