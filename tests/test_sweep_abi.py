"""Host-side checks of the key sweep that need no GPU: the new symbols are there under the unchanged ABI number, the io struct's layout
matches the binding, and every entry point rejects bad arguments before it touches the device or any buffer."""
import ctypes
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
NEW = ("svcmi_sweep_pitch_f32", "svcmi_sweep_embed_f32", "svcmi_sweep_io_bytes", "svcmi_synth_sweep_workspace_bytes", "svcmi_synth_sweep_fwd")
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
    assert "#define SVCMI_SWEEP_MAX_KEYS 32" in header and _lib.SWEEP_MAX_KEYS == 32
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    from svcmi.ops import Ops
    for name in ("sweep_pitch", "sweep_embed", "synth_sweep_fwd"):
        assert callable(getattr(Ops, name))


def test_io_struct_size_matches_ctypes(lib):
    from svcmi import _lib
    assert lib.svcmi_sweep_io_bytes() == ctypes.sizeof(_lib.SweepIO) == 7 * 8 + 32 * 8 + 4 * 4 + 2 * 8
    assert _lib.SweepIO.factors.offset == 56 and _lib.SweepIO.wave.offset == 56 + 256 + 16


def test_existing_layouts_and_op_names_keep_their_places(lib):
    """svcmi_synth_io keeps its layout; the new op rows come after every existing one."""
    from svcmi import _lib
    sizes = (ctypes.c_int64 * 8)()
    assert lib.svcmi_struct_sizes(sizes, 8) == 7 and sizes[3] == ctypes.sizeof(_lib.SynthIO) == 7 * 8 + 8 + 6 * 4 + 3 * 8
    names = []
    while lib.svcmi_trace_op_name(len(names)):
        names.append(lib.svcmi_trace_op_name(len(names)).decode())
    assert names[-2:] == ["svcmi_sweep_pitch_f32", "svcmi_sweep_embed_f32"]
    assert names[17] == "svcmi_embed_pitch_f32" and names[len(names) - 3] == "svcmi_yin_aperiodicity_f64"


class Buffers:
    """One host buffer filled with a pattern: every pointer the entry points get aims into it, and it must come back untouched."""

    def __init__(self, nbytes):
        self.raw = (ctypes.c_ubyte * (nbytes + 512))()
        ctypes.memset(self.raw, FILL, len(self.raw))
        self.p = (ctypes.addressof(self.raw) + 255) & ~255

    def untouched(self):
        return bytes(self.raw) == bytes([FILL]) * len(self.raw)


def test_kernel_entry_points_validate_without_a_gpu(lib):
    buf = Buffers(1 << 16)
    p = buf.p
    sp, se = lib.svcmi_sweep_pitch_f32, lib.svcmi_sweep_embed_f32
    fac = (ctypes.c_double * 40)(*([1.0] * 40))
    f = ctypes.addressof(fac)
    # null pointers, sizes
    for hole in range(3):
        a = [p, f, p]
        a[hole] = None
        assert sp(a[0], a[1], a[2], 3, 5, None) == EINVAL, hole
    assert sp(p, f, p, 0, 5, None) == EINVAL and sp(p, f, p, 3, 0, None) == EINVAL and sp(p, f, p, -1, 5, None) == EINVAL
    assert sp(p, f, p, 33, 5, None) == EUNSUPPORTED
    assert sp(p + 2, f, p, 3, 5, None) == EALIGN and sp(p, f + 4, p, 3, 5, None) == EALIGN and sp(p, f, p + 1, 3, 5, None) == EALIGN
    call = lambda xs=p, ldxs=8, pk=p, emb=p, ln=p, x=p, ldx=8, K=3, t=5, c=8: se(xs, ldxs, pk, emb, ln, x, ldx, K, t, c, None)
    for hole in ("xs", "pk", "emb", "x"):
        assert call(**{hole: None}) == EINVAL, hole
    assert call(K=0) == EINVAL and call(t=0) == EINVAL and call(c=0) == EINVAL and call(ldxs=4) == EINVAL and call(ldx=4) == EINVAL
    assert call(K=33) == EUNSUPPORTED
    assert call(c=6, ldxs=8, ldx=8) == EALIGN and call(ldxs=10) == EALIGN and call(ldx=10) == EALIGN          # H % 4 != 0, row strides
    for arg, off in (("xs", 4), ("x", 8), ("emb", 4), ("pk", 2), ("ln", 2)):
        assert call(**{arg: p + off}) == EALIGN, arg
    assert buf.untouched()


def test_workspace_query_and_stage_validate_without_a_gpu(lib, cmodel):
    from svcmi import _lib
    M = ctypes.byref(cmodel.struct)
    wsb, st = lib.svcmi_synth_sweep_workspace_bytes, lib.svcmi_synth_sweep_fwd
    assert wsb(M, 0, 37, 0) < 0 and wsb(M, 33, 37, 0) < 0 and wsb(M, 3, 0, 0) < 0 and wsb(None, 3, 37, 0) < 0
    assert wsb(M, 0, 37, 0) == EINVAL and wsb(M, 33, 37, 0) == EUNSUPPORTED and wsb(M, 3, 0, 0) == EINVAL
    need1, need3 = wsb(M, 1, 37, 0), wsb(M, 3, 37, 0)
    assert 0 < need1 < need3
    # one key needs what one clip needs through svcmi_synth_infer_fwd, plus its transposed track (the pitch2source share of that query aside)
    assert need1 <= lib.svcmi_synth_workspace_bytes(M, 1, 37, 0) + 1024
    buf = Buffers(4096)
    p = buf.p
    io = _lib.SweepIO()
    io.ppg = io.vec = io.pit = io.spk = io.length = io.source = io.noise = io.wave = p
    io.t, io.n_keys = 37, 3
    io.factors[0] = io.factors[1] = io.factors[2] = 1.0
    big = need3 + 4096
    assert st(M, ctypes.byref(io), p, need3 - 1, None) == EINVAL                  # a short workspace
    assert st(M, ctypes.byref(io), p, 0, None) == EINVAL
    assert st(None, ctypes.byref(io), p, big, None) == EINVAL and st(M, None, p, big, None) == EINVAL and st(M, ctypes.byref(io), None, big, None) == EINVAL
    assert st(M, ctypes.byref(io), p + 16, big, None) == EINVAL                   # the workspace wants 256-byte alignment
    for hole in ("ppg", "vec", "pit", "spk", "length", "source", "noise", "wave"):
        bad = _lib.SweepIO.from_buffer_copy(io)
        setattr(bad, hole, None)
        assert st(M, ctypes.byref(bad), p, big, None) == EINVAL, hole
    for k, want in ((0, EINVAL), (33, EUNSUPPORTED), (-2, EINVAL)):
        bad = _lib.SweepIO.from_buffer_copy(io)
        bad.n_keys = k
        assert st(M, ctypes.byref(bad), p, big, None) == want, k
    bad = _lib.SweepIO.from_buffer_copy(io)
    bad.t = 0
    assert st(M, ctypes.byref(bad), p, big, None) == EINVAL
    assert buf.untouched()


def test_emulator_stage_refuses_a_short_workspace(cmodel):
    """The same refusal through the library that can launch: nothing is written."""
    from svcmi import _lib
    from tests.emu import emu_ops
    lib = emu_ops().lib
    M = ctypes.byref(cmodel.struct)
    need = lib.svcmi_synth_sweep_workspace_bytes(M, 2, 5, 0)
    assert need > 0
    small = torch.full((need + 512,), FILL, dtype=torch.uint8)
    base = (small.data_ptr() + 255) & ~255
    io = _lib.SweepIO()
    io.ppg = io.vec = io.pit = io.spk = io.length = io.source = io.noise = io.wave = base
    io.t, io.n_keys = 5, 2
    assert lib.svcmi_synth_sweep_fwd(M, ctypes.byref(io), base, need - 1, 0) == EINVAL
    assert bool((small == FILL).all())
