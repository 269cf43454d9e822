"""Thin tensor-level wrappers over the C ABI (include/svcmi.h).

PyTorch is used for device memory and streams only.  Activations are time-major fp32 tensors
``[B, T, C]`` (contiguous, ``C % 4 == 0``); see DESIGN.md for the layout rationale.  Every method
launches one kernel on the current stream and returns its output tensor.
"""
import contextlib
import ctypes
import os
import threading

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_MISH, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, CONV_ACCUMULATE, CONV_MASK_IN,  # noqa: F401
                   CONV_MASK_OUT, CONV_PARTIALS, PREC_BF16, PREC_BF16X3, PREC_F16, PREC_F32, PRECISIONS, ConvDesc, SnakeConvDesc, SvcmiError,
                   SynthIO, TraceRecord)


SPLIT16 = "bf16x3"      # ``out16`` value: rows [hi: Cp bf16 | lo: Cp bf16], hi = bf16(v), lo = bf16(v - hi), Cp = C rounded up to 8


def _fmt16(dtype):
    """torch.bfloat16 / torch.float16 / SPLIT16 -> the svcmi_precision code of a 16-bit output copy."""
    return {torch.bfloat16: PREC_BF16, torch.float16: PREC_F16, SPLIT16: PREC_BF16X3}[dtype]


def _alloc16(lead, c, out16, device):
    """The 16-bit second output of a producer: [*lead, c] in the 16-bit dtype, or the split layout [*lead, 2*Cp] (zero-filled pads)."""
    if out16 == SPLIT16:
        cp = (c + 7) // 8 * 8
        return (torch.zeros if cp != c else torch.empty)(*lead, 2 * cp, dtype=torch.bfloat16, device=device)
    return torch.empty(*lead, c, dtype=out16, device=device)


def split16_to_f32(x16, c):
    """hi + lo of a SPLIT16 tensor as fp32 [..., c] (tests, debugging)."""
    cp = x16.shape[-1] // 2
    return x16[..., :c].float() + x16[..., cp:cp + c].float()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class Ops:
    """Bound to one loaded library.  ``Ops()`` loads the hipcc-built libsvcmi.so and requires CUDA(HIP)
    tensors; there is no CPU path in the product (tests/emu builds a separate emulation library from the
    same kernel source and passes it in explicitly)."""

    def __init__(self, lib=None):
        # streams that should overlap (clips / chunks in flight, lanes.py) each need their own hardware queue; the runtime reads
        # this when HIP initialises, so it only helps if no HIP call was made yet (the CLIs set it first thing)
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
        self.lib = lib if lib is not None else _lib.load_library()
        self.build = self.lib.svcmi_build_info().decode()
        self.on_gpu = self.build.startswith("hip")
        if self.on_gpu and not torch.cuda.is_available():
            raise SvcmiError("libsvcmi.so is the gfx950 build but no GPU is visible; svcmi has no CPU fallback")
        self.launches = 0
        self.workspaces = {}     # split-K scratch, one per (device, stream): launches on parallel streams must not share it
        self.workspace_floats = 16 * 1024 * 1024
        self._retired = []
        self._graph_pinned = set()        # workspace keys a HIP graph capture has recorded pointers into: their outgrown buffers are kept
        # split-K slices combined inside the GEMM launch by the last-arriving block of each tile.  Correct (bit-identical to
        # the two-kernel reduction, tests/test_gpu_kernels.py) but SLOWER on MI355X at these slab sizes (64-128 KB per tile):
        # 10 s step 15.8 ms (write-through slabs) / 16.1 ms (release fence per block) vs 12.6 ms -> off by default.
        self.inlaunch_reduce = False
        self.timeline = None     # set to a list to record (kernel, work, start_event, end_event) per launch
        # GEMM operand precision (include/svcmi.h: enum svcmi_precision).  fp32 is the parity default; "bf16x3" / "bf16" /
        # "f16" route every eligible convolution through svcmi_conv_gemm_lp with a 16-bit weight image packed on first use
        # (cached on the fp32 weight tensor).  Launches below `lp_min_flops` stay fp32: a GEMM of < ~1.5 GFLOP is latency-bound
        # on this chip (8-17 us whatever the operand type; measured: the 75 small prior / flow GEMMs of a 10 s clip cost the same
        # 1.35 ms through either kernel), so rounding its operands buys nothing and costs accuracy.  At batch 16 the same
        # layers are 16x the work and cross the threshold.
        self._tls = threading.local()          # `precision` is per calling thread (worker threads of the folder driver share one Ops)
        self._lock = threading.RLock()         # guards the lazily built per-tensor 16-bit weight images; re-entrant: ClipLanes.capture holds it around a capture whose warm-up may build them
        self.lp_min_flops = 1.5e9
        # development knobs of the library (svcmi_tune_set: tile variants, fused / unfused paths).  Tile / split / launch-shape knobs
        # leave every result bit-identical; two select another KERNEL FORM of the narrow generator stages and change the fp32
        # summation order (<= 5e-6 on the waveform) or the operand precision: amp_mfma (fp32 matrix-core half-step at 20 channels and
        # batch <= 2 -- so fp32 bits are reproducible per batch class, <= 2 clips vs more), amp_lp (fp16 operands).
        # SVCMI_TUNE="amp_mfma=0,ring2=15" applies them to this process (A/B runs of bench.py on the GPU box)
        self.tune = {}                         # what SVCMI_TUNE set for this process (a scoped change restores to these, not to the defaults)
        for item in filter(None, os.environ.get("SVCMI_TUNE", "").split(",")):
            k, _, v = item.partition("=")
            if self.lib.svcmi_tune_set(k.strip().encode(), int(v)) != 0:
                raise SvcmiError(f"SVCMI_TUNE: unknown knob or value {item!r}")
            self.tune[k.strip()] = int(v)

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return torch.cuda.current_stream().cuda_stream if self.on_gpu else 0

    def _chk(self, *tensors):
        for t in tensors:
            if t is None:
                continue
            if t.is_cuda != self.on_gpu:
                raise SvcmiError(f"tensor on {t.device} but library build is {self.build}")

    def _call(self, name, *args, work=None):
        if self.timeline is not None and self.on_gpu:
            # HIP events on the SAME stream the kernel is launched on (bench.py roofline leg)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = getattr(self.lib, name)(*args)
            e1.record()
            self.timeline.append((name, work or {}, e0, e1))
        else:
            rc = getattr(self.lib, name)(*args)
        self.launches += 1
        if rc != 0:
            raise SvcmiError(f"{name} failed with code {rc}")

    # ------------------------------------------------------------------ reduced precision
    @property
    def precision(self):
        return getattr(self._tls, "precision", PREC_F32)

    @precision.setter
    def precision(self, value):
        self._tls.precision = value

    def set_precision(self, precision):
        if precision not in PRECISIONS and precision not in PRECISIONS.values():
            raise SvcmiError(f"unknown precision {precision!r}; one of {sorted(k for k in PRECISIONS if k)}")
        self.precision = PRECISIONS.get(precision, precision)

    @contextlib.contextmanager
    def use_precision(self, precision):
        """``with ops.use_precision("bf16x3"): ...`` -- None leaves the current setting untouched."""
        old = self.precision
        if precision is not None:
            self.set_precision(precision)
        try:
            yield self
        finally:
            self.precision = old

    def lp_weight(self, w, prec):
        """16-bit image of the packed fp32 operand ``w`` [n, ldw] (svcmi_pack_weights_lp), made once per (tensor, precision)."""
        cache = w.__dict__.setdefault("_svcmi_lp", {})
        img = cache.get(prec)
        if img is None:
            with self._lock:
                img = cache.get(prec)
                if img is None:
                    n, ldw = w.shape
                    ldw16 = (ldw + 31) // 32 * 32
                    img = torch.empty(n, (2 if prec in (PREC_BF16X3, _lib.PREC_BF16X3_A16, _lib.PREC_F16W2_A16) else 1) * ldw16, dtype=torch.int16, device=w.device)
                    self._call("svcmi_pack_weights_lp", _ptr(w), n, ldw, prec, _ptr(img), ldw16, self._stream())
                    if self.on_gpu:            # packed on THIS thread's stream; other streams may read it right away
                        torch.cuda.current_stream().synchronize()
                    cache[prec] = img
        return img

    def _lp_eligible(self, d, w, work):
        """The reduced-precision kernels take 16-byte gathers only (c_in, ldx, batch stride % 4, aligned x)."""
        return (self.precision != PREC_F32 and work["flops"] >= self.lp_min_flops and w.dim() == 2 and w.is_contiguous()
                and d.c_in % 4 == 0 and d.ldx % 4 == 0 and d.x_bstride % 4 == 0 and (d.x or 0) % 16 == 0
                and (not d.x_row_shift or d.c_in % 32 == 0) and (d.flags >> 8) in (0, 1, 3, 4, 6, 9))

    def _to_lp(self, d, w, work):
        prec = PREC_F16 if self.precision == _lib.PREC_F16W2 else self.precision        # f16w2 without 16-bit activations = plain fp16
        img = self.lp_weight(w, prec)
        d.w, d.ldw = img.data_ptr(), img.shape[1] // (2 if prec == PREC_BF16X3 else 1)
        work["bytes"] += d.n_out * d.ksize * d.c_in * (4.0 if prec == PREC_BF16X3 else 2.0) - 4.0 * d.n_out * d.ksize * d.c_in
        return prec

    def empty(self, *shape, like=None, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=like.device if like is not None else ("cuda" if self.on_gpu else "cpu"))


    # ------------------------------------------------------------------ stage-level entry points (csrc/host_stages.hip)
    def stage_workspace(self, nbytes, device):
        """The caller-owned workspace of the stage entry points: one buffer per (device, stream), grown on demand.  Stages issued on one
        stream run one after the other, so they can share it; lanes / chunk streams each get their own."""
        key = (device, self._stream(), "stage")
        ws = self.workspaces.get(key)
        capturing = self.on_gpu and torch.cuda.is_current_stream_capturing()
        if ws is None or ws.numel() < nbytes + 256:
            grow = int(nbytes) + 512
            if ws is not None:
                # geometric growth: a run whose clip lengths keep setting new maxima re-allocates O(log) times, not per clip.  The
                # outgrown buffer is kept only if a HIP graph captured on this stream recorded pointers into it; otherwise it goes
                # back to torch's allocator, which is stream-ordered: kernels already queued on this stream finish before any reuse.
                grow = max(grow, ws.numel() + ws.numel() // 2)
                if key in self._graph_pinned or capturing:
                    self._retired.append(ws)
            ws = self.workspaces[key] = torch.empty(grow, dtype=torch.uint8, device=device)
        if capturing:
            self._graph_pinned.add(key)
        base = (ws.data_ptr() + 255) & ~255            # the entry points want 256-byte alignment (CPU tensors of the emulator tests: 64)
        return base, ws.numel() - (base - ws.data_ptr())

    def release_retired(self):
        """Drop the outgrown stage workspaces kept for captured graphs (call after the graphs that may point into them are gone)."""
        self._retired.clear()

    def _stage_call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        self.launches += 1
        if rc != 0:
            raise SvcmiError(f"{name} failed with code {rc}")

    def whisper_encoder_fwd(self, cm, mel, noise, noise_scale):
        """AudioEncoder.forward (whisper/model.py:147-163) as ONE call: mel [B, n_mels, n] (+ noise_scale * noise) -> [B, tw, n_state]."""
        self._chk(mel, noise)
        m = cm.struct
        m.lp_min_flops = max(float(self.lp_min_flops), 1e-30)
        B, _, n = mel.shape
        need = self.lib.svcmi_whisper_workspace_bytes(ctypes.byref(m), B, n)
        if need < 0:
            if (n - 1) // 2 + 1 > m.n_ctx:
                raise AssertionError("incorrect audio shape")                           # whisper/model.py:156
            raise SvcmiError(f"svcmi_whisper_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, mel.device)
        out = torch.empty(B, (n - 1) // 2 + 1, m.n_state, dtype=torch.float32, device=mel.device)
        self._stage_call("svcmi_whisper_encoder_fwd", ctypes.byref(m), _ptr(mel), _ptr(noise), float(noise_scale), B, n, _ptr(out), ws,
                         ws_bytes, self._stream())
        return out

    def pitch2source_fwd(self, cm, f0, rand_ini, noise):
        """Generator.pitch2source (vits_decoder/generator.py:160-165): f0 [B,T], rand_ini [B,11], noise [B,T*hop,11] -> [B, T*hop]."""
        self._chk(f0, rand_ini, noise)
        m = cm.struct
        B, T = f0.shape
        ws, ws_bytes = self.stage_workspace(B * T * 11 * 8 + 256, f0.device)
        out = torch.empty(B, T * m.hop, dtype=torch.float32, device=f0.device)
        self._stage_call("svcmi_pitch2source_fwd", ctypes.byref(m), _ptr(f0), _ptr(rand_ini), _ptr(noise), B, T, _ptr(out), ws,
                         ws_bytes, self._stream())
        return out

    def synth_infer_fwd(self, cm, ppg, vec, pit, spk, lengths, source, noise, *, ppg_row_shift=0, stream_frames=0, stop_after=0,
                        want_parts=False):
        """SynthesizerInfer.inference (vits/models.py:251-256) as ONE call.  ppg [B, T >> shift, ppg_dim] (a batch-strided view is fine),
        vec [B,T,vec_dim], pit [B,T], spk [B,spk_dim], lengths int32 [B], source [B, T*hop], noise [B, inter, T] -> wave [B, 1, T*hop]
        (+ time-major z_p / z [B,T,inter] with ``want_parts``)."""
        self._chk(ppg, vec, pit, spk, lengths, source, noise)
        m = cm.struct
        m.lp_min_flops = max(float(self.lp_min_flops), 1e-30)
        B, T = pit.shape
        if ppg.stride(2) != 1 or ppg.stride(1) != ppg.shape[2] or ppg.shape[1] != (T + (1 << ppg_row_shift) - 1) >> ppg_row_shift:
            raise SvcmiError(f"ppg {tuple(ppg.shape)} / strides {ppg.stride()} do not fit {T} frames with row shift {ppg_row_shift}")
        for t_, shape in ((vec, (B, T, m.vec_dim)), (spk, (B, m.spk_dim)), (source, (B, T * m.hop)), (noise, (B, m.inter, T))):
            if tuple(t_.shape) != shape or not t_.is_contiguous():
                raise SvcmiError(f"expected a contiguous tensor of shape {shape}, got {tuple(t_.shape)}")
        need = self.lib.svcmi_synth_workspace_bytes(ctypes.byref(m), B, T, int(stream_frames))
        if need < 0:
            raise SvcmiError(f"svcmi_synth_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, pit.device)
        io = SynthIO()
        io.ppg, io.vec, io.pit, io.spk, io.lengths, io.source, io.noise = (_ptr(t_) for t_ in (ppg, vec, pit, spk, lengths, source, noise))
        io.ppg_bstride, io.ppg_row_shift, io.batch, io.t = ppg.stride(0), ppg_row_shift, B, T
        io.stream_frames, io.stop_after = int(stream_frames), int(stop_after)
        wave = torch.empty(B, 1, T * m.hop, dtype=torch.float32, device=pit.device)
        parts = None
        if want_parts:
            parts = (torch.empty(B, T, m.inter, dtype=torch.float32, device=pit.device), torch.empty(B, T, m.inter, dtype=torch.float32, device=pit.device))
            io.z_p, io.z = _ptr(parts[0]), _ptr(parts[1])
        io.wave = _ptr(wave)
        self._stage_call("svcmi_synth_infer_fwd", ctypes.byref(m), ctypes.byref(io), ws, ws_bytes, self._stream())
        return (wave, parts) if want_parts else wave

    def synth_stages_fwd(self, cm, ppg, vec, pit, spk, lengths, source, noise, *, ppg_row_shift=0, stream_frames=0, flow_in=None,
                         gen_in=None):
        """The same forward pass as ``synth_infer_fwd`` through the three per-stage entry points (svcmi_text_encoder_fwd ->
        svcmi_flow_reverse_fwd -> svcmi_generator_fwd), for callers that want the intermediate tensors.  Returns (wave, z_p, z);
        z_p / z time-major [B, T, inter].  ``flow_in`` / ``gen_in`` (time-major [B, T, inter]): start the flow / the generator from
        this tensor instead of the previous stage's output (stage-by-stage parity tests)."""
        self._chk(ppg, vec, pit, spk, lengths, source, noise, flow_in, gen_in)
        m = cm.struct
        m.lp_min_flops = max(float(self.lp_min_flops), 1e-30)
        B, T = pit.shape
        for t_ in (flow_in, gen_in):
            if t_ is not None and (tuple(t_.shape) != (B, T, m.inter) or not t_.is_contiguous() or t_.dtype != torch.float32):
                raise SvcmiError(f"expected a contiguous fp32 stage input of shape {(B, T, m.inter)}, got {tuple(t_.shape)}")
        need = self.lib.svcmi_synth_workspace_bytes(ctypes.byref(m), B, T, int(stream_frames))
        if need < 0:
            raise SvcmiError(f"svcmi_synth_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, pit.device)
        io = SynthIO()
        io.ppg, io.vec, io.pit, io.spk, io.lengths, io.source, io.noise = (_ptr(t_) for t_ in (ppg, vec, pit, spk, lengths, source, noise))
        io.ppg_bstride, io.ppg_row_shift, io.batch, io.t, io.stream_frames = ppg.stride(0), ppg_row_shift, B, T, int(stream_frames)
        wave = torch.empty(B, 1, T * m.hop, dtype=torch.float32, device=pit.device)
        io.wave = _ptr(wave)
        z_p = torch.empty(B, T, m.inter, dtype=torch.float32, device=pit.device)
        self._stage_call("svcmi_text_encoder_fwd", ctypes.byref(m), ctypes.byref(io), _ptr(z_p), ws, ws_bytes, self._stream())
        z = (z_p if flow_in is None else flow_in).clone()           # the flow runs in place
        self._stage_call("svcmi_flow_reverse_fwd", ctypes.byref(m), ctypes.byref(io), _ptr(z), ws, ws_bytes, self._stream())
        self._stage_call("svcmi_generator_fwd", ctypes.byref(m), ctypes.byref(io), _ptr(z if gen_in is None else gen_in), ws, ws_bytes,
                         self._stream())
        return wave, z_p, z

    # ------------------------------------------------------------------ key sweep (csrc/sweep.hip, svcmi_synth_sweep_fwd)
    @staticmethod
    def _factors(factors):
        """The transposition factors as the C array the entry points read (host memory, doubles)."""
        f = [float(v) for v in factors]
        if not f:
            raise SvcmiError("a key sweep needs at least one factor")
        return (ctypes.c_double * len(f))(*f), len(f)

    def sweep_pitch(self, pit, factors):
        """pit [T] Hz, factors: K Python floats (2 ** (shift / 12)) -> pit_k [K, T] = float32(float64(pit) * factor): the reference's
        ``np.array(pit) * 2 ** (shift / 12)`` followed by ``torch.FloatTensor``."""
        self._chk(pit)
        fac, K = self._factors(factors)
        if pit.dim() != 1 or pit.dtype != torch.float32 or not pit.is_contiguous():
            raise SvcmiError(f"expected a contiguous fp32 pitch track [T], got {tuple(pit.shape)} {pit.dtype}")
        out = torch.empty(K, pit.shape[0], dtype=torch.float32, device=pit.device)
        self._call("svcmi_sweep_pitch_f32", _ptr(pit), ctypes.addressof(fac), _ptr(out), K, pit.shape[0], self._stream())
        return out

    def sweep_embed(self, xs, pit_k, emb, length):
        """xs [T, C] (the masked sum of the two front convolutions), pit_k [K, T], emb [256, C], length int32 [1] (or None) ->
        x [K, T, C] = (xs + emb[f0_to_coarse(pit_k)]) * mask, the arithmetic of ``embed_pitch`` on K copies of xs."""
        self._chk(xs, pit_k, emb, length)
        K, T = pit_k.shape
        C = xs.shape[1]
        if tuple(xs.shape) != (T, C) or xs.stride(1) != 1 or not pit_k.is_contiguous() or tuple(emb.shape) != (256, C) or not emb.is_contiguous():
            raise SvcmiError(f"sweep_embed: xs {tuple(xs.shape)}, pit_k {tuple(pit_k.shape)}, emb {tuple(emb.shape)} do not fit")
        x = torch.empty(K, T, C, dtype=torch.float32, device=xs.device)
        self._call("svcmi_sweep_embed_f32", _ptr(xs), xs.stride(0), _ptr(pit_k), _ptr(emb), _ptr(length), _ptr(x), C, K, T, C, self._stream())
        return x

    def synth_sweep_workspace_bytes(self, cm, n_keys, t, stream_frames=0):
        return int(self.lib.svcmi_synth_sweep_workspace_bytes(ctypes.byref(cm.struct), int(n_keys), int(t), int(stream_frames)))

    def synth_sweep_fwd(self, cm, ppg, vec, pit, spk, length, sources, noise, factors, *, ppg_row_shift=0, stream_frames=0, want_pit=False):
        """One chunk at K transpositions as ONE call (svcmi_synth_sweep_fwd).  Batch-1 inputs: ppg [T >> shift, ppg_dim], vec [T, vec_dim],
        pit [T], spk [spk_dim], length int32 [1]; per key: sources [K, T*hop], noise [K, inter, T], factors (K floats)
        -> wave [K, 1, T*hop] (+ pit_k [K, T] with ``want_pit``)."""
        self._chk(ppg, vec, pit, spk, length, sources, noise)
        m = cm.struct
        m.lp_min_flops = max(float(self.lp_min_flops), 1e-30)
        fac, K = self._factors(factors)
        T = pit.shape[0]
        if K > _lib.SWEEP_MAX_KEYS:
            raise SvcmiError(f"a key sweep takes at most {_lib.SWEEP_MAX_KEYS} keys per call, got {K}")
        for t_, shape in ((ppg, ((T + (1 << ppg_row_shift) - 1) >> ppg_row_shift, m.ppg_dim)), (vec, (T, m.vec_dim)), (pit, (T,)), (spk, (m.spk_dim,)),
                          (length, (1,)), (sources, (K, T * m.hop)), (noise, (K, m.inter, T))):
            if tuple(t_.shape) != shape or not t_.is_contiguous():
                raise SvcmiError(f"expected a contiguous tensor of shape {shape}, got {tuple(t_.shape)}")
        need = self.lib.svcmi_synth_sweep_workspace_bytes(ctypes.byref(m), K, T, int(stream_frames))
        if need < 0:
            raise SvcmiError(f"svcmi_synth_sweep_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, pit.device)
        io = _lib.SweepIO()
        io.ppg, io.vec, io.pit, io.spk, io.length, io.source, io.noise = (_ptr(t_) for t_ in (ppg, vec, pit, spk, length, sources, noise))
        for i in range(K):
            io.factors[i] = fac[i]
        io.ppg_row_shift, io.t, io.n_keys, io.stream_frames = int(ppg_row_shift), T, K, int(stream_frames)
        wave = torch.empty(K, 1, T * m.hop, dtype=torch.float32, device=pit.device)
        pit_k = torch.empty(K, T, dtype=torch.float32, device=pit.device) if want_pit else None
        io.wave, io.pit_k = _ptr(wave), _ptr(pit_k)
        self._stage_call("svcmi_synth_sweep_fwd", ctypes.byref(m), ctypes.byref(io), ws, ws_bytes, self._stream())
        return (wave, pit_k) if want_pit else wave

    # ------------------------------------------------------------------ singer sweep (csrc/sweep.hip, svcmi_synth_singers_fwd)
    def sweep_sample_prior(self, stats, noise, length):
        """stats [T, >= 2*I] (m | logs of ONE clip, a row-strided view is fine), noise [S, I, T] (the reference's randn_like(m) layout),
        length int32 [1] (or None) -> z [S, T, I] = (m + noise * exp(logs)) * mask: the bits of ``sample_prior`` on S copies of stats."""
        self._chk(stats, noise, length)
        if noise.dim() != 3 or stats.dim() != 2:
            raise SvcmiError(f"sweep_sample_prior: stats {tuple(stats.shape)}, noise {tuple(noise.shape)} do not fit")
        S, I, T = noise.shape
        if stats.shape[0] != T or stats.shape[1] < 2 * I or stats.stride(1) != 1 or not noise.is_contiguous():
            raise SvcmiError(f"sweep_sample_prior: stats {tuple(stats.shape)}, noise {tuple(noise.shape)} do not fit")
        if S > _lib.SINGERS_MAX:
            raise SvcmiError(f"a singer sweep takes at most {_lib.SINGERS_MAX} singers per call, got {S}")
        z = torch.empty(S, T, I, dtype=torch.float32, device=stats.device)
        self._call("svcmi_sweep_sample_prior_f32", _ptr(stats), stats.stride(0), _ptr(noise), _ptr(length), _ptr(z), I, S, T, I, self._stream())
        return z

    def synth_singers_workspace_bytes(self, cm, n_singers, t, stream_frames=0):
        return int(self.lib.svcmi_synth_singers_workspace_bytes(ctypes.byref(cm.struct), int(n_singers), int(t), int(stream_frames)))

    def synth_singers_fwd(self, cm, ppg, vec, pit, spks, length, source, noise, *, ppg_row_shift=0, stream_frames=0, want_parts=False):
        """One chunk in S timbres as ONE call (svcmi_synth_singers_fwd).  Batch-1 inputs: ppg [T >> shift, ppg_dim], vec [T, vec_dim],
        pit [T], length int32 [1], source [T*hop] (ONE harmonic source for all singers); per singer: spks [S, spk_dim],
        noise [S, inter, T] -> wave [S, 1, T*hop] (+ time-major z_p [S, T, inter] with ``want_parts``)."""
        self._chk(ppg, vec, pit, spks, length, source, noise)
        m = cm.struct
        m.lp_min_flops = max(float(self.lp_min_flops), 1e-30)
        T = pit.shape[0]
        S = spks.shape[0] if spks.dim() == 2 else 0
        if not 1 <= S <= _lib.SINGERS_MAX:
            raise SvcmiError(f"a singer sweep takes 1..{_lib.SINGERS_MAX} speaker rows per call, got {tuple(spks.shape)}")
        for t_, shape in ((ppg, ((T + (1 << ppg_row_shift) - 1) >> ppg_row_shift, m.ppg_dim)), (vec, (T, m.vec_dim)), (pit, (T,)), (spks, (S, m.spk_dim)),
                          (length, (1,)), (source, (T * m.hop,)), (noise, (S, m.inter, T))):
            if tuple(t_.shape) != shape or not t_.is_contiguous():
                raise SvcmiError(f"expected a contiguous tensor of shape {shape}, got {tuple(t_.shape)}")
        need = self.lib.svcmi_synth_singers_workspace_bytes(ctypes.byref(m), S, T, int(stream_frames))
        if need < 0:
            raise SvcmiError(f"svcmi_synth_singers_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, pit.device)
        io = _lib.SingersIO()
        io.ppg, io.vec, io.pit, io.length, io.source, io.spk, io.noise = (_ptr(t_) for t_ in (ppg, vec, pit, length, source, spks, noise))
        io.ppg_row_shift, io.t, io.n_singers, io.stream_frames = int(ppg_row_shift), T, S, int(stream_frames)
        wave = torch.empty(S, 1, T * m.hop, dtype=torch.float32, device=pit.device)
        z_p = torch.empty(S, T, m.inter, dtype=torch.float32, device=pit.device) if want_parts else None
        io.wave, io.z_p = _ptr(wave), _ptr(z_p)
        self._stage_call("svcmi_synth_singers_fwd", ctypes.byref(m), ctypes.byref(io), ws, ws_bytes, self._stream())
        return (wave, z_p) if want_parts else wave

    def trace_begin(self, max_records=8192):
        """Per-launch timing of everything launched from here on (stage entry points: HIP events inside the C host; single-op calls of
        this class: torch events): bench.py's roofline leg."""
        self.timeline = []
        if self.lib.svcmi_trace_begin(max_records) != 0:
            raise SvcmiError("svcmi_trace_begin failed")

    def trace_end(self):
        """-> {entry point: {launches, ms, flops, bytes}} since trace_begin (waits for the traced launches)."""
        recs = (TraceRecord * 8192)()
        n = min(self.lib.svcmi_trace_end(recs, 8192), 8192)
        tl, self.timeline = self.timeline or [], None
        agg = {}

        def add(name, ms, flops, nbytes, a16=False, prec=0):
            a = agg.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "a16_launches": 0, "precisions": []})
            if prec and prec not in a["precisions"]:
                a["precisions"].append(prec)                   # enum svcmi_precision codes the reduced-precision launches of this op ran in
            a["launches"] += 1
            a["ms"] += ms
            a["flops"] += flops
            a["bytes"] += nbytes
            a["a16_launches"] += int(a16)         # GEMM launches that took 16-bit activations (SVCMI_PREC_*_A16)
        for i in range(n):
            add(self.lib.svcmi_trace_op_name(recs[i].op).decode(), recs[i].ms, recs[i].flops, recs[i].bytes, (recs[i].op >> 8) >= _lib.PREC_BF16_A16,
                recs[i].op >> 8)
        if tl and self.on_gpu:
            torch.cuda.synchronize()
        for name, work, e0, e1 in tl:
            add(name, e0.elapsed_time(e1) if self.on_gpu else 0.0, work.get("flops", 0.0), work.get("bytes", 0.0))
        return agg

    # ------------------------------------------------------------------ conv / linear
    def _conv_desc(self, x, w, bias=None, *, ksize=1, stride=1, dilation=1, pad=0, t_out=None, act=ACT_NONE,
             res=None, alpha=1.0, accumulate=False, lengths=None, mask_in=False, mask_out=False, out=None,
             x_row_shift=0, c_in=None, ldx=None, t_in=None, n_out=None, x_bstride=None, tile=0, split_k=0, partials=False):
        """y[b,t,n] = epilogue(sum_k sum_ci x[b, t*stride + k*dilation - pad, ci] * w[n, k*c_in + ci]).
        ``x`` is [B, T, C]; ``w`` is [N, ldw] packed (weights.pack_conv)."""
        self._chk(x, w, bias, res, out, lengths)
        B = x.shape[0]
        if t_in is None:
            t_in = x.shape[1] << x_row_shift
        if ldx is None:
            ldx = x.shape[2] if x.dim() == 3 else 1
        if c_in is None:
            c_in = ldx
        if x_bstride is None:
            x_bstride = x.stride(0)
        N = w.shape[0] if n_out is None else n_out
        if t_out is None:
            t_out = (t_in + 2 * pad - dilation * (ksize - 1) - 1) // stride + 1
        if out is None and not partials:
            out = torch.empty(B, t_out, N, dtype=torch.float32, device=x.device)
        d = ConvDesc()
        d.x, d.w, d.bias, d.res, d.y, d.lengths = _ptr(x), _ptr(w), _ptr(bias), _ptr(res), _ptr(out if out is not None else x), _ptr(lengths)
        d.x_bstride, d.y_bstride = x_bstride, (out.stride(0) if out is not None else 0)
        d.res_bstride = res.stride(0) if (res is not None and res.dim() == 3) else 0   # 2-D res is shared by the batch
        d.batch, d.t_in, d.t_out, d.c_in, d.ldx = B, t_in, t_out, c_in, ldx
        d.n_out, d.ldw, d.ldy = N, w.shape[1], (out.stride(1) if out is not None else N)
        d.ldr = res.stride(-2) if res is not None else 0
        d.ksize, d.stride, d.dilation, d.pad, d.x_row_shift = ksize, stride, dilation, pad, x_row_shift
        d.act = act
        d.flags = (CONV_ACCUMULATE if accumulate else 0) | (CONV_MASK_IN if mask_in else 0) | (CONV_MASK_OUT if mask_out else 0) | \
                  (CONV_PARTIALS if partials else 0) | (tile << 8)
        d.alpha = alpha
        if split_k != 1 or partials:
            key = (x.device, self._stream())
            ws = self.workspaces.get(key)
            need = max(self.workspace_floats, B * max(split_k, 1) * t_out * N if partials else 0)
            if ws is None or ws[0].numel() < need:     # slabs + zeroed per-tile arrival counters (the library keeps them zero)
                ws = self.workspaces[key] = (torch.empty(need, dtype=torch.float32, device=x.device),
                                             torch.zeros(65536, dtype=torch.int32, device=x.device))
            d.split_k, d.workspace, d.workspace_floats = split_k, ws[0].data_ptr(), ws[0].numel()
            if self.inlaunch_reduce and not partials:
                d.counters, d.counters_len = ws[1].data_ptr(), ws[1].numel()
        else:
            d.split_k, d.workspace, d.workspace_floats = 1, 0, 0
        # algorithmic work: every operand element once (input rows, the weight matrix, the output (+ residual / accumulate))
        nbytes = 4.0 * (B * (t_in >> x_row_shift) * c_in + N * ksize * c_in + B * t_out * N * (1 + (res is not None) + bool(accumulate)))
        return d, out, (ws if (split_k != 1 or partials) else None), B, t_out, N, {"flops": 2.0 * B * t_out * N * ksize * c_in, "bytes": nbytes}

    def conv(self, x, w, bias=None, *, x16=None, out16=None, **kw):
        """y[b,t,n] = epilogue(sum_k sum_ci x[b, t*stride + k*dilation - pad, ci] * w[n, k*c_in + ci]).
        ``x`` is [B, T, C]; ``w`` is [N, ldw] packed (weights.pack_conv).  Keywords: see ``_conv_desc``.
        ``x16``: the same activations as a bf16 / float16 tensor written by the producing kernel -- in the matching 16-bit mode the launch
        then takes the _A16 kernel (no in-register rounding).  ``out16`` = torch.bfloat16 | torch.float16: also return that copy of y."""
        d, out, ws, B, t_out, N, work = self._conv_desc(x, w, bias, **kw)
        y16 = None
        if out16 is not None:
            y16 = _alloc16(out.shape[:-1], N, out16, out.device)
            d.y16, d.y16_bstride, d.ldy16, d.y16_format = y16.data_ptr(), y16.stride(0), y16.stride(1), _fmt16(out16)
        if self._lp_eligible(d, w, work):
            prec = self._to_lp(d, w, work)
            # x16 in this mode's format (bf16x3: a SPLIT16 tensor, recognised by its doubled rows)
            if x16 is not None and ((prec == PREC_BF16X3 and x16.dtype == torch.bfloat16 and x16.shape[-1] == 2 * ((d.c_in + 7) // 8 * 8))
                                    or (prec != PREC_BF16X3 and prec == _fmt16(x16.dtype))):
                self._chk(x16)
                prec = {PREC_BF16: _lib.PREC_BF16_A16, PREC_F16: _lib.PREC_F16_A16, PREC_BF16X3: _lib.PREC_BF16X3_A16}[prec]   # natural-order weight image
                if self.precision == _lib.PREC_F16W2:
                    prec = _lib.PREC_F16W2_A16                                     # ... of (hi, lo) fp16 pairs
                img = self.lp_weight(w, prec)
                d.x, d.w, d.ldx, d.x_bstride = x16.data_ptr(), img.data_ptr(), x16.stride(1), x16.stride(0)
            self._call("svcmi_conv_gemm_lp", ctypes.byref(d), prec, self._stream(), work=work)
        else:
            if (d.flags >> 8) & 15 == 9:          # SVCMI_CONV_TILE_64x128 is a reduced-precision tile: on the fp32 kernel the library chooses
                d.flags &= ~0xF00
            self._call("svcmi_conv_gemm_f32", ctypes.byref(d), self._stream(), work=work)
        if kw.get("partials"):      # [B, split, t_out, N] view of this stream's workspace; valid until the next split-K launch on it
            return ws[0][:B * d.split_k * t_out * N].view(B, d.split_k, t_out, N)
        return out if out16 is None else (out, y16)

    def conv_group(self, problems):
        """Up to 3 convolutions of one geometry in one launch (svcmi_conv_gemm_group_f32).  ``problems``: dicts of ``conv``
        arguments (x, w, bias + keywords; ``out`` required to differ).  Returns the outputs."""
        descs = (ConvDesc * len(problems))()
        outs, works, ws = [], [], []
        for i, pr in enumerate(problems):
            pr = dict(pr)
            w = pr.pop("w")
            d, out, _, _, _, _, wk = self._conv_desc(pr.pop("x"), w, pr.pop("bias", None), split_k=1, **pr)
            descs[i] = d
            outs.append(out)
            works.append(wk)
            ws.append(w)
        total = {"flops": sum(wk["flops"] for wk in works), "bytes": 0.0}
        lp = all(self._lp_eligible(descs[i], ws[i], total) for i in range(len(problems))) and (descs[0].flags >> 8) in (0, 1, 4, 6)
        prec = PREC_F32
        if lp:
            for i in range(len(problems)):
                prec = self._to_lp(descs[i], ws[i], works[i])
        total["bytes"] = sum(wk["bytes"] for wk in works)
        if lp:
            self._call("svcmi_conv_gemm_group_lp", descs, len(problems), prec, self._stream(), work=total)
        else:
            self._call("svcmi_conv_gemm_group_f32", descs, len(problems), self._stream(), work=total)
        return outs

    # ------------------------------------------------------------------ norm / attention
    def layernorm(self, x, gamma=None, beta=None, *, res=None, eps=1e-5, per_batch_affine=False, out=None, out16=None):
        """``out16`` = torch.bfloat16 | torch.float16 | SPLIT16: also return the rows rounded to that format (a following GEMM's 16-bit A operand)."""
        self._chk(x, gamma, beta, res, out)
        B, T, Cc = x.shape
        if out is None:
            out = torch.empty_like(x)
        y16 = _alloc16((B, T), Cc, out16, x.device) if out16 is not None else None
        self._call("svcmi_layernorm_f32", _ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(out), B, T, Cc,
                   x.stride(1), res.stride(1) if res is not None else 0, out.stride(1),
                   (gamma.stride(0) if gamma is not None else beta.stride(0)) if per_batch_affine else 0, eps,
                   _ptr(y16), y16.stride(1) if y16 is not None else 0, _fmt16(out16) if out16 is not None else 0, self._stream())
        return out if out16 is None else (out, y16)

    def channel_norm_gelu(self, x, gamma, beta, eps=1e-5, out=None):
        """GroupNorm(C, C) over time + GELU on time-major x [B, T, C] (hubert/hubert_model.py:78,88)."""
        self._chk(x, gamma, beta, out)
        B, T, Cc = x.shape
        if out is None:
            out = torch.empty_like(x)
        scratch = torch.empty(B * 129 * Cc, dtype=torch.float64, device=x.device)
        self._call("svcmi_channel_norm_gelu_f32", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(scratch), B, T, Cc,
                   x.stride(1), out.stride(1), eps, self._stream())
        return out

    def splitk_layernorm(self, partials, bias, x, gamma, beta, *, eps=1e-5, out=None, out16=None):
        """x += bias + sum_s partials[:, s]  (in place);  returns LayerNorm(x) * gamma + beta.  partials: [B, S, T, C]."""
        self._chk(partials, bias, x, gamma, beta, out)
        B, S, T, Cc = partials.shape
        if out is None:
            out = torch.empty_like(x)
        y16 = _alloc16((B, T), Cc, out16, x.device) if out16 is not None else None
        self._call("svcmi_splitk_layernorm_f32", _ptr(partials), S, _ptr(bias), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(out),
                   B, T, Cc, x.stride(1), out.stride(1), eps, _ptr(y16), y16.stride(1) if y16 is not None else 0,
                   _fmt16(out16) if out16 is not None else 0, self._stream())
        return out if out16 is None else (out, y16)

    def attention(self, qkv, heads, scale, *, rel_k=None, rel_v=None, window=0, lengths=None, out=None, out16=None):
        """qkv: [B, T, 3*C] fused projection (q | k | v).  Returns [B, T, C] (+ its bf16 / float16 copy with ``out16``)."""
        self._chk(qkv, rel_k, rel_v, lengths, out)
        B, T, C3 = qkv.shape
        Cc = C3 // 3
        if out is None:
            out = torch.empty(B, T, Cc, dtype=torch.float32, device=qkv.device)
        base = qkv.data_ptr()
        bs = qkv.stride(0)
        o16 = _alloc16((B, T), Cc, out16, qkv.device) if out16 is not None else None
        self._call("svcmi_attention_f32", base, base + 4 * Cc, base + 8 * Cc, _ptr(out), C3, C3, C3, out.stride(1),
                   bs, bs, bs, out.stride(0), B, T, heads, Cc // heads, scale, _ptr(rel_k), _ptr(rel_v), window,
                   _ptr(lengths), _ptr(o16), o16.stride(1) if o16 is not None else 0, o16.stride(0) if o16 is not None else 0,
                   _fmt16(out16) if out16 is not None else 0, self._stream(),
                   work={"flops": 4.0 * B * T * T * Cc})
        return out if out16 is None else (out, o16)

    def attention16(self, qkv16, heads, scale, *, rel_k=None, rel_v=None, window=0, lengths=None, want_f32=True):
        """qkv16: [B, T, 3*C] bf16 / float16 fused projection (the 16-bit output copy of the QKV GEMM).  Attention on the 16-bit matrix
        cores (svcmi_attention16); returns (o fp32 [B,T,C] or None, o16 [B,T,C] in qkv16's dtype)."""
        self._chk(qkv16, lengths, rel_k, rel_v)
        B, T, C3 = qkv16.shape
        Cc = C3 // 3
        o = torch.empty(B, T, Cc, dtype=torch.float32, device=qkv16.device) if want_f32 else None
        o16 = torch.empty(B, T, Cc, dtype=qkv16.dtype, device=qkv16.device)
        base, esz = qkv16.data_ptr(), 2
        self._call("svcmi_attention16", base, base + esz * Cc, base + 2 * esz * Cc, C3, qkv16.stride(0), _ptr(o), Cc, T * Cc, _ptr(o16), Cc, T * Cc,
                   B, T, heads, Cc // heads, scale, _ptr(rel_k), _ptr(rel_v), window, _ptr(lengths), _fmt16(qkv16.dtype), self._stream(),
                   work={"flops": 4.0 * B * T * T * Cc})
        return o, o16

    # ------------------------------------------------------------------ generator pieces
    def snake_alias(self, x, alpha_log, beta_log, filt, out=None):
        self._chk(x, alpha_log, beta_log, filt, out)
        B, L, Cc = x.shape
        if out is None:
            out = torch.empty_like(x)
        self._call("svcmi_snake_alias_f32", _ptr(x), _ptr(out), _ptr(alpha_log), _ptr(beta_log), _ptr(filt),
                   B, L, Cc, x.stride(1), self._stream(), work={"bytes": 8.0 * B * L * Cc})
        return out

    def snake_alias_group(self, xs, alpha_logs, beta_logs, filt, outs):
        """SnakeAlias of up to 3 same-shape tensors (own alpha / beta each) in one launch."""
        self._chk(*xs, *alpha_logs, *beta_logs, filt, *outs)
        n = len(xs)
        B, L, Cc = xs[0].shape
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        if outs[0].dtype != torch.float32:      # bf16 / float16 outputs: the 16-bit rows a following _A16 GEMM reads
            split = outs[0].dtype == torch.bfloat16 and outs[0].shape[-1] == 2 * xs[0].stride(1)      # SPLIT16 rows [hi: ld | lo: ld]
            self._call("svcmi_snake_alias_group_f32", arr(xs), None, arr(alpha_logs), arr(beta_logs), _ptr(filt), n,
                       B, L, Cc, xs[0].stride(1), arr(outs), _fmt16(SPLIT16 if split else outs[0].dtype), self._stream(),
                       work={"bytes": (8.0 if split else 6.0) * n * B * L * Cc})
            return outs
        self._call("svcmi_snake_alias_group_f32", arr(xs), arr(outs), arr(alpha_logs), arr(beta_logs), _ptr(filt), n,
                   B, L, Cc, xs[0].stride(1), None, 0, self._stream(), work={"bytes": 8.0 * n * B * L * Cc})
        return outs

    def block_mean(self, xs, out=None):
        """((xs[0] + xs[1]) + xs[2]) / len(xs) for contiguous same-shape tensors."""
        self._chk(*xs, out)
        if out is None:
            out = torch.empty_like(xs[0])
        arr = (ctypes.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
        self._call("svcmi_block_mean_f32", arr, len(xs), _ptr(out), xs[0].numel(), self._stream(),
                   work={"bytes": 4.0 * (len(xs) + 1) * xs[0].numel()})
        return out

    def upsample_noise_supported(self, u, cp, cin):
        return bool(self.lib.svcmi_upsample_noise_supported(u, cp, cin))

    def upsample_noise(self, x, up_w, up_b, taps, pad, u, cp, src, nz_w, nz_b, nz_k, nz_stride, nz_pad, y=None):
        """ups[i](x) + noise_convs[i](src) for the narrow stages: x [B, t_in, cin], src [B, L] -> [B, t_in*u, cp].
        With ``y`` given (= ups[i](x) already computed, [B, t_in*u, cp]) only the noise convolution is added."""
        self._chk(x, up_w, up_b, src, nz_w, nz_b, y)
        noise_only = y is not None
        if noise_only:
            B, t_in, cin = y.shape[0], y.shape[1] // u, 4
        else:
            B, t_in, cin = x.shape
            y = torch.empty(B, t_in * u, cp, dtype=torch.float32, device=x.device)
        self._call("svcmi_upsample_noise_f32", 0 if noise_only else _ptr(x), _ptr(up_w), _ptr(up_b), _ptr(src), _ptr(nz_w),
                   _ptr(nz_b), _ptr(y), B, t_in, cin, up_w.shape[1] if up_w is not None else 0, taps, pad, u, cp, src.shape[1],
                   nz_k, nz_stride, nz_pad, nz_w.shape[1], self._stream(), work={"bytes": 4.0 * B * t_in * (cin + u * cp)})
        return y

    def snake_conv_supported(self, c, ld, ksize, dilation):
        return bool(self.lib.svcmi_snake_conv_supported(c, ld, ksize, dilation))

    def snake_conv_preferred(self, c, ld, ksize, dilation):
        return bool(self.lib.svcmi_snake_conv_preferred(c, ld, ksize, dilation))

    def snake_conv(self, x, alpha_log, beta_log, filt, w, bias, *, c, ksize, dilation=1, res=None, alpha=1.0,
                   accumulate=False, out=None):
        """Fused SnakeAlias -> 'same' Conv1d (+ bias + res) * alpha (+= out) for the narrow stages; x [B, L, ld]."""
        self._chk(x, alpha_log, beta_log, filt, w, bias, res, out)
        B, L, ld = x.shape
        if out is None:
            out = torch.empty_like(x)
        self._call("svcmi_snake_conv_f32", _ptr(x), _ptr(w), _ptr(bias), _ptr(res), _ptr(out), _ptr(alpha_log),
                   _ptr(beta_log), _ptr(filt), B, L, c, ld, w.shape[1], ksize, dilation, float(alpha), int(accumulate),
                   self._stream(), work={"flops": 2.0 * B * L * c * c * ksize, "bytes": 8.0 * B * L * c})
        return out

    def snake_post_supported(self, c, ld, ksize):
        return bool(self.lib.svcmi_snake_post_supported(c, ld, ksize))

    def snake_post(self, x, alpha_log, beta_log, filt, w, *, c, ksize):
        """Output layer: tanh(conv_post(SnakeAlias(x))) with one output channel; x [B, L, ld], w [1, >= ksize*ld] -> [B, L]."""
        self._chk(x, alpha_log, beta_log, filt, w)
        B, L, ld = x.shape
        out = torch.empty(B, L, dtype=torch.float32, device=x.device)
        self._call("svcmi_snake_post_f32", _ptr(x), _ptr(w), _ptr(out), _ptr(alpha_log), _ptr(beta_log), _ptr(filt), B, L, c, ld,
                   ksize, self._stream(), work={"flops": 2.0 * B * L * c * ksize, "bytes": 4.0 * B * L * (c + 1)})
        return out

    def snake_conv_group(self, problems, filt, *, c, precision=None):
        """The fused half-step for up to 3 AMP blocks in one launch.  ``problems``: dicts with x, alpha_log, beta_log, w, bias,
        ksize, dilation (1), res (None), alpha (1.0), accumulate (False), out.  ``precision`` "f16" / "f16w2": the convolution on the
        fp16 matrix cores (svcmi_snake_conv_group_lp; same fp32 tensors in and out)."""
        descs = (SnakeConvDesc * len(problems))()
        B, L, ld = problems[0]["x"].shape
        flops = 0.0
        for i, pr in enumerate(problems):
            self._chk(pr["x"], pr["alpha_log"], pr["beta_log"], pr["w"], pr.get("bias"), pr.get("res"), pr["out"])
            d = descs[i]
            d.x, d.w, d.bias, d.res, d.y = _ptr(pr["x"]), _ptr(pr["w"]), _ptr(pr.get("bias")), _ptr(pr.get("res")), _ptr(pr["out"])
            d.alpha_log, d.beta_log = _ptr(pr["alpha_log"]), _ptr(pr["beta_log"])
            d.ldw, d.ksize, d.dilation = pr["w"].shape[1], pr["ksize"], pr.get("dilation", 1)
            d.accumulate, d.alpha = int(pr.get("accumulate", False)), float(pr.get("alpha", 1.0))
            flops += 2.0 * B * L * c * c * pr["ksize"]
        if precision is not None:
            self._call("svcmi_snake_conv_group_lp", descs, len(problems), _ptr(filt), B, L, c, ld, PRECISIONS[precision], self._stream(),
                       work={"flops": flops, "bytes": 8.0 * len(problems) * B * L * c})
        else:
            self._call("svcmi_snake_conv_group_f32", descs, len(problems), _ptr(filt), B, L, c, ld, self._stream(),
                       work={"flops": flops, "bytes": 8.0 * len(problems) * B * L * c})
        return [pr["out"] for pr in problems]

    def pitch2source(self, f0, rand_ini, noise, merge_w, merge_b, hop, sr):
        """f0 [B,T], rand_ini [B,11], noise [B,T*hop,11] -> source [B, T*hop]."""
        self._chk(f0, rand_ini, noise, merge_w)
        B, T = f0.shape
        prefix = torch.empty(B, T, 11, dtype=torch.float64, device=f0.device)
        self._call("svcmi_pitch_prefix_f64", _ptr(f0), _ptr(rand_ini), _ptr(prefix), B, T, hop, float(sr), self._stream())
        out = torch.empty(B, T * hop, dtype=torch.float32, device=f0.device)
        self._call("svcmi_pitch_source_f32", _ptr(f0), _ptr(prefix), _ptr(noise), _ptr(merge_w), float(merge_b),
                   _ptr(out), B, T, hop, float(sr), self._stream())
        return out

    # ------------------------------------------------------------------ whisper log-mel front-end
    def reflect_pad(self, x, pad):
        self._chk(x)
        B, n = x.shape
        y = torch.empty(B, n + 2 * pad, dtype=torch.float32, device=x.device)
        self._call("svcmi_reflect_pad_f32", _ptr(x), _ptr(y), B, n, pad, self._stream())
        return y

    def power_spectrum(self, ri, nbins, half):
        self._chk(ri)
        B, T, ld = ri.shape
        p = torch.empty(B, T, half, dtype=torch.float32, device=ri.device)
        self._call("svcmi_power_spectrum_f32", _ptr(ri), _ptr(p), B * T, nbins, half, ld, half, self._stream())
        return p

    def logmel_finish(self, mel_power):
        self._chk(mel_power)
        B, T, Cc = mel_power.shape
        scratch = torch.empty(B * 64, dtype=torch.float32, device=mel_power.device)
        out = torch.empty(B, Cc, T, dtype=torch.float32, device=mel_power.device)
        self._call("svcmi_logmel_finish_f32", _ptr(mel_power), _ptr(scratch), _ptr(out), B, T, Cc, self._stream())
        return out

    def pcm_resample(self, pcm, fmt, channels, taps, up, down, half):
        """Interleaved PCM frames as a wav file holds them (``pcm``: flat or [frames, channels]; ``fmt`` 0 float32, 1 int16, 2 int32,
        3 uint8) -> mono float32 [ceil(frames * up / down)]: decode, downmix and polyphase resampling in one launch
        (svcmi_pcm_resample_f32).  ``taps``: the packed filter image [up, K] of ``svcmi.whisper.audio.resample_taps`` with its
        ``half``; None (with up == down == 1) decodes and downmixes only."""
        self._chk(pcm, taps)
        pcm = pcm.contiguous()
        if 0 <= fmt <= 3 and pcm.element_size() != (4, 2, 4, 1)[fmt]:
            raise SvcmiError(f"pcm_resample: fmt {fmt} does not describe a {pcm.dtype} tensor")
        if taps is not None and not (taps.dtype == torch.float32 and taps.is_contiguous() and taps.dim() == 2 and taps.shape[0] == up):
            raise SvcmiError("pcm_resample: taps must be a contiguous float32 [up, K] image")
        frames = pcm.numel() // max(int(channels), 1)
        n_out = -(-frames * up // down) if up >= 1 and down >= 1 else 0
        out = torch.empty(max(n_out, 0), dtype=torch.float32, device=pcm.device)
        self._call("svcmi_pcm_resample_f32", _ptr(pcm), fmt, channels, frames, _ptr(taps), up, down,
                   taps.shape[1] if taps is not None else 0, half, _ptr(out), n_out, self._stream(),
                   work={"bytes": float(pcm.numel() * pcm.element_size() + 4 * n_out)})
        return out

    # ------------------------------------------------------------------ linear spectrogram (csrc/spectrogram.hip)
    def linear_spectrogram(self, x, basis, n_fft, hop, pad, eps=1e-6, out=None):
        """x [B, n] float32 (unit stride along n, any batch stride) -> STFT magnitudes [B, n_fft // 2 + 1, frames] of the signal reflect-padded
        by ``pad`` on both sides, frames = 1 + (n + 2 pad - n_fft) // hop, sqrt(re^2 + im^2 + eps): reflect padding, windowed DFT and
        magnitude in one launch (svcmi_linear_spectrogram_f32).  ``basis``: the [n_fft, n_fft + 2] table of
        ``svcmi.vits.spectrogram.spectrogram_basis``."""
        self._chk(x, basis, out)
        if not (x.dim() == 2 and x.dtype == torch.float32 and (x.shape[1] <= 1 or x.stride(1) == 1)):
            raise SvcmiError("linear_spectrogram: x must be float32 [B, n] with unit stride along n")
        bins = n_fft // 2 + 1
        if not (basis.dtype == torch.float32 and basis.is_contiguous() and tuple(basis.shape) == (n_fft, 2 * bins)):
            raise SvcmiError("linear_spectrogram: basis must be a contiguous float32 [n_fft, n_fft + 2] table")
        B, n = x.shape
        frames = 1 + (n + 2 * pad - n_fft) // hop if hop >= 1 and n + 2 * pad >= n_fft else 0
        if out is None:
            out = torch.empty(B, bins, max(frames, 0), dtype=torch.float32, device=x.device)
        elif not (out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, bins, frames)):
            raise SvcmiError("linear_spectrogram: out must be a contiguous float32 [B, bins, frames] tensor")
        self._call("svcmi_linear_spectrogram_f32", _ptr(x), x.stride(0), B, n, _ptr(basis), n_fft, hop, pad, float(eps), _ptr(out), frames,
                   self._stream(), work={"flops": 4.0 * B * frames * bins * n_fft, "bytes": 4.0 * (B * n + basis.numel() + out.numel())})
        return out

    # ------------------------------------------------------------------ checkpoint scoring (csrc/spectral_loss.hip)
    def stft_distance(self, x, y, basis, n_fft, hop, pad=None, floor=1e-7, out=None, workspace=None):
        """One STFT resolution of a pair: ``x`` predicted, ``y`` recorded, float32 [B, n] (unit stride along n, any batch strides) ->
        float64 [B, 3] = (sum (my - mx)^2, sum my^2, sum |log my - log mx|) over all bins x frames of the signals reflect-padded by ``pad``
        (default n_fft // 2: torch.stft's center=True), m = sqrt(max(re^2 + im^2, floor)) (svcmi_stft_distance_f32: no spectrogram is
        ever written).  ``basis``: the table of ``svcmi.vits.spectrogram.spectrogram_basis``.  ``workspace``: a float32 tensor of
        ``stft_distance_workspace(...)`` elements (default: a fresh one per call, so calls on different streams never share it)."""
        self._chk(x, y, basis, out, workspace)
        for name, t in (("x", x), ("y", y)):
            if not (t.dim() == 2 and t.dtype == torch.float32 and (t.shape[1] <= 1 or t.stride(1) == 1)):
                raise SvcmiError(f"stft_distance: {name} must be float32 [B, n] with unit stride along n")
        if x.shape != y.shape or x.device != y.device:
            raise SvcmiError(f"stft_distance: x {tuple(x.shape)} on {x.device} and y {tuple(y.shape)} on {y.device} differ")
        bins = n_fft // 2 + 1
        if not (basis.dtype == torch.float32 and basis.is_contiguous() and tuple(basis.shape) == (n_fft, 2 * bins)):
            raise SvcmiError("stft_distance: basis must be a contiguous float32 [n_fft, n_fft + 2] table")
        B, n = x.shape
        pad = n_fft // 2 if pad is None else pad
        frames = 1 + (n + 2 * pad - n_fft) // hop if hop >= 1 and n + 2 * pad >= n_fft else 0
        need = self.stft_distance_workspace(B, n, n_fft, hop, pad)
        if workspace is None:
            workspace = torch.empty(max(need, 1), dtype=torch.float32, device=x.device)
        elif not (workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.numel() >= need):
            raise SvcmiError(f"stft_distance: workspace must be a contiguous float32 tensor of at least {need} elements")
        if out is None:
            out = torch.empty(B, 3, dtype=torch.float64, device=x.device)
        elif not (out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (B, 3)):
            raise SvcmiError("stft_distance: out must be a contiguous float64 [B, 3] tensor")
        self._call("svcmi_stft_distance_f32", _ptr(x), x.stride(0), _ptr(y), y.stride(0), B, n, _ptr(basis), n_fft, hop, pad, float(floor), frames,
                   _ptr(workspace), 4 * workspace.numel(), _ptr(out), self._stream(),
                   work={"flops": 8.0 * B * frames * bins * n_fft, "bytes": 4.0 * (2 * B * n + basis.numel())})
        return out

    def stft_distance_workspace(self, batch, n, n_fft, hop, pad=None):
        """float32 elements of ``stft_distance``'s workspace (svcmi_stft_distance_workspace_bytes / 4); raises for a geometry the launch refuses."""
        nbytes = self.lib.svcmi_stft_distance_workspace_bytes(batch, n, n_fft, hop, n_fft // 2 if pad is None else pad)
        if nbytes < 0:
            raise SvcmiError(f"stft_distance: batch {batch}, n {n}, n_fft {n_fft}, hop {hop}, pad {pad} is not a valid geometry (code {nbytes})")
        return nbytes // 4

    def log_mel(self, spec, melT, n_mel, clip=1e-5, out=None):
        """spec [B, bins, frames] float32 contiguous -> log(max(mel @ spec, clip)) [B, n_mel, frames] on the matrix cores (svcmi_log_mel_f32).
        ``melT``: the filterbank transposed and padded, contiguous float32 [bins, ldm] with ldm >= n_mel rounded up to 32 and zeros in the
        columns past n_mel (``svcmi.vits_extend.stft.mel_table``)."""
        self._chk(spec, melT, out)
        if not (spec.dim() == 3 and spec.dtype == torch.float32 and spec.is_contiguous()):
            raise SvcmiError("log_mel: spec must be a contiguous float32 [B, bins, frames] tensor")
        B, bins, frames = spec.shape
        if not (melT.dim() == 2 and melT.dtype == torch.float32 and melT.is_contiguous() and melT.shape[0] == bins
                and melT.shape[1] >= (n_mel + 31) // 32 * 32):
            raise SvcmiError("log_mel: melT must be a contiguous float32 [bins, ldm] table, ldm >= n_mel rounded up to 32")
        if out is None:
            out = torch.empty(B, n_mel, frames, dtype=torch.float32, device=spec.device)
        elif not (out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, n_mel, frames)):
            raise SvcmiError("log_mel: out must be a contiguous float32 [B, n_mel, frames] tensor")
        self._call("svcmi_log_mel_f32", _ptr(spec), B, bins, frames, _ptr(melT), melT.shape[1], n_mel, float(clip), _ptr(out), self._stream(),
                   work={"flops": 2.0 * B * frames * bins * n_mel, "bytes": 4.0 * (spec.numel() + melT.numel() + out.numel())})
        return out

    def abs_diff_sum(self, a, b, out=None):
        """sum |a - b| per batch item of two equal-shaped float32 tensors [B, ...] (each item contiguous, any batch stride) -> float64 [B]
        (svcmi_abs_diff_sum_f32: fixed-order partials, no atomics)."""
        self._chk(a, b, out)
        if a.shape != b.shape or a.dim() < 2 or a.dtype != torch.float32 or b.dtype != torch.float32 or a.device != b.device:
            raise SvcmiError("abs_diff_sum: a and b must be float32 tensors [B, ...] of one shape on one device")
        if not (a[0].is_contiguous() and b[0].is_contiguous()):
            raise SvcmiError("abs_diff_sum: every batch item must be contiguous")
        B, count = a.shape[0], a[0].numel()
        nbytes = self.lib.svcmi_abs_diff_sum_workspace_bytes(B, count)
        if nbytes < 0:
            raise SvcmiError(f"abs_diff_sum: batch {B} x {count} elements is not a valid shape")
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device)
        if out is None:
            out = torch.empty(B, dtype=torch.float64, device=a.device)
        elif not (out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (B,)):
            raise SvcmiError("abs_diff_sum: out must be a contiguous float64 [B] tensor")
        self._call("svcmi_abs_diff_sum_f32", _ptr(a), a.stride(0), _ptr(b), b.stride(0), B, count, _ptr(workspace), nbytes, _ptr(out), self._stream(),
                   work={"bytes": 8.0 * B * count})
        return out

    # ------------------------------------------------------------------ speaker encoder (csrc/lstm.hip)
    def lstm_step(self, gx, whh, hseq, c, t):
        """One time step of one LSTM layer, in place: ``gx`` [B, T, 4H] (tile order, biases included), ``whh`` [4H, H] (tile order),
        ``hseq`` [B, T, H] (row t - 1 read, row t written), ``c`` [B, H] (updated)."""
        self._chk(gx, whh, hseq, c)
        B, T, H = hseq.shape
        self._call("svcmi_lstm_step_f32", _ptr(gx), gx.stride(0), _ptr(whh), _ptr(hseq), hseq.stride(0), hseq.stride(1), _ptr(c), c.stride(0),
                   B, H, t, T, self._stream(), work={"flops": 8.0 * B * H * H if t else 0.0, "bytes": 16.0 * H * H if t else 0.0})
        return hseq

    def preemph_pad(self, x, pad, coef):
        """x [B, n] -> [B, n + 2 pad]: pre-emphasis y[n] = x[n] - coef x[n - 1] (y[0] = x[0]) and reflect padding in one pass."""
        self._chk(x)
        B, n = x.shape
        y = torch.empty(B, n + 2 * pad, dtype=torch.float32, device=x.device)
        self._call("svcmi_preemph_pad_f32", _ptr(x), _ptr(y), B, n, pad, float(coef), self._stream())
        return y

    def magnitude_spectrum(self, ri, nbins, half):
        self._chk(ri)
        B, T, ld = ri.shape
        p = torch.empty(B, T, half, dtype=torch.float32, device=ri.device)
        self._call("svcmi_magnitude_spectrum_f32", _ptr(ri), _ptr(p), B * T, nbins, half, ld, half, self._stream())
        return p

    def speaker_mel_finish(self, mel, ref_level_db=20.0, min_level_db=-100.0, max_norm=4.0):
        """In place on the contiguous mel projection: amplitude -> dB, - ref level, range normalisation to +-max_norm, clip."""
        self._chk(mel)
        assert mel.is_contiguous()
        self._call("svcmi_speaker_mel_finish_f32", _ptr(mel), mel.numel(), float(ref_level_db), float(min_level_db), float(max_norm),
                   self._stream())
        return mel

    def l2norm_rows(self, x):
        """x [rows, d] -> x / max(|x|_2, 1e-12) per row."""
        self._chk(x)
        y = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
        self._call("svcmi_l2norm_rows_f32", _ptr(x), x.stride(0), x.shape[0], x.shape[1], _ptr(y), y.stride(0), self._stream())
        return y

    def group_mean(self, x, rows_per_group):
        """x [groups * rows_per_group, d] (contiguous) -> [groups, d]: the mean of every run of ``rows_per_group`` rows."""
        self._chk(x)
        assert x.is_contiguous() and x.shape[0] % rows_per_group == 0
        y = torch.empty(x.shape[0] // rows_per_group, x.shape[1], dtype=torch.float32, device=x.device)
        self._call("svcmi_group_mean_f32", _ptr(x), rows_per_group, y.shape[0], x.shape[1], _ptr(y), self._stream())
        return y

    def speaker_encoder_fwd(self, cm, mel):
        """LSTMSpeakerEncoder.inference as ONE call: mel [B <= 64, T, input_dim] -> L2-normalised embeddings [B, proj_dim]."""
        self._chk(mel)
        m = cm.struct
        mel = mel.contiguous()
        B, T, _ = mel.shape
        need = self.lib.svcmi_speaker_encoder_workspace_bytes(ctypes.byref(m), B, T)
        if need < 0:
            raise SvcmiError(f"svcmi_speaker_encoder_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, mel.device)
        out = torch.empty(B, m.proj_dim, dtype=torch.float32, device=mel.device)
        self._stage_call("svcmi_speaker_encoder_fwd", ctypes.byref(m), _ptr(mel), B, T, _ptr(out), ws, ws_bytes, self._stream())
        return out

    # ------------------------------------------------------------------ voice-activity detector (csrc/vad.hip)
    @staticmethod
    def _vad_geometry(audio, offsets, lengths):
        if audio.dim() != 1 or audio.dtype != torch.float32 or not audio.is_contiguous():
            raise SvcmiError("vad: audio must be one contiguous float32 buffer [n] holding every recording")
        for t in (offsets, lengths):
            if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous() or t.device != audio.device or t.shape != offsets.shape:
                raise SvcmiError("vad: offsets / lengths must be contiguous int64 [batch] tensors on the audio's device")
        return int(offsets.shape[0])

    def vad_frontend(self, cm, audio, offsets, lengths, wmax):
        """Everything in front of the LSTM for every window of ``batch`` recordings (recording b = audio[offsets[b] : offsets[b] +
        lengths[b]], device int64 tensors): (feat [batch, wmax, 64], gates [batch, wmax, 256]); rows past a recording's last window
        stay zero."""
        self._chk(audio, offsets, lengths)
        B = self._vad_geometry(audio, offsets, lengths)
        feat = torch.zeros(B, wmax, 64, dtype=torch.float32, device=audio.device)
        gates = torch.zeros(B, wmax, 256, dtype=torch.float32, device=audio.device)
        self._call("svcmi_vad_frontend_f32", ctypes.byref(cm.struct), _ptr(audio), _ptr(offsets), _ptr(lengths), B, wmax, _ptr(feat), _ptr(gates),
                   self._stream(), work={"flops": 1.3e6 * B * wmax})
        return feat, gates

    def vad_lstm_scan(self, cm, gates, lengths, state=None):
        """The two LSTM layers and the decoder over every recording's windows: gates [batch, wmax, 256] (layer 0's pre-activations),
        lengths int64 [batch] in samples -> probabilities [batch, wmax] (zero past a recording's last window).  ``state`` [batch, 4, 64]
        (h0, c0, h1, c1) is read at the start and overwritten with the final state; None starts from zero."""
        self._chk(gates, lengths, state)
        B, wmax, _ = gates.shape
        if not gates.is_contiguous() or gates.shape[2] != 256 or tuple(lengths.shape) != (B,) or lengths.dtype != torch.int64:
            raise SvcmiError("vad_lstm_scan: gates must be contiguous [batch, wmax, 256] and lengths int64 [batch]")
        if state is not None and not (state.is_contiguous() and tuple(state.shape) == (B, 4, 64) and state.dtype == torch.float32):
            raise SvcmiError("vad_lstm_scan: state must be a contiguous float32 [batch, 4, 64] tensor")
        probs = torch.zeros(B, wmax, dtype=torch.float32, device=gates.device)
        self._call("svcmi_vad_lstm_scan_f32", ctypes.byref(cm.struct), _ptr(gates), _ptr(lengths), B, wmax, _ptr(state), _ptr(probs), self._stream())
        return probs

    def vad_probs_fwd(self, cm, audio, offsets, lengths, wmax, state=None):
        """Both launches as ONE stage call (svcmi_vad_probs_fwd): probabilities [batch, wmax]."""
        self._chk(audio, offsets, lengths, state)
        B = self._vad_geometry(audio, offsets, lengths)
        if state is not None and not (state.is_contiguous() and tuple(state.shape) == (B, 4, 64) and state.dtype == torch.float32):
            raise SvcmiError("vad_probs_fwd: state must be a contiguous float32 [batch, 4, 64] tensor")
        need = self.lib.svcmi_vad_workspace_bytes(B, wmax)
        if need < 0:
            raise SvcmiError(f"svcmi_vad_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, audio.device)
        probs = torch.zeros(B, wmax, dtype=torch.float32, device=audio.device)
        self._stage_call("svcmi_vad_probs_fwd", ctypes.byref(cm.struct), _ptr(audio), _ptr(offsets), _ptr(lengths), B, wmax, _ptr(state),
                         _ptr(probs), ws, ws_bytes, self._stream())
        return probs

    def mask_spans(self, x, spans, n_ref, ratio=2):
        """x float32 [n_in]; spans int32 [S, 2] (sorted, disjoint, in samples of the reference rate; S may be 0) -> float32
        [min(n_in, ratio * n_ref)]: x inside the spans scaled by ``ratio``, zero outside."""
        self._chk(x, spans)
        if x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous():
            raise SvcmiError("mask_spans: x must be a contiguous float32 [n] tensor")
        if spans.dtype != torch.int32 or spans.dim() != 2 or spans.shape[1] != 2 or not spans.is_contiguous():
            raise SvcmiError("mask_spans: spans must be a contiguous int32 [S, 2] tensor")
        n = min(int(x.shape[0]), int(ratio) * int(n_ref))
        out = torch.empty(max(n, 0), dtype=torch.float32, device=x.device)
        S = int(spans.shape[0])
        self._call("svcmi_mask_spans_f32", _ptr(x), x.shape[0], _ptr(spans) if S else 0, S, int(n_ref), int(ratio), _ptr(out), n, self._stream(),
                   work={"bytes": 8.0 * n})
        return out

    # ------------------------------------------------------------------ salience F0 extractor (csrc/salience.hip)
    @staticmethod
    def _salience_frames(plan, n):
        frames = 1 + int(n) // int(plan.hop)
        if frames < 2:
            raise SvcmiError(f"salience: {n} samples at hop {plan.hop} give {frames} frame; the phase increment needs at least 2")
        return frames

    def salience_stft(self, plan, x):
        """x float32 [n] (unit stride) -> complex64 [frames, n_bins]: the centred, zero-padded STFT restricted to the plan's bins
        (svcmi_salience_stft_f32).  ``plan``: the ``struct`` of ``svcmi.pitch.core.salience.salience_plan``."""
        self._chk(x)
        if not (x.dim() == 1 and x.dtype == torch.float32 and (x.shape[0] <= 1 or x.stride(0) == 1)):
            raise SvcmiError("salience_stft: x must be float32 [n] with unit stride")
        frames = self._salience_frames(plan, x.shape[0])
        X = torch.empty(frames, plan.n_bins, dtype=torch.complex64, device=x.device)
        self._call("svcmi_salience_stft_f32", ctypes.byref(plan), _ptr(x), x.shape[0], _ptr(X), frames, self._stream(),
                   work={"flops": 4.0 * frames * plan.n_bins * plan.n_fft})
        return X

    def salience_map(self, plan, X):
        """X complex64 [frames, n_bins] -> (lf [frames, n_pitch], z [frames, n_pitch], gmax uint32-as-int32 [2]): the smoothed and
        thresholded log-frequency spectrogram, the salience map, and the bit patterns of their maxima before thresholding."""
        self._chk(X)
        if not (X.dim() == 2 and X.dtype == torch.complex64 and X.is_contiguous() and X.shape[1] == plan.n_bins):
            raise SvcmiError("salience_map: X must be a contiguous complex64 [frames, n_bins] tensor")
        frames = X.shape[0]
        lf = torch.empty(frames, plan.n_pitch, dtype=torch.float32, device=X.device)
        z = torch.empty(frames, plan.n_pitch, dtype=torch.float32, device=X.device)
        gmax = torch.empty(2, dtype=torch.int32, device=X.device)
        self._call("svcmi_salience_map_f32", ctypes.byref(plan), _ptr(X), frames, _ptr(lf), _ptr(z), _ptr(gmax), self._stream())
        return lf, z, gmax

    def salience_dp(self, z, tol, log_hi, log_lo):
        """z float32 [frames, n_pitch] -> path int32 [frames]: the trajectory of pitch/core/salience.py:306-349 in fp64, every
        predecessor evaluated, lowest index on ties (svcmi_salience_dp_f64)."""
        self._chk(z)
        if not (z.dim() == 2 and z.dtype == torch.float32 and z.is_contiguous()):
            raise SvcmiError("salience_dp: z must be a contiguous float32 [frames, n_pitch] tensor")
        frames, B = z.shape
        ptr = torch.empty(frames, B, dtype=torch.int16, device=z.device)
        path = torch.empty(frames, dtype=torch.int32, device=z.device)
        self._call("svcmi_salience_dp_f64", _ptr(z), frames, B, int(tol), float(log_hi), float(log_lo), _ptr(ptr), _ptr(path), self._stream())
        return path

    def salience_f0_fwd(self, plan, x, want_map=False):
        """waveform float32 [n] -> path int32 [frames] as ONE stage call (svcmi_salience_f0_fwd); ``want_map``: also the salience map
        [frames, n_pitch]."""
        self._chk(x)
        if not (x.dim() == 1 and x.dtype == torch.float32 and (x.shape[0] <= 1 or x.stride(0) == 1)):
            raise SvcmiError("salience_f0_fwd: x must be float32 [n] with unit stride")
        frames = self._salience_frames(plan, x.shape[0])
        need = self.lib.svcmi_salience_workspace_bytes(ctypes.byref(plan), x.shape[0])
        if need < 0:
            raise SvcmiError(f"svcmi_salience_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, x.device)
        path = torch.empty(frames, dtype=torch.int32, device=x.device)
        z = torch.empty(frames, plan.n_pitch, dtype=torch.float32, device=x.device) if want_map else None
        self._stage_call("svcmi_salience_f0_fwd", ctypes.byref(plan), _ptr(x), x.shape[0], _ptr(path), _ptr(z), ws, ws_bytes, self._stream())
        return (path, z) if want_map else path

    # ------------------------------------------------------------------ pYIN F0 extractor (csrc/pyin.hip)
    @staticmethod
    def _pyin_clip(name, plan, x):
        if not (x.dim() == 1 and x.dtype == torch.float32 and (x.shape[0] <= 1 or x.stride(0) == 1)):
            raise SvcmiError(f"{name}: x must be float32 [n] with unit stride")
        frames = 1 + int(x.shape[0]) // int(plan.hop)
        if frames < 2:
            raise SvcmiError(f"{name}: {x.shape[0]} samples at hop {plan.hop} give one frame; the trajectory needs at least 2")
        return frames

    def pyin_cmndf(self, plan, x):
        """x float32 [n] (unit stride) -> (cmndf float64 [frames, p_max + 1], rms float64 [frames]): YIN's cumulative mean normalised
        difference function of every centred frame (svcmi_pyin_cmndf_f64).  ``plan``: the ``struct`` of ``svcmi.pitch.core.pyin.pyin_plan``."""
        self._chk(x)
        frames = self._pyin_clip("pyin_cmndf", plan, x)
        cm = torch.empty(frames, plan.p_max + 1, dtype=torch.float64, device=x.device)
        rms = torch.empty(frames, dtype=torch.float64, device=x.device)
        self._call("svcmi_pyin_cmndf_f64", ctypes.byref(plan), _ptr(x), x.shape[0], _ptr(cm), _ptr(rms), frames, self._stream(),
                   work={"flops": 3.0 * frames * plan.p_max * plan.n_fft})
        return cm, rms

    def pyin_observe(self, plan, cmndf, want_log=False):
        """cmndf float64 [frames, p_max + 1] -> (O float64 [frames, 2 n_pitch], lag_thr, val_thr float64 [frames, n_thr]) and, with
        ``want_log``, log(O + tiny) as a fourth tensor (svcmi_pyin_observe_f64)."""
        self._chk(cmndf)
        if not (cmndf.dim() == 2 and cmndf.dtype == torch.float64 and cmndf.is_contiguous() and cmndf.shape[1] == plan.p_max + 1 and cmndf.shape[0] >= 1):
            raise SvcmiError("pyin_observe: cmndf must be a contiguous float64 [frames, p_max + 1] tensor")
        frames = cmndf.shape[0]
        new = lambda cols: torch.empty(frames, cols, dtype=torch.float64, device=cmndf.device)
        O, lag, val = new(2 * plan.n_pitch), new(plan.n_thr), new(plan.n_thr)
        logO = new(2 * plan.n_pitch) if want_log else None
        self._call("svcmi_pyin_observe_f64", ctypes.byref(plan), _ptr(cmndf), frames, _ptr(O), _ptr(logO), _ptr(lag), _ptr(val), self._stream())
        return (O, lag, val, logO) if want_log else (O, lag, val)

    def pyin_viterbi(self, logO, band, log_tiny, log_cross, log_c):
        """logO float64 [frames, 2 B] (time-major), band float64 [B, 2 max_step + 1] -> path int32 [frames]: numpy's argmax index for
        index (svcmi_pyin_viterbi_f64)."""
        self._chk(logO)
        self._chk(band)
        if not (logO.dim() == 2 and logO.dtype == torch.float64 and logO.is_contiguous() and logO.shape[1] % 2 == 0):
            raise SvcmiError("pyin_viterbi: logO must be a contiguous float64 [frames, 2 B] tensor")
        frames, B = logO.shape[0], logO.shape[1] // 2
        if not (band.dim() == 2 and band.dtype == torch.float64 and band.is_contiguous() and band.shape[0] == B and band.shape[1] % 2 == 1):
            raise SvcmiError("pyin_viterbi: band must be a contiguous float64 [B, 2 max_step + 1] tensor")
        ptr = torch.empty(frames, 2 * B, dtype=torch.int16, device=logO.device)
        path = torch.empty(frames, dtype=torch.int32, device=logO.device)
        self._call("svcmi_pyin_viterbi_f64", _ptr(logO), frames, B, band.shape[1] // 2, _ptr(band), float(log_tiny), float(log_cross), float(log_c),
                   _ptr(ptr), _ptr(path), self._stream())
        return path

    def pyin_f0_fwd(self, plan, x, want_parts=False):
        """clip float32 [n] -> out float64 [2, frames] (f0, conf) and path int32 [frames] as ONE stage call (svcmi_pyin_f0_fwd);
        ``want_parts``: also a dict of rms [frames], O [frames, 2 n_pitch], lag_thr and val_thr [frames, n_thr]."""
        self._chk(x)
        frames = self._pyin_clip("pyin_f0_fwd", plan, x)
        need = self.lib.svcmi_pyin_workspace_bytes(ctypes.byref(plan), x.shape[0])
        if need < 0:
            raise SvcmiError(f"svcmi_pyin_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, x.device)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=x.device)
        out = new(2, frames)
        path = torch.empty(frames, dtype=torch.int32, device=x.device)
        parts = dict(rms=new(frames), O=new(frames, 2 * plan.n_pitch), lag_thr=new(frames, plan.n_thr), val_thr=new(frames, plan.n_thr)) if want_parts else {}
        self._stage_call("svcmi_pyin_f0_fwd", ctypes.byref(plan), _ptr(x), x.shape[0], _ptr(out[0]), _ptr(out[1]), _ptr(path), _ptr(parts.get("rms")),
                         _ptr(parts.get("O")), _ptr(parts.get("lag_thr")), _ptr(parts.get("val_thr")), ws, ws_bytes, self._stream())
        return (out, path, parts) if want_parts else (out, path)

    # ------------------------------------------------------------------ YIN F0 extractor (csrc/yin.hip)
    @staticmethod
    def _yin_clip(name, plan, x):
        if not (x.dim() == 1 and x.dtype == torch.float32 and x.shape[0] >= 1 and (x.shape[0] <= 1 or x.stride(0) == 1)):
            raise SvcmiError(f"{name}: x must be float32 [n >= 1] with unit stride")
        return 1 + int(x.shape[0]) // int(plan.hop)

    def yin_cmndf(self, plan, x):
        """x float32 [n] (unit stride) -> cmndf float64 [frames, lag_max + 1], frames = 1 + n // hop >= 1: the rows of ``pyin_cmndf`` at
        p_max = lag_max, bit for bit (svcmi_yin_cmndf_f64).  ``plan``: the ``struct`` of ``svcmi.pitch.core.yin.yin_plan``."""
        self._chk(x)
        frames = self._yin_clip("yin_cmndf", plan, x)
        cm = torch.empty(frames, plan.lag_max + 1, dtype=torch.float64, device=x.device)
        rms = torch.empty(frames, dtype=torch.float64, device=x.device)      # the shared kernel writes it; YIN has no use for it
        self._call("svcmi_yin_cmndf_f64", ctypes.byref(plan), _ptr(x), x.shape[0], _ptr(cm), _ptr(rms), frames, self._stream(),
                   work={"flops": 3.0 * frames * plan.lag_max * plan.n_fft})
        return cm

    def yin_pick(self, plan, cmndf, want_parts=False):
        """cmndf float64 [frames, lag_max + 1] (no NaN, no inf; not modified) -> out float64 [2, frames] (lag, f0 = fs / lag): the two
        thresholdings of svcmi_yin_pick_f64; ``want_parts``: also (lag_first float64 [frames], kind int32 [frames])."""
        self._chk(cmndf)
        if not (cmndf.dim() == 2 and cmndf.dtype == torch.float64 and cmndf.is_contiguous() and cmndf.shape[1] == plan.lag_max + 1 and cmndf.shape[0] >= 1):
            raise SvcmiError("yin_pick: cmndf must be a contiguous float64 [frames, lag_max + 1] tensor")
        frames = cmndf.shape[0]
        out = torch.empty(2, frames, dtype=torch.float64, device=cmndf.device)
        first = torch.empty(frames, dtype=torch.float64, device=cmndf.device) if want_parts else None
        kind = torch.empty(frames, dtype=torch.int32, device=cmndf.device) if want_parts else None
        self._call("svcmi_yin_pick_f64", ctypes.byref(plan), _ptr(cmndf), frames, _ptr(out[0]), _ptr(out[1]), _ptr(first), _ptr(kind), self._stream())
        return (out, first, kind) if want_parts else out

    def yin_aperiodicity(self, plan, x, lag):
        """x float32 [n] (unit stride), lag float64 [1 + n // hop] (0 <= lag <= n_fft, a fractional one < n_fft) -> ap float64 [frames]
        (svcmi_yin_aperiodicity_f64)."""
        self._chk(x)
        self._chk(lag)
        frames = self._yin_clip("yin_aperiodicity", plan, x)
        if not (lag.dim() == 1 and lag.dtype == torch.float64 and lag.is_contiguous() and lag.shape[0] == frames):
            raise SvcmiError(f"yin_aperiodicity: lag must be a contiguous float64 [{frames}] tensor")
        ap = torch.empty(frames, dtype=torch.float64, device=x.device)
        self._call("svcmi_yin_aperiodicity_f64", ctypes.byref(plan), _ptr(x), x.shape[0], _ptr(lag), frames, _ptr(ap), self._stream())
        return ap

    def yin_f0_fwd(self, plan, x, want_parts=False):
        """clip float32 [n] -> out float64 [2, frames] (f0, ap) as ONE stage call (svcmi_yin_f0_fwd: three launches, nothing waits);
        ``want_parts``: also a dict of lag, lag_first float64 [frames] and kind int32 [frames]."""
        self._chk(x)
        frames = self._yin_clip("yin_f0_fwd", plan, x)
        need = self.lib.svcmi_yin_workspace_bytes(ctypes.byref(plan), x.shape[0])
        if need < 0:
            raise SvcmiError(f"svcmi_yin_workspace_bytes failed with code {need}")
        ws, ws_bytes = self.stage_workspace(need, x.device)
        new = lambda dtype: torch.empty(frames, dtype=dtype, device=x.device)
        out = torch.empty(2, frames, dtype=torch.float64, device=x.device)
        parts = dict(lag=new(torch.float64), lag_first=new(torch.float64), kind=new(torch.int32)) if want_parts else {}
        self._stage_call("svcmi_yin_f0_fwd", ctypes.byref(plan), _ptr(x), x.shape[0], _ptr(out[0]), _ptr(out[1]), _ptr(parts.get("lag")),
                         _ptr(parts.get("lag_first")), _ptr(parts.get("kind")), ws, ws_bytes, self._stream())
        return (out, parts) if want_parts else out

    # ------------------------------------------------------------------ SWIPE' F0 extractor (csrc/swipe.hip)
    def _swipe_frames(self, plan, window, n):
        frames = self.lib.svcmi_swipe_frames(ctypes.byref(plan), int(window), int(n))
        if frames < 0:
            raise SvcmiError(f"svcmi_swipe_frames failed with code {frames}")
        return int(frames)

    @staticmethod
    def _swipe_rows(name, t, cols):
        if not (t.dim() == 2 and t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == cols and t.shape[0] >= 1):
            raise SvcmiError(f"{name}: expected a contiguous float32 [frames, {cols}] tensor, got {tuple(t.shape)}")

    def swipe_mag(self, plan, window, x):
        """x float32 [n] (unit stride) -> Y float32 [frames_w, ld(N / 2 + 1)]: the centred Hann STFT magnitudes of the end-padded clip at
        window ``window`` of the plan, pad columns zero (svcmi_swipe_mag_f32).  ``plan``: the ``struct`` of ``swipe_plan``."""
        self._chk(x)
        if not (x.dim() == 1 and x.dtype == torch.float32 and (x.shape[0] <= 1 or x.stride(0) == 1)):
            raise SvcmiError("swipe_mag: x must be float32 [n] with unit stride")
        frames = self._swipe_frames(plan, window, x.shape[0])
        N = plan.win[window].n_fft
        Y = torch.empty(frames, (N // 2 + 8) & ~7, dtype=torch.float32, device=x.device)
        self._call("svcmi_swipe_mag_f32", ctypes.byref(plan), int(window), _ptr(x), x.shape[0], _ptr(Y), self._stream(),
                   work={"flops": 4.0 * frames * (N // 2 + 1) * N})
        return Y

    def swipe_resample(self, plan, window, Y):
        """Y float32 [frames, ld(N / 2 + 1)] -> L float32 [frames, ld(n_log)] = W_N Y per frame (svcmi_swipe_resample_f32)."""
        self._chk(Y)
        self._swipe_rows("swipe_resample", Y, (plan.win[window].n_fft // 2 + 8) & ~7)
        L = torch.empty(Y.shape[0], (plan.n_log + 7) & ~7, dtype=torch.float32, device=Y.device)
        self._call("svcmi_swipe_resample_f32", ctypes.byref(plan), int(window), _ptr(Y), Y.shape[0], _ptr(L), self._stream(),
                   work={"flops": 2.0 * Y.shape[0] * Y.shape[1] * plan.n_log})
        return L

    def swipe_strength(self, plan, window, L):
        """L float32 [frames, ld(n_log)] -> S_N float32 [frames, n_cand] = K_N L / (||L|| + eps) per frame (svcmi_swipe_strength_f32)."""
        self._chk(L)
        self._swipe_rows("swipe_strength", L, (plan.n_log + 7) & ~7)
        SN = torch.empty(L.shape[0], plan.win[window].n_cand, dtype=torch.float32, device=L.device)
        self._call("svcmi_swipe_strength_f32", ctypes.byref(plan), int(window), _ptr(L), L.shape[0], _ptr(SN), self._stream(),
                   work={"flops": 2.0 * L.shape[0] * L.shape[1] * SN.shape[1]})
        return SN

    def swipe_accum(self, plan, parts, n):
        """parts: the windows' S_N in the plan's order, for a clip of ``n`` samples -> S float32 [ceil(n / hop), n_pitch]: linear
        interpolation in time and the weighted sum, smallest window first (svcmi_swipe_accum_f32)."""
        self._chk(*parts)
        if len(parts) != plan.n_win:
            raise SvcmiError(f"swipe_accum: {len(parts)} parts for {plan.n_win} windows")
        for w, t in enumerate(parts):
            self._swipe_rows("swipe_accum", t, plan.win[w].n_cand)
            if t.shape[0] != self._swipe_frames(plan, w, n):
                raise SvcmiError(f"swipe_accum: window {w} has {t.shape[0]} frames, a clip of {n} samples gives {self._swipe_frames(plan, w, n)}")
        sn = torch.cat([t.reshape(-1) for t in parts])
        S = torch.empty(self._swipe_frames(plan, -1, n), plan.n_pitch, dtype=torch.float32, device=sn.device)
        self._call("svcmi_swipe_accum_f32", ctypes.byref(plan), _ptr(sn), int(n), _ptr(S), self._stream())
        return S

    def swipe_finish(self, S, n_log, f_min, step, threshold=0.0):
        """S float32 [frames, B] -> (out float64 [2, frames] = f0, conf; amax int32 [frames]; flags int32 [1], the number of frames whose
        arg-max is B - 1): svcmi_swipe_finish_f64."""
        self._chk(S)
        if not (S.dim() == 2 and S.dtype == torch.float32 and S.is_contiguous() and S.shape[0] >= 1):
            raise SvcmiError("swipe_finish: S must be a contiguous float32 [frames, B] tensor")
        frames, B = S.shape
        out = torch.empty(2, frames, dtype=torch.float64, device=S.device)
        amax = torch.empty(frames, dtype=torch.int32, device=S.device)
        flags = torch.empty(1, dtype=torch.int32, device=S.device)
        self._call("svcmi_swipe_finish_f64", _ptr(S), frames, B, int(n_log), float(f_min), float(step), float(threshold), _ptr(out[0]), _ptr(out[1]),
                   _ptr(amax), _ptr(flags), self._stream())
        return out, amax, flags

    def swipe_f0_fwd(self, plan, x, want_map=False):
        """clip float32 [n] -> out float64 [3, frames] (f0, conf, and the flag word as a float64 in every cell of the third row, so that
        ONE device -> host copy carries everything) as one stage call (svcmi_swipe_f0_fwd); ``want_map``: also S [frames, n_pitch]."""
        self._chk(x)
        if not (x.dim() == 1 and x.dtype == torch.float32 and (x.shape[0] <= 1 or x.stride(0) == 1)):
            raise SvcmiError("swipe_f0_fwd: x must be float32 [n] with unit stride")
        need = self.lib.svcmi_swipe_workspace_bytes(ctypes.byref(plan), x.shape[0])
        if need < 0:
            raise SvcmiError(f"svcmi_swipe_workspace_bytes failed with code {need}")
        frames = self._swipe_frames(plan, -1, x.shape[0])
        ws, ws_bytes = self.stage_workspace(need, x.device)
        out = torch.empty(3, frames, dtype=torch.float64, device=x.device)
        flags = torch.empty(1, dtype=torch.int32, device=x.device)
        S = torch.empty(frames, plan.n_pitch, dtype=torch.float32, device=x.device) if want_map else None
        self._stage_call("svcmi_swipe_f0_fwd", ctypes.byref(plan), _ptr(x), x.shape[0], _ptr(out[0]), _ptr(out[1]), _ptr(S), _ptr(flags), ws, ws_bytes,
                         self._stream())
        out[2] = flags.to(torch.float64)
        return (out, S) if want_map else out

    # ------------------------------------------------------------------ CREPE glue
    def crepe_frames(self, audio, hop, frame0, frames, ld=1536):
        """audio [n] -> normalised, first-layer-padded frames [frames, ld] (crepe/core.py:664-703)."""
        self._chk(audio)
        out = torch.empty(frames, ld, dtype=torch.float32, device=audio.device)
        self._call("svcmi_crepe_frames_f32", _ptr(audio), audio.numel(), hop, frame0, frames, _ptr(out), ld, self._stream())
        return out

    def bn_maxpool2(self, x, scale, shift, out16=None):
        """x [B, T, C] (T even) -> max over row pairs of x*scale + shift: [B, T/2, C] (crepe/model.py:128-134).  ``out16``: also return
        the 16-bit copy (torch.bfloat16 | torch.float16 | SPLIT16) the next layer's GEMM reads."""
        self._chk(x, scale, shift)
        B, T, Cc = x.shape
        y = torch.empty(B, T // 2, Cc, dtype=torch.float32, device=x.device)
        y16 = _alloc16((B, T // 2), Cc, out16, x.device) if out16 is not None else None
        self._call("svcmi_bn_maxpool2_f32", _ptr(x), _ptr(scale), _ptr(shift), _ptr(y), B * (T // 2), Cc, x.stride(1), y.stride(1),
                   _ptr(y16), y16.stride(1) if y16 is not None else 0, _fmt16(out16) if out16 is not None else 0,
                   self._stream(), work={"bytes": 6.0 * B * T * Cc})
        return y if out16 is None else (y, y16)

    def act16_format(self):
        """The 16-bit activation format of the current precision mode (``out16`` of the producers), None in fp32 (f16w2 = fp16 rows, as
        fmt16_of() on the C side)."""
        return {PREC_BF16: torch.bfloat16, PREC_F16: torch.float16, _lib.PREC_F16W2: torch.float16, PREC_BF16X3: SPLIT16}.get(self.precision)

    def viterbi_decode(self, prob, log_trans, batch_frames, minidx, maxidx, band=0, return_loglik=False):
        """prob [frames, 360] (sigmoid outputs), log_trans [360, 360] float64 -> decoded bins int32 [frames].
        ``band`` > 0: entries with |i - j| > band are one constant (see ``transition_band``).
        ``return_loglik``: also return the per-frame log-likelihoods the dynamic programme read, fp32 [frames, 360] (tests)."""
        self._chk(prob, log_trans)
        Fr = prob.shape[0]
        lp = torch.empty(Fr * 360, dtype=torch.float32, device=prob.device)
        ptr = torch.empty(Fr * 360, dtype=torch.int16, device=prob.device)
        path = torch.empty(Fr, dtype=torch.int32, device=prob.device)
        self._call("svcmi_viterbi_decode", _ptr(prob), _ptr(log_trans), _ptr(lp), _ptr(ptr), _ptr(path), Fr, batch_frames,
                   minidx, maxidx, band, self._stream())
        return (path, lp.view(Fr, 360)) if return_loglik else path

    # ------------------------------------------------------------------ feature retrieval
    def row_sqnorm(self, x):
        """x [rows, d] -> [rows] squared L2 norms."""
        self._chk(x)
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        self._call("svcmi_row_sqnorm_f32", _ptr(x), x.stride(0), x.shape[0], x.shape[1], _ptr(out), self._stream())
        return out

    def knn_blend(self, x, bank, dots, bank_sq, k, ratio, out=None):
        """x [t, d], bank [n, d], dots [t, >= n] = x @ bank.T -> (1 - ratio) * x + ratio * weighted k-NN mean."""
        self._chk(x, bank, dots, bank_sq, out)
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        self._call("svcmi_knn_blend_f32", _ptr(x), x.stride(0), _ptr(bank), bank.stride(0), _ptr(dots), dots.stride(0),
                   _ptr(bank_sq), _ptr(out), out.stride(0), x.shape[0], bank.shape[0], x.shape[1], k, ratio, self._stream())
        return out

    def ivf_assign(self, x, dots, cent_sq, want_dist=False):
        """x [t, d], dots [t, >= nlist] = x @ centroids.T -> int32 [t] nearest centroid (+ its BLAS-form distance)."""
        self._chk(x, dots, cent_sq)
        t = x.shape[0]
        assign = torch.empty(t, dtype=torch.int32, device=x.device)
        dist = torch.empty(t, dtype=torch.float32, device=x.device) if want_dist else None
        self._call("svcmi_ivf_assign_f32", _ptr(x), x.stride(0), _ptr(dots), dots.stride(0), _ptr(cent_sq), t, cent_sq.shape[0],
                   x.shape[1], _ptr(assign), _ptr(dist) if want_dist else 0, self._stream())
        return (assign, dist) if want_dist else assign

    def ivf_blend(self, x, assign, list_off, bank, k, ratio, out=None, want_neighbours=False):
        """x [t, d], assign int32 [t], list_off int32 [nlist + 1], bank [n, d] grouped by cell -> blended [t, d]
        (+ int32 [t, k] bank rows, float [t, k] distances)."""
        self._chk(x, bank, out)
        t = x.shape[0]
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        idx = torch.empty(t, k, dtype=torch.int32, device=x.device) if want_neighbours else None
        dist = torch.empty(t, k, dtype=torch.float32, device=x.device) if want_neighbours else None
        self._call("svcmi_ivf_blend_f32", _ptr(x), x.stride(0), _ptr(assign), _ptr(list_off), _ptr(bank), bank.stride(0), _ptr(out),
                   out.stride(0), t, x.shape[1], k, ratio, _ptr(idx) if want_neighbours else 0, _ptr(dist) if want_neighbours else 0,
                   self._stream())
        return (out, idx, dist) if want_neighbours else out

    def segment_mean(self, x, order, seg_off, out):
        """out[c] = mean of x[order[seg_off[c]:seg_off[c+1]]] (empty segments untouched)."""
        self._chk(x, out)
        self._call("svcmi_segment_mean_f32", _ptr(x), x.stride(0), _ptr(order), _ptr(seg_off), _ptr(out), out.stride(0),
                   seg_off.shape[0] - 1, x.shape[1], self._stream())
        return out

    def source2wav(self, x):
        self._chk(x)
        x = x.contiguous()
        out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
        self._call("svcmi_source2wav_i16", _ptr(x), _ptr(out), x.numel(), self._stream())
        return out

    # ------------------------------------------------------------------ flow / prior glue
    def wn_gate(self, a, out=None, bias=None):
        """a [B, T, 2H] -> tanh(a[..., :H]) * sigmoid(a[..., H:]); or a [B, S, T, 2H] = split-K slabs of the in_layer
        convolution (``conv(partials=True)``) summed here together with ``bias``."""
        self._chk(a, out, bias)
        if a.dim() == 4:
            B, S, T, H2 = a.shape
            assert a.is_contiguous()
        else:
            (B, T, H2), S = a.shape, 1
            assert a.stride(0) == T * a.stride(1)
        H = H2 // 2
        if out is None:
            out = torch.empty(B, T, H, dtype=torch.float32, device=a.device)
        self._call("svcmi_wn_gate_f32", _ptr(a), _ptr(bias), _ptr(out), B, T, H, a.stride(-2), out.stride(1), S, self._stream())
        return out

    def wn_update(self, rs, x, skip, lengths, first, last):
        self._chk(rs, x, skip, lengths)
        B, T, H = skip.shape
        self._call("svcmi_wn_update_f32", _ptr(rs), _ptr(x), _ptr(skip), _ptr(lengths), B, T, H, rs.stride(1),
                   int(first), int(last), self._stream())

    def coupling_pre(self, x, x0_off, ms_vs, lengths, half):
        self._chk(x, ms_vs, lengths)
        B, T, _ = x.shape
        out = torch.empty(B, T, half, dtype=torch.float32, device=x.device)
        self._call("svcmi_coupling_pre_f32", _ptr(x), x.stride(1), x0_off, _ptr(ms_vs), _ptr(out), half, _ptr(lengths),
                   B, T, half, self._stream())
        return out

    def coupling_post(self, x, x1_off, m, ms_vs, lengths, half):
        self._chk(x, m, ms_vs, lengths)
        B, T, _ = x.shape
        self._call("svcmi_coupling_post_f32", _ptr(x), x.stride(1), x1_off, _ptr(m), m.stride(1), _ptr(ms_vs),
                   _ptr(lengths), B, T, half, self._stream())

    def embed_pitch(self, x, pit, emb, lengths):
        self._chk(x, pit, emb, lengths)
        B, T, Cc = x.shape
        self._call("svcmi_embed_pitch_f32", _ptr(x), x.stride(1), _ptr(pit), _ptr(emb), _ptr(lengths), B, T, Cc, self._stream())

    def sample_prior(self, stats, noise_ncl, lengths):
        self._chk(stats, noise_ncl, lengths)
        B, T, I2 = stats.shape
        I = I2 // 2
        z = torch.empty(B, T, I, dtype=torch.float32, device=stats.device)
        self._call("svcmi_sample_prior_f32", _ptr(stats), stats.stride(1), _ptr(noise_ncl), _ptr(lengths), _ptr(z), I,
                   B, T, I, self._stream())
        return z

    def ncl_to_nlc(self, x, add=None, add_scale=0.0, ld=None):
        self._chk(x, add)
        B, Cc, T = x.shape
        ld = ld or Cc
        y = torch.empty(B, T, ld, dtype=torch.float32, device=x.device) if ld == Cc else \
            torch.zeros(B, T, ld, dtype=torch.float32, device=x.device)
        self._call("svcmi_ncl_to_nlc_f32", _ptr(x), _ptr(add), float(add_scale), _ptr(y), B, Cc, T, ld, self._stream())
        return y

    def nlc_to_ncl(self, x, c=None):
        self._chk(x)
        B, T, ld = x.shape
        c = c or ld
        y = torch.empty(B, c, T, dtype=torch.float32, device=x.device)
        self._call("svcmi_nlc_to_ncl_f32", _ptr(x), x.stride(1), _ptr(y), B, c, T, self._stream())
        return y
