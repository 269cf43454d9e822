"""Checks of the checkpoint-scoring kernels (csrc/spectral_loss.hip: the fused STFT pair distance, the mel projection + log, the
|a - b| sum), shared by the emulator tests (CPU) and the GPU tests like tests/spectrogram_cases.py: every function takes ``ops`` and
``device``.  Oracles: CPU ``torch.stft`` and matmul in float64.

Pair inputs: y = 0.5-amplitude 220 Hz tone + 0.05 white noise with the first quarter exactly zero (spectrogram_cases.tone_noise); x = 0.8
times the same recipe at 233 Hz from another seed.  The two differ everywhere, and the silent quarter sits on the 1e-7 floor in both.

Tolerance of the three sums of svcmi_stft_distance_f32 and of svcmi_abs_diff_sum_f32: relative error <= 1e-5 against the float64 oracle.
Not a per-element worst case (propagated through log near the floor it exceeds the sums themselves and would pin nothing): on exactly
these inputs the reference recipe itself, torch.stft in fp32 on a CPU, is within 7e-7 of the float64 oracle on every sum at every shape
below, and the faults guarded against (a dropped or doubled tile, an unmasked padding row or column, the wrong floor) move a sum by
1e-2 or more.  Worst measured relative error of the three sums per shape (n_fft, hop, win, n):

    shape                          emulator     MI355X
    (64, 16, 48, 200)              7.7e-07      7.7e-07
    (512, 50, 240, 1500)           1.5e-07      1.5e-07
    (1024, 120, 600, 8057)         3.9e-08      4.9e-08
    (2048, 240, 1200, 4000)        6.8e-07      6.8e-07
    (4096, 480, 2400, 6000)        3.7e-07      3.7e-07
    (64, 7, 64, 300)               7.0e-08      7.0e-08
    10 s item, worst of the four   -            8.2e-08      (configs/base.yaml's resolutions at n = 320000)

The two columns differ only where the device's logf rounds another way than the host's (the DFT and the sums are the same fmaf chains).
svcmi_abs_diff_sum_f32: at most 6.8e-08 on both; svcmi_log_mel_f32: at most 0.115 of its bound on both (0.057 at configs/base.yaml's shape).

Bound of svcmi_log_mel_f32, per element, derived as in spectrogram_cases.py.  With u = 2^-24, bs[k, t] = sqrt(2) (n_fft + 2) u A[t] + 4 u
spec[k, t] the spectrogram bound of that file (it holds for any eps: d sqrt(re^2 + im^2 + eps) / d re <= 1), v = sum_k mel[m, k] spec[k, t]:

    dv             <=  sum_k mel[m, k] bs[k, t]  +  (bins + 2) u v         (the input's error; any-order fp32 accumulation of `bins` products)
    |out - oracle| <=  dv / max(v - dv, clip)  +  4 u |oracle|             (log's slope on the segment, clamped where the clamp is; logf)

A silent frame (every padded sample zero) is sqrt(1e-9) in every bin, projects below the clip in every channel and must be exactly
float32(log(1e-5)).
"""
import functools
import math

import numpy as np
import torch

from tests import spectrogram_cases as S

U = 2.0 ** -24
FLOOR = 1e-7
CLIP = 1e-5
TOL = 1e-5
# (n_fft, hop, win, n), center=True
SHAPES = [(64, 16, 48, 200),                    # small, win < n_fft
          (512, 50, 240, 1500),                 # 31 frames: one short tile
          (1024, 120, 600, 120 * 67 + 17),      # 68 frames: two full tiles + 4 frames
          (2048, 240, 1200, 4000),              # the block's spans do not fit LDS: samples read from global memory
          (4096, 480, 2400, 6000),              # global span, n barely above pad
          (64, 7, 64, 300)]                     # odd hop: the LDS span without its skew
RESOLUTIONS = [(1024, 120, 600), (2048, 240, 1200), (4096, 480, 2400), (512, 50, 240)]      # configs/base.yaml: mrd.resolutions
# (n_fft, hop, win, n_mel, fmin, fmax, n)
MEL_SHAPES = [(1024, 320, 1024, 100, 50.0, 16000.0, 320 * 35 + 5),      # configs/base.yaml: 513 bins (odd), 4 row tiles (the last: 4 rows), 32 + 3 frames
              (64, 16, 64, 10, 0.0, None, 200)]
GLOBAL_SMALL = (64, 200, 64, 1000)              # 31 hop + n_fft = 6264 samples per signal: the global-memory span at a short K (structural checks)
FULL_N = 320000                                 # GPU only: 10 s at 32 kHz


def recipe(n, freq, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / S.SR
    x = 0.5 * np.sin(2 * np.pi * freq * t) + 0.05 * rng.standard_normal(n)
    x[:n // 4] = 0.0
    return (scale * x).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pair(n, seed=0):
    """(x predicted, y recorded), float32 [n] each; cached and never modified."""
    y = recipe(n, 220.0, 2 * seed + n % 1009)
    x = recipe(n, 233.0, 2 * seed + 1 + n % 1009, scale=0.8)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def magnitudes64(x32, n_fft, hop, win):
    x = torch.from_numpy(np.asarray(x32, dtype=np.float64))
    spec = torch.stft(x, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=torch.float64), center=True,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    return torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=FLOOR))          # [B, bins, frames]


@functools.lru_cache(maxsize=None)
def _oracle_cached(n, seed, n_fft, hop, win):
    x, y = pair(n, seed)
    return oracle_sums(x[None], y[None], n_fft, hop, win)[0]


def oracle_sums(x32, y32, n_fft, hop, win):
    """float64 numpy [B, 3]: the reference recipe (stft_loss.py:12-28) in float64."""
    mx, my = magnitudes64(x32, n_fft, hop, win), magnitudes64(y32, n_fft, hop, win)
    return torch.stack([((my - mx) ** 2).sum((1, 2)), (my ** 2).sum((1, 2)), (my.log() - mx.log()).abs().sum((1, 2))], 1).numpy()


def run_distance(ops, device, x, y, n_fft, hop, win):
    """x, y: numpy [B, n] or tensors on ``device`` -> float64 numpy [B, 3] through the ops layer."""
    from svcmi.vits.spectrogram import spectrogram_basis
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(device) if isinstance(x, np.ndarray) else x
    yd = torch.from_numpy(np.array(y, dtype=np.float32)).to(device) if isinstance(y, np.ndarray) else y
    out = ops.stft_distance(xd, yd, spectrogram_basis(n_fft, win, xd.device), n_fft, hop, n_fft // 2, FLOOR)
    assert out.dtype == torch.float64 and tuple(out.shape) == (xd.shape[0], 3) and str(out.device).startswith(str(device))
    return out.cpu().numpy()


def rel_errors(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all() and (want > 0).all()
    return np.abs(got - want) / want


def check_shape(ops, device, n_fft, hop, win, n):
    """The pair at one shape against the float64 oracle; returns the largest relative error of the three sums."""
    x, y = pair(n)
    got = run_distance(ops, device, x[None], y[None], n_fft, hop, win)[0]
    return float(rel_errors(got, _oracle_cached(n, 0, n_fft, hop, win)).max())


def check_self_distance(ops, device, shapes=((64, 16, 48, 200), (1024, 120, 600, 1500), GLOBAL_SMALL)):
    """distance(y, y): both signals go through the same arithmetic chain, so the first and the third sum are exactly 0.0."""
    for n_fft, hop, win, n in shapes:
        _, y = pair(n)
        got = run_distance(ops, device, y[None], y[None], n_fft, hop, win)[0]
        assert got[0] == 0.0 and got[2] == 0.0, (n_fft, got)
        assert rel_errors(got[1], _oracle_cached(n, 0, n_fft, hop, win)[1]) <= TOL


def strided_pairs(device, n):
    """Three pairs as rows of wider buffers (different strides for x and y).  Returns (x view, y view, x numpy, y numpy)."""
    ps = [pair(n, seed) for seed in (1, 2, 3)]
    xs, ys = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    bx = torch.full((3, n + 37), 7.0, dtype=torch.float32, device=device)
    by = torch.full((3, n + 5), -7.0, dtype=torch.float32, device=device)
    bx[:, :n] = torch.from_numpy(xs).to(device)
    by[:, :n] = torch.from_numpy(ys).to(device)
    vx, vy = bx[:, :n], by[:, :n]
    assert vx.stride(0) == n + 37 and vy.stride(0) == n + 5 and not vx.is_contiguous()
    return vx, vy, xs, ys


def check_batch(ops, device, n_fft=512, hop=50, win=240, n=1500):
    """batch = 3, strided: inside the tolerance, every item bit-equal to its solo run, and swapping two items swaps their results.
    Returns the largest relative error."""
    vx, vy, xs, ys = strided_pairs(device, n)
    got = run_distance(ops, device, vx, vy, n_fft, hop, win)
    worst = float(rel_errors(got, oracle_sums(xs, ys, n_fft, hop, win)).max())
    for b in range(3):
        solo = run_distance(ops, device, xs[b:b + 1], ys[b:b + 1], n_fft, hop, win)
        assert np.array_equal(got[b], solo[0]), (b, got[b], solo[0])
    order = [2, 1, 0]
    swapped = run_distance(ops, device, xs[order], ys[order], n_fft, hop, win)
    assert np.array_equal(swapped, got[order])
    assert not np.array_equal(got[0], got[2])                                  # the items do differ: the check compares something
    return worst


# ------------------------------------------------------------------------------------------------ |a - b| sum
ABS_COUNTS = [(5,), (4096,), (4097,), (100, 35), (3 * 4096 + 17,)]             # one partial block, exactly one, one + 1 element, a [mel, frames] item, 4 blocks


def check_abs_diff(ops, device, shape):
    """batch 3 with different batch strides for a and b; returns the largest relative error against the float64 sum."""
    rng = np.random.default_rng(int(np.prod(shape)))
    a = rng.standard_normal((3,) + shape).astype(np.float32)
    b = (a + rng.standard_normal((3,) + shape) * np.array([1.0, 1e-3, 10.0]).reshape((3,) + (1,) * len(shape))).astype(np.float32)
    ba = torch.zeros((4,) + shape, dtype=torch.float32, device=device)
    bb = torch.zeros((6,) + shape, dtype=torch.float32, device=device)
    ba[:3] = torch.from_numpy(a).to(device)
    bb[::2] = torch.from_numpy(b).to(device)
    va, vb = ba[:3], bb[::2]
    got = ops.abs_diff_sum(va, vb)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,)
    got = got.cpu().numpy()
    want = np.abs(a.astype(np.float64) - b.astype(np.float64)).reshape(3, -1).sum(1)
    for i in range(3):
        solo = ops.abs_diff_sum(torch.from_numpy(a[i:i + 1]).to(device), torch.from_numpy(b[i:i + 1]).to(device)).cpu().numpy()
        assert solo[0] == got[i], i
    return float(rel_errors(got, want).max())


# ------------------------------------------------------------------------------------------------ mel projection + log
def mel_filterbank64(n_fft, n_mel, fmin, fmax):
    from svcmi.whisper.audio import slaney_mel_filterbank
    return slaney_mel_filterbank(S.SR, n_fft, n_mel, fmin, fmax).astype(np.float64)      # the float32 values the kernel reads


def mel_oracle(x32, n_fft, hop, win, n_mel, fmin, fmax):
    """x32 [B, n] -> (float64 reference [B, n_mel, frames], per-element bound, silent-frame mask [B, frames])."""
    x = torch.from_numpy(np.asarray(x32, dtype=np.float64))
    pad = S.pad_of(n_fft, hop)
    xp = torch.nn.functional.pad(x.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    w = torch.hann_window(win, dtype=torch.float64)
    spec = torch.stft(xp, n_fft, hop_length=hop, win_length=win, window=w, center=False, normalized=False, onesided=True, return_complex=True)
    spec = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    wp = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win) // 2
    wp[left:left + win] = w
    a = (xp.abs().unfold(1, n_fft, hop) * wp).sum(-1)                                   # [B, frames]
    bs = math.sqrt(2.0) * (n_fft + 2) * U * a[:, None, :] + 4 * U * spec
    mel = torch.from_numpy(mel_filterbank64(n_fft, n_mel, fmin, fmax))
    v = mel @ spec
    dv = mel @ bs + (spec.shape[1] + 2) * U * v
    ref = torch.log(torch.clamp(v, min=CLIP))
    bound = dv / torch.clamp(v - dv, min=CLIP) + 4 * U * ref.abs()
    silent = xp.abs().unfold(1, n_fft, hop).amax(-1) == 0
    return ref.numpy(), bound.numpy(), silent.numpy()


def run_mel(ops, device, x, n_fft, hop, win, n_mel, fmin, fmax):
    from svcmi.vits_extend.stft import TacotronSTFT
    stft = TacotronSTFT(n_fft, hop, win, n_mel, S.SR, fmin, fmax, device=device, ops=ops)
    return stft.mel_spectrogram(torch.from_numpy(x).to(device) if isinstance(x, np.ndarray) else x)


def check_mel(ops, device, n_fft, hop, win, n_mel, fmin, fmax, n):
    """Every element inside the derived bound, silent frames exactly float32(log(1e-5)); returns the largest error / bound."""
    x = np.stack([S.tone_noise(n, seed=n % 1009), S.tone_noise(n, seed=3)[::-1].copy()])
    out = run_mel(ops, device, x, n_fft, hop, win, n_mel, fmin, fmax)
    ref, bound, silent = mel_oracle(x, n_fft, hop, win, n_mel, fmin, fmax)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == ref.shape == (2, n_mel, S.frames_of(n_fft, hop, n))
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(err).all()
    assert silent[0].sum() >= 1 and not silent.all()
    log_clip = np.float32(np.log(np.float64(np.float32(CLIP))))
    assert (got.transpose(0, 2, 1)[silent] == log_clip).all(), "a silent frame is not exactly log(1e-5)"
    assert (got > log_clip).any()
    return float((err / bound).max())


# ------------------------------------------------------------------------------------------------ argument checks
@functools.lru_cache(maxsize=None)
def _valid_call():
    n_fft, hop, n = 64, 16, 200
    return n_fft, hop, n_fft // 2, n, 1 + n // hop


def check_argument_validation(ops, device):
    """Each error case returns its code and leaves the output AND the workspace untouched; the unchanged call launches and fills both."""
    from svcmi.vits.spectrogram import spectrogram_basis
    n_fft, hop, pad, n, frames = _valid_call()
    x, y = (torch.from_numpy(a.copy()).to(device).view(1, n) for a in pair(n))
    basis = spectrogram_basis(n_fft, n_fft, device)
    need = ops.stft_distance_workspace(1, n, n_fft, hop, pad)
    assert need == 3 * ((frames + 31) // 32) * ((n_fft // 2 + 1 + 63) // 64)            # the documented formula
    ws = torch.full((need,), -5.0, dtype=torch.float32, device=device)
    out = torch.full((1, 3), -5.0, dtype=torch.float64, device=device)
    f = ops.lib.svcmi_stft_distance_f32
    st = ops._stream()
    xp, yp, bp, wp, op, wb = x.data_ptr(), y.data_ptr(), basis.data_ptr(), ws.data_ptr(), out.data_ptr(), 4 * need
    EINVAL, EALIGN = -1, -3
    cases = {
        "null x": ((None, n, yp, n, 1, n, bp, n_fft, hop, pad, FLOOR, frames, wp, wb, op, st), EINVAL),
        "null y": ((xp, n, None, n, 1, n, bp, n_fft, hop, pad, FLOOR, frames, wp, wb, op, st), EINVAL),
        "null basis": ((xp, n, yp, n, 1, n, None, n_fft, hop, pad, FLOOR, frames, wp, wb, op, st), EINVAL),
        "null workspace": ((xp, n, yp, n, 1, n, bp, n_fft, hop, pad, FLOOR, frames, None, wb, op, st), EINVAL),
        "null out": ((xp, n, yp, n, 1, n, bp, n_fft, hop, pad, FLOOR, frames, wp, wb, None, st), EINVAL),
        "batch < 1": ((xp, n, yp, n, 0, n, bp, n_fft, hop, pad, FLOOR, frames, wp, wb, op, st), EINVAL),
        "n <= pad": ((xp, n, yp, n, 1, pad, bp, n_fft, hop, pad, FLOOR, 1 + pad // hop, wp, wb, op, st), EINVAL),
        "hop < 1": ((xp, n, yp, n, 1, n, bp, n_fft, 0, pad, FLOOR, frames, wp, wb, op, st), EINVAL),
        "n_fft odd": ((xp, n, yp, n, 1, n, bp, n_fft - 1, hop, pad, FLOOR, 1 + (n + 2 * pad - (n_fft - 1)) // hop, wp, wb, op, st), EINVAL),
        "pad < 0": ((xp, n, yp, n, 1, n, bp, n_fft, hop, -1, FLOOR, frames, wp, wb, op, st), EINVAL),
        "another frame count": ((xp, n, yp, n, 1, n, bp, n_fft, hop, pad, FLOOR, frames + 1, wp, wb, op, st), EINVAL),
        "floor 0": ((xp, n, yp, n, 1, n, bp, n_fft, hop, pad, 0.0, frames, wp, wb, op, st), EINVAL),
        "workspace too small": ((xp, n, yp, n, 1, n, bp, n_fft, hop, pad, FLOOR, frames, wp, wb - 4, op, st), EINVAL),
        "y stride shorter than a row": ((xp, n, yp, n - 1, 2, n, bp, n_fft, hop, pad, FLOOR, frames, wp, 2 * wb, op, st), EINVAL),
        "misaligned x": ((xp + 2, n, yp, n, 1, n, bp, n_fft, hop, pad, FLOOR, frames, wp, wb, op, st), EALIGN),
        "misaligned out": ((xp, n, yp, n, 1, n, bp, n_fft, hop, pad, FLOOR, frames, wp, wb, op + 4, st), EALIGN),
    }
    for name, (args, code) in cases.items():
        assert f(*args) == code, name
    if ops.on_gpu:
        torch.cuda.synchronize()
    assert bool((out == -5.0).all()) and bool((ws == -5.0).all()), "an error case wrote to the output or the workspace"
    assert f(xp, n, yp, n, 1, n, bp, n_fft, hop, pad, FLOOR, frames, wp, wb, op, st) == 0
    if ops.on_gpu:
        torch.cuda.synchronize()
    assert bool((out >= 0).all()) and bool((ws >= 0).all())
    assert np.array_equal(out.cpu().numpy(), run_distance(ops, device, x, y, n_fft, hop, n_fft))

    # log_mel and abs_diff_sum: the same promise
    spec = torch.rand(1, 33, 12, dtype=torch.float32, device=device)
    melT = torch.rand(33, 32, dtype=torch.float32, device=device)
    mo = torch.full((1, 10, 12), -5.0, dtype=torch.float32, device=device)
    g = ops.lib.svcmi_log_mel_f32
    sp, mp, mop = spec.data_ptr(), melT.data_ptr(), mo.data_ptr()
    assert g(None, 1, 33, 12, mp, 32, 10, CLIP, mop, st) == EINVAL and g(sp, 1, 33, 12, None, 32, 10, CLIP, mop, st) == EINVAL
    assert g(sp, 1, 33, 12, mp, 32, 10, CLIP, None, st) == EINVAL and g(sp, 0, 33, 12, mp, 32, 10, CLIP, mop, st) == EINVAL
    assert g(sp, 1, 33, 0, mp, 32, 10, CLIP, mop, st) == EINVAL and g(sp, 1, 33, 12, mp, 31, 10, CLIP, mop, st) == EINVAL      # ldm < 32
    assert g(sp, 1, 33, 12, mp, 32, 33, CLIP, mop, st) == EINVAL                                                                   # 33 rows need ldm 64
    assert g(sp, 1, 33, 12, mp, 32, 10, 0.0, mop, st) == EINVAL and g(sp, 1, 33, 12, mp, 32, 10, CLIP, mop + 2, st) == EALIGN
    h = ops.lib.svcmi_abs_diff_sum_f32
    ao = torch.full((1,), -5.0, dtype=torch.float64, device=device)
    aw = torch.full((1,), -5.0, dtype=torch.float32, device=device)
    aop, awp = ao.data_ptr(), aw.data_ptr()
    assert ops.lib.svcmi_abs_diff_sum_workspace_bytes(1, 396) == 4 and ops.lib.svcmi_abs_diff_sum_workspace_bytes(3, 4097) == 24
    assert h(None, 396, sp, 396, 1, 396, awp, 4, aop, st) == EINVAL and h(sp, 396, None, 396, 1, 396, awp, 4, aop, st) == EINVAL
    assert h(sp, 396, sp, 396, 1, 396, None, 4, aop, st) == EINVAL and h(sp, 396, sp, 396, 1, 396, awp, 4, None, st) == EINVAL
    assert h(sp, 396, sp, 396, 1, 0, awp, 4, aop, st) == EINVAL and h(sp, 396, sp, 396, 1, 396, awp, 0, aop, st) == EINVAL
    assert h(sp, 396, sp, 100, 2, 198, awp, 8, aop, st) == EINVAL and h(sp, 396, sp, 396, 1, 396, awp, 4, aop + 4, st) == EALIGN
    if ops.on_gpu:
        torch.cuda.synchronize()
    assert bool((mo == -5.0).all()) and bool((ao == -5.0).all()) and bool((aw == -5.0).all())
    assert g(sp, 1, 33, 12, mp, 32, 10, CLIP, mop, st) == 0 and h(sp, 396, mp, 396, 1, 396, awp, 4, aop, st) == 0
    if ops.on_gpu:
        torch.cuda.synchronize()
    assert bool((mo > -5.0).all()) and float(ao[0]) > 0
