"""Checks of the GPU wav loader (csrc/resample.hip: PCM decode + downmix + polyphase resampling in one launch), shared by the
emulator tests (CPU) and the GPU tests like tests/kernel_cases.py: every function takes ``ops`` and ``device``.

Oracle: ``scipy.signal.resample_poly`` in float64 on the host-decoded, downmixed signal (what ``load_audio`` feeds its resampler).
Tolerance, derived and not tuned: the kernel rounds each tap to fp32 (relative 2^-24) and accumulates K products in fp32 (each
product and each sum: relative 2^-24 of a partial result bounded by sum |h x|), so in any order, with or without FMA,

    |y[m] - ref[m]|  <=  (K + 2) * 2^-24 * sum_k |h[p + k up] x[j - k]|

The right-hand side is itself a resampling: ``resample_poly(|x|, up, down, window=|firwin taps|)`` (scipy scales an explicit tap
array by ``up`` like its default design).  An indexing error is O(1e-2) of the signal; every output is checked.
"""
import functools
import math
import os

import numpy as np
import torch

SR = 16000
# (from, to): up / down after the gcd; the last one has 16000 phases -- its tap image does not fit LDS and is read from global memory
RATE_PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (16000, 32000), (47999, 16000)]
# format x channels; fmt codes of svcmi_pcm_resample_f32
FORMATS = [("int16", 1), ("int16", 2), ("int32", 2), ("uint8", 1), ("float32", 3)]
FMT = {"float32": 0, "int16": 1, "int32": 2, "uint8": 3}
TILE = 1024          # outputs per block of the kernel at these ratios: sizes below are chosen around its seams
FRAMES = (1, 7, 441, 4411)


def ratio(rate_from, rate_to):
    g = math.gcd(rate_from, rate_to)
    return rate_to // g, rate_from // g


def mid_tile_frames(up, down):
    """An input length whose output ends in the middle of the third tile."""
    return -(-(2 * TILE + 300) * down // up)


def make_pcm(dtype, channels, frames, seed):
    """Seeded uniform [-1, 1) (or the integer equivalent) as interleaved frames [frames, channels] ([frames] for mono, like a wav file)."""
    rng = np.random.default_rng(seed)
    shape = (frames,) if channels == 1 else (frames, channels)
    if dtype == "float32":
        return rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    if dtype == "uint8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    info = np.iinfo(dtype)
    return rng.integers(info.min, int(info.max) + 1, shape, dtype=dtype)


def host_decode(x):
    """The decode + downmix of svcmi.whisper.audio.load_audio, verbatim."""
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    elif x.dtype.kind == "u":
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = x.astype(np.float32)
    if x.ndim > 1:
        x = x.mean(axis=1)
    return x


@functools.lru_cache(maxsize=None)
def abs_firwin(up, down):
    from scipy.signal import firwin
    half = 10 * max(up, down)
    return np.abs(firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0))), half


def oracle(x32, up, down):
    """(fp64 reference, per-output bound) for the downmixed float32 signal."""
    from scipy.signal import resample_poly
    x64 = x32.astype(np.float64)
    ref = resample_poly(x64, up, down)
    habs, half = abs_firwin(up, down)
    k = -(-(2 * half + 1) // up)
    bound = (k + 2) * 2.0 ** -24 * resample_poly(np.abs(x64), up, down, window=habs)
    return ref, bound


def run_kernel(ops, device, x, up, down):
    from svcmi.whisper import audio as A
    channels = 1 if x.ndim == 1 else x.shape[1]
    taps, half = A.resample_taps(up, down, device)
    return ops.pcm_resample(torch.from_numpy(x).to(device), FMT[x.dtype.name], channels, taps, up, down, half)


def check_rate_pair(ops, device, rate_from, rate_to):
    """Every output of every (length, format x channels) case of one rate pair inside the derived bound; returns the largest
    error / bound ratio seen."""
    up, down = ratio(rate_from, rate_to)
    worst = 0.0
    for frames in FRAMES + (mid_tile_frames(up, down),):
        for i, (dtype, channels) in enumerate(FORMATS):
            x = make_pcm(dtype, channels, frames, seed=1000 * i + frames % 997)
            y = run_kernel(ops, device, x, up, down)
            ref, bound = oracle(host_decode(x), up, down)
            assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape == (-(-frames * up // down),), (y.shape, ref.shape)
            err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
            bad = np.nonzero(err > bound)[0]
            assert bad.size == 0, (rate_from, rate_to, frames, dtype, channels, int(bad[0]), float(err[bad[0]]), float(bound[bad[0]]))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 values, exactly: the product and the sum as integers, rounded once to 24 bits (nearest even).
    (No subnormal handling: the test's partial sums are far above 2^-126.)"""
    from fractions import Fraction
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        return np.float32(0.0)
    n, s = abs(v.numerator), v.denominator.bit_length() - 1          # |v| = n / 2^s: every float is a dyadic rational
    shift = n.bit_length() - 24
    if shift > 0:
        q, rem = n >> shift, n & ((1 << shift) - 1)
        if rem > (1 << (shift - 1)) or (rem == (1 << (shift - 1)) and (q & 1)):
            q += 1
    else:
        q, shift = n, 0
    r = math.ldexp(q, shift - s)
    return np.float32(-r if v < 0 else r)


def check_fma_chain_bits(ops, device):
    """Both tap paths -- the image in LDS (44.1 kHz: 160 phases) and in global memory (47999 Hz: 16000 phases) -- give the bits of the
    specified arithmetic: an fmaf chain in ascending k over the fp32 image, evaluated here exactly.  So they also agree with each
    other, whatever the tile or the grid."""
    from svcmi.whisper import audio as A
    for (rate_from, rate_to) in ((44100, 16000), (47999, 16000)):
        up, down = ratio(rate_from, rate_to)
        frames = 300
        x = make_pcm("int16", 1, frames, seed=5)
        y = run_kernel(ops, device, x, up, down).cpu().numpy()
        taps, half = A.resample_taps(up, down, "cpu")
        t, x32 = taps.numpy(), host_decode(x)
        want = np.zeros(y.shape[0], dtype=np.float32)
        for m in range(y.shape[0]):
            c = m * down + half
            p, j = c % up, c // up
            acc = np.float32(0.0)
            for k in range(t.shape[1]):
                acc = _fma32(x32[j - k] if 0 <= j - k < frames else 0.0, t[p, k], acc)
            want[m] = acc
        assert np.array_equal(y, want), (rate_from, float(np.abs(y - want).max()))


def write_wavs(tmpdir, rate, frames=4411, seed0=77):
    """One wav file per format x channels combination at ``rate``; returns the paths."""
    from scipy.io import wavfile
    paths = []
    for i, (dtype, channels) in enumerate(FORMATS):
        path = os.path.join(str(tmpdir), f"pcm_{rate}_{dtype}_{channels}.wav")
        wavfile.write(path, rate, make_pcm(dtype, channels, frames, seed=seed0 + i))
        paths.append(path)
    return paths


def check_decode_only(ops, device, tmpdir):
    """16 kHz files: ``pcm_resample(up = down = 1, taps = None)`` and ``load_audio_device`` against ``load_audio``, bit for bit."""
    from scipy.io import wavfile
    from svcmi.whisper import audio as A
    for path in write_wavs(tmpdir, SR):
        want = A.load_audio(path)
        rate, x = wavfile.read(path)
        assert rate == SR
        channels = 1 if x.ndim == 1 else x.shape[1]
        got = ops.pcm_resample(torch.from_numpy(np.array(x)).to(device), FMT[x.dtype.name], channels, None, 1, 1, 0)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want), path
        assert np.array_equal(A.load_audio_device(path, device=device, ops=ops).cpu().numpy(), want), path


def check_loader_against_host(ops, device, path):
    """``load_audio_device`` against ``load_audio`` on one file: each is within the bound of the fp64 reference, so they are within
    twice the bound of each other (scipy's own float32 path: the same count of fp32 operations per output)."""
    from scipy.io import wavfile
    from svcmi.whisper import audio as A
    rate, x = wavfile.read(path)
    up, down = ratio(rate, SR)
    got = A.load_audio_device(path, device=device, ops=ops)
    want = A.load_audio(path)
    assert got.dtype == torch.float32 and str(got.device).startswith(str(device)) and tuple(got.shape) == want.shape
    ref, bound = oracle(host_decode(np.array(x)), up, down)
    g = got.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(g - ref) <= bound), float((np.abs(g - ref) / np.maximum(bound, 1e-300)).max())
    assert np.all(np.abs(g - want.astype(np.float64)) <= 2 * bound)
    return got
