"""Checks of the key sweep (csrc/sweep.hip, svcmi_synth_sweep_fwd, svc_infer_sweep, svcmi.svc_inference_shift), shared by the emulator
tests (CPU) and the GPU tests.  The references are the solo path itself (``svc_infer`` on the transposed track: a sweep must give what a
loop over keys gives) and, for one key, the CPU oracle."""
import functools

import numpy as np
import torch

from oracle import svc_oracle as O
from tests import engine_cases as E
from workload import config as C
from workload import inputs as I

KEYS = (-12, -7, 0, 5, 12)
BATCH_TOL = 1e-5          # a batch against its solo runs: test_equal_length_batch_reproduces_solo_runs (batch size selects tile / split-K policies)


def factor(s):
    return 2 ** (s / 12)


def expected_pitch(pit, s):
    """svc_inference_shift.py:63-65: float64 product, then FloatTensor."""
    return torch.FloatTensor(np.asarray(pit, np.float64) * 2 ** (s / 12))


def pitch_values(t):
    """0 (unvoiced), the clamp pitches, integers as the CSV gives them, a few non-integers; cycled to t values."""
    base = [0.0, 30.0, 440.0, 1000.0, 187.0, 233.0, 96.0, 523.0, 261.6255653, 99.99999, 0.1, 700.5, 1.0e-3, 333.3333, 65.40639]
    return [base[i % len(base)] + (i // len(base)) for i in range(t)]


def check_pitch_bits(ops, device, t):
    pit = torch.tensor(pitch_values(t), dtype=torch.float32)
    got = ops.sweep_pitch(pit.to(device), [factor(s) for s in KEYS]).cpu()
    assert got.shape == (len(KEYS), t) and got.dtype == torch.float32
    for k, s in enumerate(KEYS):
        want = expected_pitch(pit.numpy(), s)
        assert torch.equal(got[k], want), (s, got[k], want)
    assert torch.equal(got[KEYS.index(0)], pit)                    # shift 0 leaves the track untouched
    assert (got[:, pit == 0] == 0).all()                            # unvoiced stays unvoiced


def bin_boundaries(n=3):
    """Pairs of ADJACENT fp32 pitches whose coarse bins differ, found by bisection on the fp32 restatement of f0_to_coarse."""
    out = []
    for lo, hi in ((100.0, 110.0), (300.0, 320.0), (640.0, 700.0))[:n]:
        a, b = np.float32(lo), np.float32(hi)
        ba = int(O.f0_to_coarse(torch.tensor([a]))[0])
        assert ba != int(O.f0_to_coarse(torch.tensor([b]))[0])
        while np.nextafter(a, np.float32(np.inf)) < b:
            mid = np.float32((np.float64(a) + np.float64(b)) / 2)
            if int(O.f0_to_coarse(torch.tensor([mid]))[0]) == ba:
                a = mid
            else:
                b = mid
        out += [float(a), float(b)]
    return out


def check_embed_bits(ops, device, t, H, K):
    """sweep_embed against embed_pitch on K copies of the same xs with the rows of pit_k; masked tail (length < t where t allows)."""
    g = torch.Generator().manual_seed(100 * t + H + K)
    length = max(1, t - 5)
    xs = torch.randn(t, H, generator=g)
    emb = torch.randn(256, H, generator=g)
    shifts = [(-12, 12, 0)[k % 3] if k < 3 else ((k * 5) % 25) - 12 for k in range(K)]
    vals = [1000.0, 30.0, 0.0] + bin_boundaries() + pitch_values(t)
    pit = torch.tensor(vals[:t] if t > 1 else [1000.0], dtype=torch.float32)
    pit_k = ops.sweep_pitch(pit.to(device), [factor(s) for s in shifts])
    if t > 9:                                                       # the boundary pairs as they are, in the row of every key
        pit_k[:, 3:9] = torch.tensor(bin_boundaries(), dtype=torch.float32).to(device)
    len_d = torch.tensor([length], dtype=torch.int32).to(device)
    got = ops.sweep_embed(xs.to(device), pit_k, emb.to(device), len_d)
    want = xs.to(device).unsqueeze(0).repeat(K, 1, 1).contiguous()
    ops.embed_pitch(want, pit_k, emb.to(device), len_d.repeat(K))
    assert got.shape == (K, t, H)
    assert torch.equal(got, want)
    bins = O.f0_to_coarse(pit_k.cpu())
    if t > 2 and K >= 3:
        assert int(bins[1, 0]) == 255 and int(bins[0, 1]) == 1 and (bins[:, 2] == 1).all()      # 1000 Hz at +12, 30 Hz at -12, unvoiced
    if t > 9:
        assert all(int(bins[0, 3 + 2 * i]) != int(bins[0, 4 + 2 * i]) for i in range(3))         # the pairs straddle a bin edge
    if length < t:
        assert (got[:, length:] == 0).all()


def check_embed_strided(ops, device):
    """xs with a padded row stride (a view into a wider buffer)."""
    g = torch.Generator().manual_seed(5)
    t, H, K = 7, 8, 2
    wide = torch.randn(t, 16, generator=g).to(device)
    emb = torch.randn(256, H, generator=g).to(device)
    pit_k = ops.sweep_pitch(torch.tensor(pitch_values(t), dtype=torch.float32).to(device), [factor(-3), factor(4)])
    got = ops.sweep_embed(wide[:, :H], pit_k, emb, None)
    want = wide[:, :H].unsqueeze(0).repeat(K, 1, 1).contiguous()
    ops.embed_pitch(want, pit_k, emb, torch.tensor([t, t], dtype=torch.int32).to(device))
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ stage / driver
def sweep_noise(hp, T, K, seed):
    """The noise dict of svc_infer_sweep (leading key axis) and its per-key svc_infer dicts."""
    g = torch.Generator().manual_seed(seed)
    L = T * hp.data.hop_length
    plan = O.chunk_schedule(T, hp.data.hop_length)
    noise = {"rand_ini": torch.rand(K, 1, 11, generator=g), "src_noise": torch.randn(K, 1, L, 11, generator=g),
             "enc_noises": [torch.randn(K, 1, hp.vits.inter_channels, ce - cs, generator=g) for (cs, ce, _, _) in plan]}
    solo = [{"rand_ini": noise["rand_ini"][k], "src_noise": noise["src_noise"][k], "enc_noises": [e[k] for e in noise["enc_noises"]]}
            for k in range(K)]
    return noise, solo


@functools.lru_cache(maxsize=4)
def _clip(T, seed, base):
    hp = C.base_hp() if base else C.tiny_hp()
    d = I.synth_clip(T=T, hp=hp, seed=seed, B=1)
    d["pit"][0, : min(3, T)] = torch.tensor([0.0, 30.0, 1000.0])[: min(3, T)]      # unvoiced and the two clamp pitches, in every clip
    return hp, d


def _args(d, hp, device):
    return (d["spk"][0], d["pit"][0], d["ppg"][0], d["vec"][0], hp, device)


def solo_run(m, d, hp, device, s, noise, retrieval=None):
    """svc_infer on the transposed track of key s: the float64 product of svc_inference_shift.py, then FloatTensor."""
    from svcmi import svc_infer
    spk, pit, ppg, vec = d["spk"][0], d["pit"][0], d["ppg"][0], d["vec"][0]
    return svc_infer(m, retrieval, spk, expected_pitch(pit.numpy(), s), ppg, vec, hp, device, noise=noise, write_pit_wav=False)


def check_one_key_is_the_solo_run(ops, device, T=37):
    """K = 1, shift 0: the same launches at the same sizes as svc_infer -> the same bits."""
    from svcmi.svc_inference import svc_infer_sweep
    hp, d = _clip(T, 11, False)
    m, _ = E.make_model(hp, ops, device)
    noise, solo = sweep_noise(hp, T, 1, 3)
    got = svc_infer_sweep(m, None, *_args(d, hp, device), [0], noise=noise)
    want = solo_run(m, d, hp, device, 0, solo[0])
    assert len(got) == 1 and got[0].dtype == np.float32 and got[0].shape == want.shape == (T * hp.data.hop_length - 1,)
    err = float(np.abs(got[0] - want).max())
    print(f"sweep K=1 shift 0 vs svc_infer: max error {err:.3e}")
    assert err == 0.0


THREE = [-12, 0, 12]
_three_cache = {}


def three_keys(ops, device, T):
    """The K = 3 sweep at the default key batch and its three solo runs, computed once per (library, T) and shared by the checks below."""
    from svcmi.svc_inference import svc_infer_sweep
    key = (id(ops), device, T)
    if key not in _three_cache:
        hp, d = _clip(T, 11, False)
        m, _ = E.make_model(hp, ops, device)
        noise, solo = sweep_noise(hp, T, 3, 4)
        got = svc_infer_sweep(m, None, *_args(d, hp, device), THREE, noise=noise)
        want = [solo_run(m, d, hp, device, s, solo[k]) for k, s in enumerate(THREE)]
        _three_cache[key] = (got, want)
    return _three_cache[key]


def check_three_keys(ops, device, T=37):
    """K = 3, shifts [-12, 0, 12]: pit_k and the sources bit-equal to the solo path's, waveforms within BATCH_TOL of the solo runs, one key
    against the CPU oracle."""
    hp, d = _clip(T, 11, False)
    m, sd = E.make_model(hp, ops, device)
    shifts = THREE
    noise, solo = sweep_noise(hp, T, 3, 4)
    pit = d["pit"][0]
    pit_k = ops.sweep_pitch(pit.to(device), [factor(s) for s in shifts])
    src = m.pitch2source(pit_k, noise=(noise["rand_ini"].reshape(3, -1), noise["src_noise"].reshape(3, T * 320, -1)))
    for k, s in enumerate(shifts):
        want_pit = expected_pitch(pit.numpy(), s)
        assert torch.equal(pit_k[k].cpu(), want_pit), s
        solo_src = m.pitch2source(want_pit[None], noise=(solo[k]["rand_ini"], solo[k]["src_noise"]))
        assert torch.equal(src[k].cpu(), solo_src[0].cpu()), s
    got, want = three_keys(ops, device, T)
    errs = {s: float(np.abs(got[k] - want[k]).max()) for k, s in enumerate(shifts)}
    print(f"sweep K=3 vs solo svc_infer: {errs}")
    assert max(errs.values()) <= BATCH_TOL, errs
    # key +12 against the CPU oracle
    k = 2
    with torch.no_grad():
        p = expected_pitch(pit.numpy(), shifts[k])[None]
        o_src = O.pitch2source(sd, hp, p, solo[k]["rand_ini"], solo[k]["src_noise"])
        o_wav = O.synth_inference(sd, hp, d["ppg"], d["vec"], p, d["spk"], d["lengths"], o_src, solo[k]["enc_noises"][0])
    e_or = float(np.abs(got[k] - o_wav[0, 0, :-1].numpy()).max())
    print(f"sweep key +12 vs the CPU oracle: {e_or:.3e}")
    assert e_or <= E.WAVE_TOL, e_or


def check_grouping(ops, device, T=37):
    """K = 3 with key_batch = 2 (groups of 2 and 1): each key within BATCH_TOL of the key_batch = 3 result, the group of one bit-equal to its
    solo run."""
    from svcmi.svc_inference import svc_infer_sweep
    hp, d = _clip(T, 11, False)
    m, _ = E.make_model(hp, ops, device)
    noise, _ = sweep_noise(hp, T, 3, 4)
    whole, want = three_keys(ops, device, T)               # (the default key batch holds all three: key_batch = 3)
    split = svc_infer_sweep(m, None, *_args(d, hp, device), THREE, noise=noise, key_batch=2)
    errs = [float(np.abs(a - b).max()) for a, b in zip(whole, split)]
    print(f"sweep key_batch 2 vs 3: {errs}")
    assert max(errs) <= BATCH_TOL, errs
    assert float(np.abs(split[2] - want[2]).max()) == 0.0


def check_two_chunks(ops, device, T=2600):
    """K = 2 over the chunk seam (the length svc_infer_tiny_2chunks uses)."""
    from svcmi.svc_inference import svc_infer_sweep
    hp, d = _clip(T, 2, False)
    m, _ = E.make_model(hp, ops, device)
    shifts = [-5, 7]
    noise, solo = sweep_noise(hp, T, 2, 6)
    got = svc_infer_sweep(m, None, *_args(d, hp, device), shifts, noise=noise)
    seam = C.CHUNK_FRAMES * 320
    for k, s in enumerate(shifts):
        want = solo_run(m, d, hp, device, s, solo[k])
        assert got[k].shape == (320 * T - 1,)
        err, e_seam = float(np.abs(got[k] - want).max()), float(np.abs(got[k][seam - 3000:seam + 3000] - want[seam - 3000:seam + 3000]).max())
        print(f"sweep two chunks key {s}: max error {err:.3e} (seam {e_seam:.3e})")
        assert err <= BATCH_TOL, (s, err)


def check_retrieval_once_per_chunk(ops, device, T=90, check_changed=True):
    """K = 2 with the on-device kNN blend: each key within BATCH_TOL of solo svc_infer with the same retrieval, and the blend ran once per
    chunk, not once per key."""
    from svcmi.feature_retrieval import KnnFeatureIndex, KnnIndexRetrieval
    from svcmi.svc_inference import svc_infer_sweep
    hp, d = _clip(T, 5, False)
    m, _ = E.make_model(hp, ops, device)
    gen = torch.Generator().manual_seed(9)
    banks = {"ppg": torch.randn(400, hp.vits.ppg_dim, generator=gen).numpy(), "vec": torch.randn(333, hp.vits.vec_dim, generator=gen).numpy()}
    knn = KnnIndexRetrieval(hubert_index=KnnFeatureIndex(banks["vec"], 0.5, 3, device=device, ops=ops),
                            whisper_index=KnnFeatureIndex(banks["ppg"], 0.5, 3, device=device, ops=ops))

    class Counting:
        on_device = True
        calls = {"whisper": 0, "hubert": 0}

        def retriv_whisper(self, v):
            self.calls["whisper"] += 1
            return knn.retriv_whisper(v)

        def retriv_hubert(self, v):
            self.calls["hubert"] += 1
            return knn.retriv_hubert(v)

    shifts = [-3, 4]
    noise, solo = sweep_noise(hp, T, 2, 8)
    counting = Counting()
    got = svc_infer_sweep(m, counting, *_args(d, hp, device), shifts, noise=noise)
    n_chunks = len(O.chunk_schedule(T, 320))
    assert counting.calls == {"whisper": n_chunks, "hubert": n_chunks}, counting.calls
    plain = svc_infer_sweep(m, None, *_args(d, hp, device), shifts, noise=noise) if check_changed else None
    for k, s in enumerate(shifts):
        want = solo_run(m, d, hp, device, s, solo[k], retrieval=knn)
        err = float(np.abs(got[k] - want).max())
        print(f"sweep with retrieval key {s}: max error {err:.3e}")
        assert err <= BATCH_TOL, (s, err)
        if check_changed:
            assert float(np.abs(got[k] - plain[k]).max()) > 100 * BATCH_TOL      # the blend actually changed the features


def check_base_model(ops, device, T=200, K=16):
    """base.yaml widths at the default key batch: keys 0, 7 and 15 within BATCH_TOL of their solo runs."""
    from svcmi.svc_inference import svc_infer_sweep
    hp, d = _clip(T, 13, True)
    m, _ = E.make_model(hp, ops, device)
    shifts = list(range(-8, -8 + K))
    noise, solo = sweep_noise(hp, T, K, 10)
    got = svc_infer_sweep(m, None, *_args(d, hp, device), shifts, noise=noise, key_batch=K)
    for k in (0, 7, 15):
        want = solo_run(m, d, hp, device, shifts[k], solo[k])
        err = float(np.abs(got[k] - want).max())
        print(f"sweep base model key index {k} (shift {shifts[k]}): max error {err:.3e}")
        assert err <= BATCH_TOL, (k, err)


def check_driver_arguments(ops, device):
    import pytest
    from svcmi.svc_inference import svc_infer_sweep
    hp, d = _clip(5, 1, False)
    m, _ = E.make_model(hp, ops, device)
    for bad in (dict(shifts=[]), dict(shifts=[0], key_batch=0), dict(shifts=[0], key_batch=33)):
        with pytest.raises(ValueError):
            svc_infer_sweep(m, None, *_args(d, hp, device), **bad)
    outs = svc_infer_sweep(m, None, *_args(d, hp, device), [1, 2], return_tensor=True)      # fresh draws per key
    assert len(outs) == 2 and all(torch.is_tensor(o) and o.shape == (5 * 320 - 1,) for o in outs)
