"""Checks of the singer sweep (csrc/sweep.hip: sweep_sample_prior, svcmi_synth_singers_fwd, svc_infer_singers), shared by the emulator
tests (CPU) and the GPU tests.  The references are the solo path itself (``svc_infer`` per speaker row with the same noise: a sweep must
give what a loop over singers gives, the shared NSF excitation aside -- the solo runs are handed that same excitation) and, for one
singer, the CPU oracle."""
import functools

import numpy as np
import torch

from oracle import svc_oracle as O
from tests import engine_cases as E
from tests.sweep_cases import BATCH_TOL
from workload import config as C
from workload import inputs as I


# ------------------------------------------------------------------------------------------------ kernel
def _stats(t, i, pad, g):
    """m | logs as the projection writes them, in a buffer `pad` floats wider than 2 i; logs kept where exp stays finite."""
    wide = torch.randn(t, 2 * i + pad, generator=g)
    wide[:, i:2 * i] *= 0.7
    return wide


def check_sample_bits(ops, device, t, i, S):
    """sweep_sample_prior against sample_prior on S copies of the statistics, with length = max(1, t - 5) and with NULL; rows past the
    length exactly 0."""
    g = torch.Generator().manual_seed(1000 * t + 10 * i + S)
    stats = _stats(t, i, 0, g).to(device)
    noise = torch.randn(S, i, t, generator=g).to(device)
    copies = stats.unsqueeze(0).repeat(S, 1, 1).contiguous()
    for length in (max(1, t - 5), None):
        len_d = None if length is None else torch.tensor([length], dtype=torch.int32).to(device)
        got = ops.sweep_sample_prior(stats, noise, len_d)
        want = ops.sample_prior(copies, noise, None if length is None else len_d.repeat(S))
        assert got.shape == (S, t, i) and got.dtype == torch.float32
        assert torch.equal(got, want), (t, i, S, length, float((got - want).abs().max()))
        if length is not None and length < t:
            assert (got[:, length:] == 0).all()
            assert (got[:, :length] != 0).any()
    # the arithmetic itself, against fp64 (one fp32 rounding of the exp, one of the multiply-add)
    ref = stats[:, :i].double().cpu() + noise.double().cpu().transpose(1, 2) * stats[:, i:].double().cpu().exp()
    assert float((got.cpu().double() - ref).abs().max() / ref.abs().max().clamp(min=1.0)) < 1e-5


def check_sample_strided(ops, device, t=37, i=40, S=3):
    """stats as a view into a wider buffer (lds > 2 i)."""
    g = torch.Generator().manual_seed(77)
    wide = _stats(t, i, 24, g).to(device)
    view = wide[:, :2 * i]
    assert view.stride(0) == 2 * i + 24
    noise = torch.randn(S, i, t, generator=g).to(device)
    len_d = torch.tensor([t - 5], dtype=torch.int32).to(device)
    got = ops.sweep_sample_prior(view, noise, len_d)
    want = ops.sample_prior(view.unsqueeze(0).repeat(S, 1, 1).contiguous(), noise, len_d.repeat(S))
    assert torch.equal(got, want)
    assert torch.equal(wide[:, 2 * i:].cpu(), _stats(t, i, 24, torch.Generator().manual_seed(77))[:, 2 * i:])      # the padding is not written


def check_sample_split(ops, device, t=37, i=40):
    """S = 32 as one call and as 3 + 29: the rows-per-block policy does not reach the bits."""
    g = torch.Generator().manual_seed(78)
    stats = _stats(t, i, 0, g).to(device)
    noise = torch.randn(32, i, t, generator=g).to(device)
    len_d = torch.tensor([t - 5], dtype=torch.int32).to(device)
    whole = ops.sweep_sample_prior(stats, noise, len_d)
    parts = torch.cat([ops.sweep_sample_prior(stats, noise[:3].contiguous(), len_d), ops.sweep_sample_prior(stats, noise[3:].contiguous(), len_d)])
    assert torch.equal(whole, parts)


# ------------------------------------------------------------------------------------------------ stage / driver
def singer_rows(hp, S, seed=40):
    """S seeded randn rows at the norm of the reference's singer files, all different."""
    rows = torch.stack([I.synth_spk(hp.vits.spk_dim, seed=seed + s) for s in range(S)])
    assert all(not torch.equal(rows[a], rows[b]) for a in range(S) for b in range(a))
    return rows


def singers_noise(hp, T, S, seed):
    """The noise dict of svc_infer_singers (shared source draws, per-singer prior draws) and its per-singer svc_infer dicts."""
    g = torch.Generator().manual_seed(seed)
    L = T * hp.data.hop_length
    plan = O.chunk_schedule(T, hp.data.hop_length)
    noise = {"rand_ini": torch.rand(1, 11, generator=g), "src_noise": torch.randn(1, L, 11, generator=g),
             "enc_noises": [torch.randn(S, 1, hp.vits.inter_channels, ce - cs, generator=g) for (cs, ce, _, _) in plan]}
    solo = [{"rand_ini": noise["rand_ini"], "src_noise": noise["src_noise"], "enc_noises": [e[s] for e in noise["enc_noises"]]} for s in range(S)]
    return noise, solo


@functools.lru_cache(maxsize=4)
def _clip(T, seed, base):
    hp = C.base_hp() if base else C.tiny_hp()
    d = I.synth_clip(T=T, hp=hp, seed=seed, B=1)
    d["pit"][0, : min(3, T)] = torch.tensor([0.0, 30.0, 1000.0])[: min(3, T)]      # unvoiced and the two clamp pitches, in every clip
    return hp, d


def _args(d, hp, device):
    return (d["pit"][0], d["ppg"][0], d["vec"][0], hp, device)


def solo_run(m, d, hp, device, spk, noise, retrieval=None):
    from svcmi import svc_infer
    return svc_infer(m, retrieval, spk, *_args(d, hp, device), noise=noise, write_pit_wav=False)


class Watch:
    """The model with its calls counted and the z_p of every ``inference`` / ``inference_singers`` call kept (``return_parts`` adds one
    copy launch and changes no value)."""

    def __init__(self, model):
        self._m, self.z_p, self.calls = model, [], {"pitch2source": 0, "inference": 0, "inference_singers": 0}

    def __getattr__(self, k):
        return getattr(self._m, k)

    def pitch2source(self, *a, **k):
        self.calls["pitch2source"] += 1
        return self._m.pitch2source(*a, **k)

    def inference(self, *a, **k):
        self.calls["inference"] += 1
        out, parts = self._m.inference(*a, return_parts=True, **k)
        self.z_p.append(parts["z_p"].cpu())
        return out

    def inference_singers(self, *a, **k):
        self.calls["inference_singers"] += 1
        out, parts = self._m.inference_singers(*a, return_parts=True, **k)
        self.z_p.append(parts["z_p"].cpu())
        return out


def check_one_singer_is_the_solo_run(ops, device, T=37):
    """S = 1: the launches of svc_infer at the same sizes (the sample through the fan-out kernel) -> the same bits."""
    from svcmi.svc_inference import svc_infer_singers
    hp, d = _clip(T, 11, False)
    m, _ = E.make_model(hp, ops, device)
    spks = singer_rows(hp, 1)
    noise, solo = singers_noise(hp, T, 1, 3)
    got = svc_infer_singers(m, None, spks, *_args(d, hp, device), noise=noise)
    want = solo_run(m, d, hp, device, spks[0], solo[0])
    assert len(got) == 1 and got[0].dtype == np.float32 and got[0].shape == want.shape == (T * hp.data.hop_length - 1,)
    err = float(np.abs(got[0] - want).max())
    print(f"singers S=1 vs svc_infer: max error {err:.3e}")
    assert err == 0.0


_three_cache = {}


def three_singers(ops, device, T):
    """The S = 3 sweep in one group and its three solo runs (waveforms, z_p, call counts), computed once per (library, T) and shared."""
    from svcmi.svc_inference import svc_infer_singers
    key = (id(ops), device, T)
    if key not in _three_cache:
        hp, d = _clip(T, 11, False)
        m, _ = E.make_model(hp, ops, device)
        spks = singer_rows(hp, 3)
        noise, solo = singers_noise(hp, T, 3, 4)
        w = Watch(m)
        got = svc_infer_singers(w, None, spks, *_args(d, hp, device), noise=noise)
        ws = Watch(m)
        want = [solo_run(ws, d, hp, device, spks[s], solo[s]) for s in range(3)]
        _three_cache[key] = dict(got=got, want=want, z_p=w.z_p[0], solo_z_p=[z[0] for z in ws.z_p], calls=w.calls, solo_calls=ws.calls)
    return _three_cache[key]


def check_three_singers(ops, device, T=37):
    """S = 3: z_p bit-equal to the solo path's, waveforms within BATCH_TOL of the solo runs, the speakers really used, one pitch2source
    call, one singer against the CPU oracle."""
    hp, d = _clip(T, 11, False)
    _, sd = E.make_model(hp, ops, device)
    spks = singer_rows(hp, 3)
    _, solo = singers_noise(hp, T, 3, 4)
    r = three_singers(ops, device, T)
    assert r["calls"] == {"pitch2source": 1, "inference": 0, "inference_singers": 1}, r["calls"]       # the source is made once for all singers
    assert r["solo_calls"] == {"pitch2source": 3, "inference": 3, "inference_singers": 0}
    assert r["z_p"].shape == (3, hp.vits.inter_channels, T)
    for s in range(3):
        assert torch.equal(r["z_p"][s], r["solo_z_p"][s]), (s, float((r["z_p"][s] - r["solo_z_p"][s]).abs().max()))
    errs = [float(np.abs(r["got"][s] - r["want"][s]).max()) for s in range(3)]
    print(f"singers S=3 vs solo svc_infer: {errs}")
    assert max(errs) <= BATCH_TOL, errs
    apart = {(a, b): float(np.abs(r["got"][a] - r["got"][b]).max()) for a in range(3) for b in range(a)}
    print(f"singers S=3, distance between singers: {apart}")
    assert min(apart.values()) > 100 * BATCH_TOL, apart
    s = 2
    with torch.no_grad():
        o_src = O.pitch2source(sd, hp, d["pit"], solo[s]["rand_ini"], solo[s]["src_noise"])
        o_wav = O.synth_inference(sd, hp, d["ppg"], d["vec"], d["pit"], spks[s:s + 1], d["lengths"], o_src, solo[s]["enc_noises"][0])
    e_or = float(np.abs(r["got"][s] - o_wav[0, 0, :-1].numpy()).max())
    print(f"singer {s} vs the CPU oracle: {e_or:.3e}")
    assert e_or <= E.WAVE_TOL, e_or


def check_grouping(ops, device, T=37):
    """S = 3 with singer_batch = 2 (groups of 2 and 1): each singer within BATCH_TOL of the one-group result, the group of one bit-equal to
    its solo run."""
    from svcmi.svc_inference import svc_infer_singers
    hp, d = _clip(T, 11, False)
    m, _ = E.make_model(hp, ops, device)
    noise, _ = singers_noise(hp, T, 3, 4)
    r = three_singers(ops, device, T)
    split = svc_infer_singers(m, None, singer_rows(hp, 3), *_args(d, hp, device), noise=noise, singer_batch=2)
    errs = [float(np.abs(a - b).max()) for a, b in zip(r["got"], split)]
    print(f"singers singer_batch 2 vs 3: {errs}")
    assert max(errs) <= BATCH_TOL, errs
    assert float(np.abs(split[2] - r["want"][2]).max()) == 0.0


def check_two_chunks(ops, device, T=2600):
    """S = 2 over the chunk seam (the length svc_infer_tiny_2chunks uses)."""
    from svcmi.svc_inference import svc_infer_singers
    hp, d = _clip(T, 2, False)
    m, _ = E.make_model(hp, ops, device)
    spks = singer_rows(hp, 2)
    noise, solo = singers_noise(hp, T, 2, 6)
    got = svc_infer_singers(m, None, spks, *_args(d, hp, device), noise=noise)
    seam = C.CHUNK_FRAMES * 320
    for s in range(2):
        want = solo_run(m, d, hp, device, spks[s], solo[s])
        assert got[s].shape == (320 * T - 1,)
        err, e_seam = float(np.abs(got[s] - want).max()), float(np.abs(got[s][seam - 3000:seam + 3000] - want[seam - 3000:seam + 3000]).max())
        print(f"singers two chunks singer {s}: max error {err:.3e} (seam {e_seam:.3e})")
        assert err <= BATCH_TOL, (s, err)


def check_retrieval_once_per_chunk(ops, device, T=90, check_changed=True):
    """S = 2 with the on-device kNN blend: each singer within BATCH_TOL of solo svc_infer with the same retrieval, and the blend ran once
    per chunk, not once per singer."""
    from svcmi.feature_retrieval import KnnFeatureIndex, KnnIndexRetrieval
    from svcmi.svc_inference import svc_infer_singers
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

    spks = singer_rows(hp, 2)
    noise, solo = singers_noise(hp, T, 2, 8)
    counting = Counting()
    got = svc_infer_singers(m, counting, spks, *_args(d, hp, device), noise=noise)
    n_chunks = len(O.chunk_schedule(T, 320))
    assert counting.calls == {"whisper": n_chunks, "hubert": n_chunks}, counting.calls
    plain = svc_infer_singers(m, None, spks, *_args(d, hp, device), noise=noise) if check_changed else None
    for s in range(2):
        want = solo_run(m, d, hp, device, spks[s], solo[s], retrieval=knn)
        err = float(np.abs(got[s] - want).max())
        print(f"singers with retrieval singer {s}: max error {err:.3e}")
        assert err <= BATCH_TOL, (s, err)
        if check_changed:
            assert float(np.abs(got[s] - plain[s]).max()) > 100 * BATCH_TOL      # the blend actually changed the features


def check_base_model(ops, device, T=200, S=16):
    """base.yaml widths at the default singer batch: singers 0, 7 and 15 within BATCH_TOL of their solo runs."""
    from svcmi.svc_inference import SINGER_BATCH, svc_infer_singers
    assert SINGER_BATCH == S
    hp, d = _clip(T, 13, True)
    m, _ = E.make_model(hp, ops, device)
    spks = singer_rows(hp, S)
    noise, solo = singers_noise(hp, T, S, 10)
    got = svc_infer_singers(m, None, spks, *_args(d, hp, device), noise=noise)
    for s in (0, 7, 15):
        want = solo_run(m, d, hp, device, spks[s], solo[s])
        err = float(np.abs(got[s] - want).max())
        print(f"singers base model singer {s}: max error {err:.3e}")
        assert err <= BATCH_TOL, (s, err)


def check_driver_arguments(ops, device):
    import pytest
    from svcmi.svc_inference import svc_infer_singers
    hp, d = _clip(5, 1, False)
    m, _ = E.make_model(hp, ops, device)
    one = singer_rows(hp, 1)
    for bad in (dict(spks=one[:0]), dict(spks=one[0]), dict(spks=one, singer_batch=0), dict(spks=one, singer_batch=33)):
        with pytest.raises(ValueError):
            svc_infer_singers(m, None, bad.pop("spks"), *_args(d, hp, device), **bad)
    twice = torch.cat([one, one])                                  # the same voice twice, no noise given: a fresh prior draw per singer
    outs = svc_infer_singers(m, None, twice, *_args(d, hp, device), return_tensor=True)
    assert len(outs) == 2 and all(torch.is_tensor(o) and o.shape == (5 * 320 - 1,) and o.device.type == torch.device(device).type for o in outs)
    assert not torch.equal(outs[0], outs[1])
