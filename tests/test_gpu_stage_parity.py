"""Stage-by-stage parity against the fp64 oracle at the shapes the benchmark runs (BASELINE.json configs[1] - configs[4]).

The end-to-end tests hold the north-star bar (1e-3 on the waveform); fp32 reaches ~400x less, so a launch that is subtly wrong at
production size passes them.  Here every stage starts from the rounded fp64 result of the stage before it and is held to the fp32 class
of that stage (engine_cases.check_stages_fp64 / check_whisper_fp64: 8x the fp32 oracle's own error, floor 2e-6, cap 5e-5), with the
engine's dispatch at production size: the 16x16x4 tile policy at t_out >= 1024, the prior FFN's K split by B*T, Whisper's B = 1 tuning
table and its flattened M = B*tw projections above 1024 rows, the generator's batch-size-chosen forms.  The fp64 references are CPU
work; items and sub-batches are chosen to keep the module near three minutes."""
import pytest
import torch

from workload import config as C
from workload import inputs as I
from oracle import svc_oracle as O
from workload import weights as W
from tests import engine_cases as E

pytestmark = pytest.mark.gpu

PERTURBATION = 1e-3          # as tests/test_engine_emu.py: one engine weight tensor x (1 + PERTURBATION)


@pytest.fixture(scope="module")
def ops():
    from svcmi import Ops
    o = Ops()
    assert o.build == "hip:gfx950" and o.on_gpu
    return o


@pytest.fixture(scope="module")
def large_v2(ops):
    from svcmi.whisper.inference import load_model
    ck = W.make_whisper_state(C.WHISPER_LARGE_V2)
    return ck, load_model(ck, "cuda", ops=ops)


@pytest.fixture(scope="module")
def clip10s():
    """configs[1]'s clip (the one test_full_10s_clip_against_oracle uses) with its oracle results, computed once: the fp64 stage
    references and the fp32 oracle waveform."""
    hp = C.base_hp()
    sd = W.make_vits_state(hp, seed=1234)
    d = I.synth_clip(T=1000, hp=hp, seed=0, B=1)
    refs = E.synth_stage_refs(sd, hp, d)
    with torch.no_grad():
        o_src = O.pitch2source(sd, hp, d["pit"], d["rand_ini"], d["src_noise"])
        o_wav = O.synth_inference(sd, hp, d["ppg"], d["vec"], d["pit"], d["spk"], d["lengths"], o_src, d["enc_noise"])
    return hp, sd, d, refs, o_wav


def _mel(B, n, seed):
    """Pre-summed fp32 mel + 0.1 * noise (E.check_whisper_fp64)."""
    g = torch.Generator().manual_seed(seed)
    mel = (torch.randn(B, 80, n, generator=g) * 0.5).clamp(-1, 1.5)
    return mel + 0.1 * torch.randn(B, 80, n, generator=g)


def test_config1_whisper_against_fp64(ops, large_v2):
    """configs[1] Whisper: large-v2 (24 kept blocks) on one 10 s window, n = 1000 -> 500 rows: the B = 1 tuning table."""
    ck, wm = large_v2
    E.check_whisper_fp64(wm, ck, C.WHISPER_LARGE_V2, _mel(1, 1000, 11), title="configs[1] whisper")


def test_config1_synth_stages_against_fp64(ops, clip10s):
    """configs[1] synthesizer: pitch2source, prior encoder, flow, generator of one 10 s clip (B = 1, T = 1000)."""
    hp, sd, d, refs, _ = clip10s
    m, _ = E.make_model(hp, ops, "cuda")
    E.check_stages_fp64(m, sd, hp, d, refs=refs, title="configs[1]")


def test_config1_stage_bars_catch_a_perturbation_the_waveform_bar_misses(ops, clip10s):
    hp, _, d, refs, o_wav = clip10s
    E.check_perturbation_caught(ops, "cuda", hp, d, PERTURBATION, refs=refs, o_wav=o_wav)


def test_config3_whisper_flattened_batch_equals_solo_runs_and_fp64(ops):
    """configs[3] Whisper: B = 16 windows x n = 1000 at the production threshold (16 x 500 rows > 1024: one M = 8000 matrix per
    projection on the library's 128-row tiles, ragged last tile) -- every item bit-identical to the batch run unflattened without K
    slices, within TIGHT of its solo run (B = 1: conv2 of the stem takes 8 K slices), items 0, 7 and 15 against the oracle and the fp64
    oracle."""
    print(E.check_whisper_batched_rows_flattened(ops, "cuda", C.WHISPER_LARGE_V2, B=16, n=1000, small_m_rows=None, oracle_items=(0, 7, 15),
                                                 solo_bits=False))


def test_config3_batch_of_16_end_to_end_equals_solo_conversions(ops, large_v2):
    """configs[3] as the benchmark's lane function composes one batch: encoder -> [:, :T/2] -> inference_ppg50 (row shift 1), B = 16;
    items 0 and 15 against their solo conversions (the bar of test_batch16_x_10s_items_equal_solo_runs)."""
    _, wm = large_v2
    hp = C.base_hp()
    m, _ = E.make_model(hp, ops, "cuda")
    B, T = 16, 1000
    items = [I.synth_clip(T=T, hp=hp, seed=60 + s, B=1, ppg=False) for s in range(B)]
    d = {k: torch.cat([it[k] for it in items], 0).cuda() for k in items[0]}
    d["lengths"] = d["lengths"].to(torch.int32)

    def convert(x):
        ppg50 = wm.encoder(x["mel"], x["mel_noise"], 0.1)[:, :T // 2]
        src = m.pitch2source(x["pit"], noise=(x["rand_ini"], x["src_noise"]))
        return m.inference_ppg50(ppg50, x["vec"], x["pit"], x["spk"], x["lengths"], src, noise=x["enc_noise"])

    wav = convert(d)
    assert wav.shape == (B, 1, T * 320) and bool(torch.isfinite(wav).all())
    for b in (0, 15):
        solo = convert({k: v[b:b + 1] for k, v in d.items()})
        err = E.maxerr(solo, wav[b:b + 1])
        print(f"configs[3] batch item {b} vs solo conversion: {err:.2e}")
        assert err <= 1e-5, (b, err)


def test_config2_flow_and_generator_against_fp64(ops):
    """configs[2]: the engine runs all 16 x 10 s clips (batch-size-dependent dispatch of the flow and the generator); items 0 and 15 go
    through the fp64 stage check, the oracle on that 2-item sub-batch."""
    hp = C.base_hp()
    m, sd = E.make_model(hp, ops, "cuda")
    items = [I.synth_clip(T=1000, hp=hp, seed=s, B=1) for s in range(16)]
    d = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    E.check_stages_fp64(m, sd, hp, d, items=(0, 15), stages=("z", "wave"), title="configs[2]")


def test_config4_whisper_two_15s_windows_against_fp64(ops, large_v2):
    """configs[4] Whisper: the two 15 s windows of a 30 s clip as one batch (B = 2 x n = 1500: 1500 rows > 1024, flattened); item 1."""
    ck, wm = large_v2
    E.check_whisper_fp64(wm, ck, C.WHISPER_LARGE_V2, _mel(2, 1500, 13), items=(1,), title="configs[4] whisper")
