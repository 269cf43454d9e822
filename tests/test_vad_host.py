"""The span logic of svcmi.vad.utils.get_speech_timestamps against the reference's function, without any kernel: a stand-in model
replays every stored probability track of tests/golden/silero_vad.npz (scripts/make_vad_golden.py: about 200 tracks of 1 to 400 windows
-- all speech, all silence, values exactly on the two decision levels, single-window blips and dips, over-long speech that the
``max_speech_duration_s`` logic splits -- under eight parameter sets), and every result must equal the reference's exactly."""
import warnings

import numpy as np
import pytest
import torch

from tests import vad_cases as V


def test_every_stored_case_equals_the_reference_exactly():
    from svcmi.vad.utils import get_speech_timestamps
    n = per_set = splits = on_level = 0
    seen = set()
    for params, track, samples, want in V.state_machine_cases():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                 # (the 32 kHz set warns about the cast to 16 kHz, like the reference)
            got = get_speech_timestamps(torch.zeros(samples), V.Replay(track), **params)
        assert [[float(t["start"]), float(t["end"])] for t in got] == want, (n, params, samples, got, want)
        if not params.get("return_seconds"):
            assert all(isinstance(t["start"], int) and isinstance(t["end"], int) for t in got)
        n += 1
        seen.add(tuple(sorted(params.items())))
        splits += int("max_speech_duration_s" in params and len(want) > 1)
        on_level += int(bool((track == np.float32(params["threshold"])).any()))
    assert n >= 190 and len(seen) >= 6 and splits >= 5 and on_level >= 5, (n, len(seen), splits, on_level)


def test_track_lengths_cover_one_window_to_four_hundred():
    z = V.golden()
    assert int(z["sm_windows"].min()) == 1 and int(z["sm_windows"].max()) == 400
    assert int(z["sm_nspans"].sum()) == z["sm_spans"].reshape(-1, 2).shape[0] and int((z["sm_nspans"] == 0).sum()) > 0


def test_unsupported_inputs_raise_before_the_model_is_asked():
    from svcmi.vad.utils import get_speech_timestamps

    class Never:
        def audio_forward(self, *a, **k):
            raise AssertionError("the model must not be called")
    x = torch.zeros(4096)
    with pytest.raises(ValueError, match="8 kHz"):
        get_speech_timestamps(x, Never(), sampling_rate=8000)
    with pytest.raises(ValueError, match="512"):
        get_speech_timestamps(x, Never(), window_size_samples=1024)
    with pytest.raises(ValueError, match="16000"):
        get_speech_timestamps(x, Never(), sampling_rate=22050)
    with pytest.raises(ValueError):
        get_speech_timestamps(torch.zeros(2, 4096), Never())
    assert get_speech_timestamps(torch.zeros(0), Never()) == []


def test_fixture_holds_the_16k_tensors_only_and_stays_small():
    import os
    z = V.golden()
    names = [k for k in z if k.startswith("sd/")]
    assert sum(int(np.prod(z[k].shape)) for k in names) == 156488
    assert not [k for k in names if "8k" in k]
    assert os.path.getsize(os.path.join(V.GOLDEN, "silero_vad.npz")) < 944 * 1024
    assert float(z["ref_dev_035"]) < 5e-6 and float(z["ref_dev_010"]) < 1e-5
