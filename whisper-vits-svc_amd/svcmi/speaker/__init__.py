"""Drop-in for the reference's ``speaker`` package (row N5): the LSTM speaker encoder that turns a recording into the 256-float
timbre embedding ``--spk`` takes, on the svcmi kernels.

    from svcmi.speaker.models.lstm import LSTMSpeakerEncoder        # speaker/models/lstm.py
    from svcmi.speaker.utils.audio import AudioProcessor            # speaker/utils/audio.py (the inference subset)
    python -m svcmi.speaker.infer MODEL CONFIG -s in.wav -t out.spk.npy
"""
from .models.lstm import LSTMSpeakerEncoder      # noqa: F401
from .utils.audio import AudioProcessor          # noqa: F401
