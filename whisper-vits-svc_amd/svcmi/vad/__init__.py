"""Drop-in for the reference's ``vad`` package (Silero voice-activity detection, vad/utils.py) on the kernels of csrc/vad.hip.

    from svcmi.vad.utils import init_jit_model, get_speech_timestamps
"""
from .utils import SileroVad, get_speech_timestamps, init_jit_model  # noqa: F401
