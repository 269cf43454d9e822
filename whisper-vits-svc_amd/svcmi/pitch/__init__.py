"""svcmi.pitch -- F0 extraction for the SVC pipeline (drop-in for the reference's pitch/inference.py + its vendored crepe)."""
from .inference import Crepe, bins_to_hz, compute_f0_sing, compute_f0_train, decode, f0_train_postfilter, load_csv_pitch, load_crepe, save_csv_pitch, viterbi_path  # noqa: F401
from .inference import compute_f0_salience, compute_f0_salience_begin, move_average  # noqa: F401
from .inference import compute_f0_pyin, compute_f0_pyin_begin  # noqa: F401
from .inference import compute_f0_swipe, compute_f0_swipe_begin  # noqa: F401
from .inference import compute_f0_yin, compute_f0_yin_begin  # noqa: F401
