"""svcmi.pitch.core -- the network-free F0 estimators (drop-in for the reference's pitch/core): ``from svcmi.pitch.core.salience import salience``, ``from svcmi.pitch.core.pyin import pyin``, ``from svcmi.pitch.core.swipe_slim import swipe_slim``, ``from svcmi.pitch.core.yin import yin, yin_plan, yin_begin``.

``svcmi.pitch.core.yin`` is the MODULE, as in the reference (a package attribute cannot be the module and its function of the same name);
``yin_plan`` and ``yin_begin`` are also reachable from the package itself."""


def __getattr__(name):
    if name in ("yin_plan", "yin_begin"):
        from . import yin as _yin
        return getattr(_yin, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
