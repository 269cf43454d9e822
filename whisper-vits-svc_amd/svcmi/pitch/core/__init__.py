"""svcmi.pitch.core -- the network-free F0 estimators (drop-in for the reference's pitch/core): ``from svcmi.pitch.core.salience import salience``, ``from svcmi.pitch.core.pyin import pyin``."""
