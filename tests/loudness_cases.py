"""Inputs the loudness tests share (tests/test_loudness_cpu.py, tests/test_loudness_gpu.py): the gating fixture and the margin of its blocks from the gates."""
import numpy as np


def gating_fixture():
    """(x fp32 [64000], 8000): 3 s of a 0.5-amplitude 440 Hz sine, 3 s of the same sine 30 dB lower, 2 s of 1e-4 normal noise.  The loud part passes both gates,
    the quiet one only the absolute gate (it is 30 dB under the loud one: the relative gate sits 10 dB under the mean of the two), the noise neither (-80 dBFS)."""
    sr = 8000
    t = np.arange(3 * sr) / sr
    tone = 0.5 * np.sin(2.0 * np.pi * 440.0 * t)
    noise = 1e-4 * np.random.default_rng(0).standard_normal(2 * sr)
    return np.concatenate([tone, tone * 10.0 ** (-30.0 / 20.0), noise]).astype(np.float32), sr


def gate_margin(S, n_steps, s):
    """the smallest relative distance of a block of one row -- its step sums S[:n_steps] -- from the absolute gate and from the relative gate"""
    from visinger_amd import loudness as lo
    if n_steps < 4:
        return np.inf
    z = (S[0:n_steps - 3] + S[1:n_steps - 2] + S[2:n_steps - 1] + S[3:n_steps]) / (4.0 * s)
    z = z[np.isfinite(z)]
    margin = np.abs(z / lo.ABS_GATE - 1.0).min() if len(z) else np.inf
    over = z > lo.ABS_GATE
    if over.any():
        margin = min(margin, np.abs(z / (lo.REL_GATE * z[over].mean()) - 1.0).min())
    return float(margin)
