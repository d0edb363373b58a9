#!/usr/bin/env python3
"""Generate the pitch-control fixtures under tests/golden/ by IMPORTING the reference (read-only), the way make_golden.py does (whose import
set-up and helpers are reused by importing it):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pitch_golden.py

Nothing from the reference is copied; only .npz data is written.

Reference symbols exercised (file:line under the reference's root):
  utils/audio/pitch/utils.py:42-57     norm_interp_f0 (per item, numpy / np.interp)
  utils/commons/dataset_utils.py:17-35 collate_1d_or_2d (how tasks/dataset_utils.py:205-206 pads f0 with 0.0 and uv with 0)
  models/visinger.py:71-135            VISinger.forward(f0=, uv=, infer=True) on the weights / inputs / noise of visinger_tiny_pitch.npz

norm_interp_f0.npz        rows r<i>.f0 (fp32 Hz, 0 = unvoiced) -> r<i>.f0_norm, r<i>.uv; `names` lists what each row covers
visinger_tiny_guide.npz   f0_hz [2, 23] (item 1: 17 frames), f0_norm / uv as the reference's dataset + collate produce them, and its teacher-forced
                          synthesis wav_out / f0_pred
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stubs the missing third-party modules, puts the reference on sys.path)

from utils.audio.pitch.utils import norm_interp_f0  # noqa: E402
from utils.commons.dataset_utils import collate_1d_or_2d  # noqa: E402


def gen_norm_interp():
    r = np.random.default_rng(91)

    def hz(n):
        return r.uniform(80.0, 900.0, n).astype(np.float32)

    rows = {}
    rows["all_voiced"] = hz(37)
    rows["all_unvoiced"] = np.zeros(19, np.float32)
    one = np.zeros(23, np.float32)
    one[9] = 220.0
    rows["one_voiced_frame"] = one
    lead = hz(29)
    lead[:7] = 0
    rows["leading_gap"] = lead
    trail = hz(31)
    trail[-9:] = 0
    rows["trailing_gap"] = trail
    inner = hz(41)
    inner[11:27] = 0
    rows["interior_gap"] = inner
    alt = hz(33)
    alt[1::2] = 0
    rows["alternating_single_frames"] = alt
    rows["t1_voiced"] = np.array([440.0], np.float32)
    rows["t1_unvoiced"] = np.zeros(1, np.float32)
    mixed = hz(300)
    mixed[:3] = 0
    mixed[40:45] = 0
    mixed[100] = 0
    mixed[250:262] = 0
    mixed[-4:] = 0
    rows["mixed_gaps_300"] = mixed
    two = np.zeros(600, np.float32)
    two[3], two[580] = 110.0, 880.0
    rows["two_anchors_600"] = two
    arrays = {"names": np.array(list(rows))}
    for i, (name, f0) in enumerate(rows.items()):
        f0_norm, uv = norm_interp_f0(f0.copy())
        assert f0_norm.dtype == torch.float32 and uv.dtype == torch.float32 and bool(torch.isfinite(f0_norm).all()), name
        arrays[f"r{i}.f0"], arrays[f"r{i}.f0_norm"], arrays[f"r{i}.uv"] = f0, f0_norm, uv
    mg.save("norm_interp_f0", **arrays)


def gen_model_guide():
    """forward(f0=, uv=, infer=True) of the reference on the visinger_tiny_pitch weights, inputs and noise, with f0 / uv its own norm_interp_f0 of each
    item's guide, padded as its collate pads.  The one call-site adaptation of frame_prior is the one gen_model_pitch documents: the condition
    is handed over as [B, T, 1] so that the reference's own transpose restores what its Conv1d(1, H, 1) expects."""
    from models.visinger import VISinger
    z = np.load(os.path.join(HERE, "visinger_tiny_pitch.npz"))
    hp = json.load(open(os.path.join(HERE, "visinger_tiny_pitch_hparams.json")))
    m = VISinger(13, 9, 7, hp).eval()
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}, strict=True)
    inner = m.frame_prior.forward
    m.frame_prior.forward = lambda x, x_mask, g=None: inner(x, x_mask, None if g is None else g.transpose(1, 2))
    text, pitch, dur, mel2ph, spk_id = (torch.from_numpy(z[k]) for k in ("text", "pitch", "dur", "mel2ph", "spk_id"))
    B, T = mel2ph.shape
    lens = (mel2ph > 0).sum(1).tolist()
    assert (B, T, lens) == (2, 23, [23, 17])
    r = np.random.default_rng(92)
    guides = []
    for n in lens:
        f0 = r.uniform(80.0, 900.0, n).astype(np.float32)
        guides.append(f0)
    guides[0][:2] = 0            # leading gap
    guides[0][8:13] = 0          # interior gap
    guides[0][17] = 0            # a single dropped frame
    guides[0][-3:] = 0           # trailing gap
    guides[1][:1] = 0
    guides[1][5:9] = 0
    guides[1][-2:] = 0
    pairs = [norm_interp_f0(g.copy()) for g in guides]
    f0 = collate_1d_or_2d([p[0] for p in pairs], 0.0)
    uv = collate_1d_or_2d([p[1] for p in pairs])
    f0_hz = collate_1d_or_2d([torch.from_numpy(g) for g in guides], 0.0)
    assert f0.shape == uv.shape == f0_hz.shape == (B, T)
    noise = torch.from_numpy(z["noise"])
    real = torch.randn_like
    torch.randn_like = lambda *a, **k: noise.clone()          # the sample visinger_tiny_pitch was made with (models/visinger.py:107)
    try:
        ret = m(text, pitch, dur, mel2ph, spk_id=spk_id, f0=f0, uv=uv, infer=True)
    finally:
        torch.randn_like = real
    margin = float(ret["f0_pred"][:, :, 1].abs().min())
    assert margin > 1e-3, margin          # no predicted voicing logit within 1e-3 of the threshold (voicing="model" is compared bit for bit)
    assert float((ret["f0_pred"] - torch.from_numpy(z["f0_pred"])).abs().max()) == 0.0          # the predictor does not see the guide
    assert float((ret["wav_out"] - torch.from_numpy(z["wav_out"])).abs().max()) > 1e-3          # ... the waveform does
    mg.save("visinger_tiny_guide", f0_hz=f0_hz, f0_norm=f0, uv=uv, wav_out=ret["wav_out"], f0_pred=ret["f0_pred"])


if __name__ == "__main__":
    gen_norm_interp()
    gen_model_guide()
