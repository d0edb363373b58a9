"""Pitch-curve control, the part that needs no GPU: numpy / fp64 restatements of the two kernels of csrc/pitch_ops.hip written FROM THEIR
DEFINITIONS (include/visinger_hip.h "f4") and held against the reference's own norm_interp_f0 outputs
(tests/golden/norm_interp_f0.npz, made by tests/golden/make_pitch_golden.py); the two exports exist and validate their arguments before
anything is launched; the driver keeps guided and unguided items apart.  tests/test_pitch_gpu.py compares the kernels with
`norm_interp_ref` and `condition_ref` below."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

F0_MIN, F0_MAX = 50.0, 1250.0          # denorm_f0's default range


def norm_interp_ref(f0_hz, lengths=None):
    """fp64 (f0_norm, uv) of f0_hz [B, T] (or one row [T]): row b is its first lengths[b] frames, the rest is 0 in both outputs"""
    f0 = np.atleast_2d(np.asarray(f0_hz, dtype=np.float64))
    B, T = f0.shape
    lengths = [T] * B if lengths is None else [min(max(int(n), 0), T) for n in lengths]
    f0_norm, uv = np.zeros((B, T)), np.zeros((B, T))
    for b, n in enumerate(lengths):
        row = f0[b, :n]
        voiced = np.isfinite(row) & (row > 0)
        uv[b, :n] = ~voiced
        anchors = np.flatnonzero(voiced)
        if len(anchors) == 0:
            continue                                         # a row without a voiced frame is all 0
        val = np.log2(row[anchors] + 1.0)
        for t in range(n):
            k = np.searchsorted(anchors, t)                  # first anchor at or after t
            if k < len(anchors) and anchors[k] == t:
                f0_norm[b, t] = val[k]
            elif k == 0:
                f0_norm[b, t] = val[0]                       # before the first voiced frame: its value
            elif k == len(anchors):
                f0_norm[b, t] = val[-1]                      # after the last: its value
            else:
                l, r = anchors[k - 1], anchors[k]
                f0_norm[b, t] = val[k - 1] + (val[k] - val[k - 1]) * (t - l) / (r - l)
    if np.ndim(f0_hz) == 1:
        return f0_norm[0], uv[0]
    return f0_norm, uv


def condition_ref(mask=None, pred=None, f0_norm=None, uv=None, cents=None):
    """fp64 (cond [B, T], f0_hz_out [B, T]) of vs_pitch_condition's definition"""
    x = np.asarray(f0_norm if f0_norm is not None else pred[..., 0], dtype=np.float64).copy()
    voiced = (np.asarray(uv) == 0) if uv is not None else (np.asarray(pred)[..., 1] <= 0)
    if cents is not None:
        c = np.asarray(cents, dtype=np.float64)[:, None] * np.ones_like(x)
        x = np.where(c != 0, np.log2((2.0 ** x - 1.0) * 2.0 ** (c / 1200.0) + 1.0), x)
    m = np.ones_like(x) if mask is None else np.asarray(mask, dtype=np.float64).reshape(x.shape)
    on = voiced & (m != 0)
    return np.where(on, x * m, 0.0), np.where(on, np.clip(2.0 ** x - 1.0, F0_MIN, F0_MAX), 0.0)


def golden_rows():
    z = np.load(os.path.join(GOLDEN, "norm_interp_f0.npz"))
    return {str(name): (z[f"r{i}.f0"], z[f"r{i}.f0_norm"], z[f"r{i}.uv"]) for i, name in enumerate(z["names"])}


def test_restatement_equals_the_reference():
    rows = golden_rows()
    for want in ("all_voiced", "all_unvoiced", "one_voiced_frame", "leading_gap", "trailing_gap", "interior_gap", "alternating_single_frames",
                 "t1_voiced", "t1_unvoiced", "two_anchors_600"):
        assert want in rows
    f0 = rows["two_anchors_600"][0]
    assert len(f0) == 600 and list(np.flatnonzero(f0)) == [3, 580]
    for name, (f0, f0_norm, uv) in rows.items():
        assert f0.dtype == f0_norm.dtype == uv.dtype == np.float32
        got_norm, got_uv = norm_interp_ref(f0)
        assert np.array_equal(got_uv, uv), name
        err = float(np.abs(got_norm - f0_norm).max())
        assert err <= 1e-6, (name, err)


def test_restatement_lengths_and_bad_values():
    rows = golden_rows()
    f0, f0_norm, uv = rows["interior_gap"]
    n = len(f0)
    padded = np.concatenate([f0, np.full(7, 333.0, np.float32)])          # voiced frames beyond the length take no part
    got_norm, got_uv = norm_interp_ref(np.stack([padded, padded]), lengths=[n, 5])
    assert np.abs(got_norm[0, :n] - f0_norm).max() <= 1e-6 and np.array_equal(got_uv[0, :n], uv)
    assert (got_norm[0, n:] == 0).all() and (got_uv[0, n:] == 0).all() and (got_norm[1, 5:] == 0).all() and (got_uv[1, 5:] == 0).all()
    assert np.array_equal(got_norm[1, :5], norm_interp_ref(f0[:5])[0])
    bad = np.array([100.0, -3.0, np.nan, np.inf, 200.0], np.float32)      # negative / non-finite: unvoiced, bridged like a 0
    got_norm, got_uv = norm_interp_ref(bad)
    assert list(got_uv) == [0, 1, 1, 1, 0] and np.isfinite(got_norm).all()
    assert np.allclose(got_norm, norm_interp_ref(np.array([100.0, 0, 0, 0, 200.0]))[0])


def test_condition_restatement_is_the_reference_expression_without_a_shift():
    g = np.random.default_rng(5)
    B, T = 3, 11
    pred = g.standard_normal((B, T, 2)) + np.array([7.0, 0.0])
    mask = (np.arange(T)[None, :] < np.array([11, 6, 1])[:, None]).astype(np.float64)
    cond, hz = condition_ref(mask, pred=pred)
    assert np.array_equal(cond, pred[..., 0] * (pred[..., 1] <= 0) * mask)
    on = (pred[..., 1] <= 0) & (mask != 0)
    assert np.array_equal(hz, np.where(on, np.clip(2.0 ** pred[..., 0] - 1, 50, 1250), 0))
    up, hz_up = condition_ref(mask, pred=pred, cents=[1200.0, 0.0, -1200.0])
    assert np.array_equal(up[1], cond[1]) and np.array_equal(hz_up[1], hz[1])
    free = on[0] & (2 * (2.0 ** pred[0, :, 0] - 1) < 1250) & (2.0 ** pred[0, :, 0] - 1 > 50)
    assert free.any() and np.allclose(hz_up[0][free], 2 * hz[0][free], rtol=1e-12)


def test_library_exports_the_pitch_entry_points():
    from visinger_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "vs_f0_norm_interp") and hasattr(lib, "vs_pitch_condition")
    assert _lib.lib().vs_abi_version() == _lib.EXPECTED_ABI == 7


def test_pitch_arguments_are_validated_before_anything_is_launched():
    """every VS_EINVAL case returns non-zero with the function's name in the message.  The pointers are HOST memory and no call here is valid,
    so nothing may reach the device."""
    from visinger_amd import _lib
    L = _lib.lib()
    bufs = [(ctypes.c_int64 * 64)() for _ in range(3)]
    p, q, r = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)

    def interp(f0=p, lengths=None, f0_norm=q, uv=r, B=2, T=5):
        return L.vs_f0_norm_interp(f0, lengths, f0_norm, uv, B, T, None)

    def cond(pred=p, f0_norm=None, uv=None, mask=None, cents=None, cond=q, hz=None, B=2, T=5):
        return L.vs_pitch_condition(pred, f0_norm, uv, mask, cents, cond, hz, B, T, None)

    sizes = [dict(B=0), dict(T=0), dict(B=-1), dict(T=-7)]
    for kw in sizes + [dict(f0=None), dict(f0_norm=None), dict(uv=None), dict(T=1 << 24), dict(T=(1 << 24) + 5), dict(f0_norm=p), dict(uv=p), dict(uv=q)]:
        assert interp(**kw) != 0, kw
        assert b"vs_f0_norm_interp" in L.vs_last_error(), kw
    for kw in sizes + [dict(cond=None), dict(pred=None), dict(pred=None, uv=r), dict(pred=None, f0_norm=r), dict(pred=ctypes.c_void_p(p.value + 4))]:
        assert cond(**kw) != 0, kw
        assert b"vs_pitch_condition" in L.vs_last_error(), kw


def test_python_layer_refuses_cpu_tensors_and_bad_shifts():
    from visinger_amd import _lib, pitch
    with pytest.raises(_lib.VisingerHipError):
        pitch.norm_interp_f0(torch.zeros(2, 5))
    with pytest.raises(_lib.VisingerHipError):
        pitch.pitch_condition(None, pred=torch.zeros(2, 5, 2))
    with pytest.raises(_lib.VisingerHipError):
        pitch.pitch_condition(None)
    assert pitch.cents_tensor(50, 3, "cpu").tolist() == [50.0] * 3 and pitch.cents_tensor([1, -2.5], 2, "cpu").tolist() == [1.0, -2.5]
    assert pitch.cents_tensor(np.float32(7), 2, "cpu").dtype == torch.float32
    with pytest.raises(ValueError):
        pitch.cents_tensor([1, 2, 3], 2, "cpu")
    with pytest.raises(ValueError):
        pitch.cents_tensor(float("nan"), 2, "cpu")


def item(n_frames, n_tokens=2, f0=None):
    it = dict(text_tokens=np.arange(1, n_tokens + 1), pitch_tokens=np.arange(1, n_tokens + 1), dur_tokens=np.arange(1, n_tokens + 1),
              mel2ph=np.repeat(np.arange(1, n_tokens + 1), n_frames // n_tokens + 1)[:n_frames])
    if f0 is not None:
        it["f0"] = f0
    return it


def test_driver_keeps_guided_and_unguided_items_apart():
    from visinger_amd import synth
    a, b = item(6, f0=np.array([0, 100, 0, 0, 200, 0.0])), item(4, f0=[300.0, 0, 0, 310.0])
    batch = synth.collate([a, b], "cpu")
    assert batch["f0_hz"].dtype == torch.float32 and batch["f0_hz"].shape == batch["mel2ph"].shape == (2, 6)
    assert batch["f0_hz"].tolist() == [[0, 100, 0, 0, 200, 0], [300, 0, 0, 310, 0, 0]]
    assert "f0_hz" not in synth.collate([item(6), item(4)], "cpu")
    with pytest.raises(ValueError, match="guide"):
        synth.collate([a, item(4)], "cpu")
    with pytest.raises(ValueError, match="frames"):
        synth.collate([item(6, f0=np.ones(5))], "cpu")
    with pytest.raises(ValueError, match="frames"):
        synth.collate([item(6, f0=np.ones((6, 1)))], "cpu")
    # bucket_by_length's keys: (guided, token count) never mixes, where lengths alone would
    lengths, guided, tokens = [6, 6, 6, 6], [True, False, True, False], [2, 2, 3, 2]
    assert len(synth.bucket_by_length(lengths, 1000)) == 1
    by_guide = synth.bucket_by_length(lengths, 1000, keys=guided)
    assert sorted(map(sorted, by_guide)) == [[0, 2], [1, 3]]
    both = synth.bucket_by_length(lengths, 1000, keys=list(zip(guided, tokens)))
    assert sorted(map(sorted, both)) == [[0], [1, 3], [2]]
    model = torch.nn.Linear(2, 2)               # never reached: the arguments are checked first
    with pytest.raises(ValueError, match="voicing"):
        synth.synthesize(model, [a], 8, voicing="tracker")
    with pytest.raises(ValueError, match="pitch shifts"):
        synth.synthesize(model, [a, b], 8, pitch_shift_cents=[1.0])
    with pytest.raises(ValueError, match="frames"):
        synth.synthesize(model, [item(6, f0=np.ones(5))], 8)


def test_model_refuses_contradicting_pitch_arguments():
    from visinger_amd.models.visinger import VISinger
    fwd = VISinger.forward

    class Stub:
        hparams = {"use_pitch_embed": False}
    x = torch.zeros(1, 3)
    with pytest.raises(ValueError, match="voicing"):
        fwd(Stub(), x, x, x, x, infer=True, voicing="tracker")
    with pytest.raises(ValueError, match="use_pitch_embed"):
        fwd(Stub(), x, x, x, x, infer=True, f0_hz=x)
    with pytest.raises(ValueError, match="use_pitch_embed"):
        fwd(Stub(), x, x, x, x, infer=True, pitch_shift_cents=10.0)
    Stub.hparams = {"use_pitch_embed": True}
    with pytest.raises(ValueError, match="f0_hz"):
        fwd(Stub(), x, x, x, x, infer=True, f0_hz=x, f0=x, uv=x)
    with pytest.raises(ValueError, match="f0_hz"):
        fwd(Stub(), x, x, x, x, infer=True, f0_hz=x, uv=x)
