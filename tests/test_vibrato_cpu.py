"""Vibrato (rule "f13", visinger_amd/vibrato.py) without a GPU: the numpy restatement of the rule against the properties the rule promises, the
host-side argument checks, the note segmentation and the driver's refusals."""
import ctypes
import math

import numpy as np
import pytest
import torch

SR, HOP = 24000, 256          # 93.75 frames a second


def score(T, T_ph=6):
    """one row: tokens 1 .. T_ph spread evenly over T frames (mel2ph), int64 [1, T]"""
    return (np.arange(T, dtype=np.int64) * T_ph // T + 1)[None]


def ints(**kw):
    from visinger_amd import vibrato as V
    return np.asarray([V.check_args(SR, HOP, **kw)], dtype=np.int64)


def test_offsets_vanish_on_rests_before_the_delay_on_short_notes_and_beyond_the_row():
    from visinger_amd import vibrato as V
    T = 600
    m2p = score(T)                                                      # six tokens of 100 frames
    m2p[0, 560:] = 0                                                    # the row is 560 frames long
    notes = np.array([[0, 1, 1, 2, 0, 3]], dtype=np.int32)              # a rest, a note of 200 frames, one of 100, a rest, one of 60 (cut by the row's end)
    prm = ints(depth_cents=100.0, rate_hz=6.0, delay_s=0.32, attack_s=0.1, release_s=0.1, min_note_s=0.8)      # delay 30, min_len 75 frames
    assert prm[0].tolist()[2:] == [30, 9, 9, 75]
    curve = np.full((1, T), 8.0, dtype=np.float32)
    off, out = V.vibrato_ref(curve, m2p, notes, prm)
    assert off.shape == out.shape == (1, T)
    assert not off[0, :100].any() and not off[0, 400:500].any()          # rests
    assert not off[0, 100:130].any() and not off[0, 300:330].any()       # before the delay of both long notes
    assert off[0, 130] == 0 and off[0, 131] != 0                         # the first modulated frame is 0 (ea = 0), the next is not
    assert np.abs(off[0, 131:300]).max() > 1000 and np.abs(off[0, 331:400]).max() > 1000
    assert not off[0, 500:].any()                                        # 60 frames < min_len; and beyond the row
    assert (out[0, 560:] == 0).all() and (out[0, :560][off[0, :560] == 0] == 8.0).all()
    assert np.abs(off).max() <= prm[0, 0] == 1600
    # the release: the last frame of a note has er = 1 of 9
    assert abs(off[0, 299]) <= math.ceil(1600 / 9) and abs(off[0, 399]) <= math.ceil(1600 / 9)
    # the curve moves by the offset: 2^x - 1 Hz times 2^(off / 19200)
    on = off[0] != 0
    hz = 2.0 ** out[0, on] - 1.0
    assert np.allclose(hz, 255.0 * 2.0 ** (off[0, on] / 19200.0), rtol=1e-12)
    # explicit lengths cut the row like mel2ph's padding does; a depth of 0 and a per-note override of 0 silence everything
    off2, _ = V.vibrato_ref(curve, score(T), notes, prm, lengths=[560])
    assert np.array_equal(off2[0, :500], off[0, :500]) and not off2[0, 560:].any()
    assert not V.vibrato_ref(curve, m2p, notes, ints(depth_cents=0.0))[0].any()
    dq = np.array([[-1, 0, 77, -1, -1, -1]], dtype=np.int32)             # note 1's depth is read at its FIRST token: 0; the 77 on its second token is not read
    off3, _ = V.vibrato_ref(curve, m2p, notes, prm, note_depth_q=dq)
    assert not off3[0, 100:300].any() and np.array_equal(off3[0, 300:], off[0, 300:])


@pytest.mark.parametrize("rate_hz,depth_cents", [(5.5, 50.0), (7.3, 1200.0), (0.37, 3.0)])
def test_sustain_follows_the_sine_within_the_derived_bound(rate_hz, depth_cents):
    """In the sustain of a long note (ea = attack, er = release, p < 65536): |offset_q - depth_q sin(2 pi rate p hop / sr)| <= 0.5 + depth_q 2e-4.  The terms,
    relative to depth_q: table rounding 0.5 / 16384 = 3.1e-5; linear interpolation (2 pi / 1024)^2 / 8 = 4.7e-6; the interpolation's floor
    1 / 16384 = 6.1e-5; the phase step's rounding 2 pi 2^-33 65536 = 4.8e-5; dropping the low 6 phase bits 2 pi 2^-26 = 9.4e-8; together 1.45e-4, rounded up
    to 2e-4.  The 0.5 is the final rounding to a whole unit."""
    from visinger_amd import vibrato as V
    T = 60000
    prm = ints(depth_cents=depth_cents, rate_hz=rate_hz, delay_s=0.0, attack_s=0.2, release_s=0.1, min_note_s=0.0)
    depth_q, inc, delay, attack, release, _ = prm[0].tolist()
    off, _ = V.vibrato_ref(np.full((1, T), 8.0, np.float32), np.ones((1, T), np.int64), np.array([[1]], np.int32), prm)
    p = np.arange(attack, T - release)
    want = depth_q * np.sin(2.0 * np.pi * rate_hz * p * HOP / SR)
    err = np.abs(off[0, p] - want)
    print(f"rate {rate_hz} Hz, depth {depth_q}: max error {err.max():.3f} units, bound {0.5 + depth_q * 2e-4:.3f}")
    assert p.max() < 65536 and err.max() <= 0.5 + depth_q * 2e-4
    assert np.abs(off).max() <= depth_q and np.abs(off[0, p]).max() >= depth_q - 1 - depth_q * 2e-4 - depth_q * (np.pi * rate_hz * HOP / SR) ** 2 / 2


def test_sine_table_and_the_integer_sine_stay_inside_their_range():
    from visinger_amd import vibrato as V
    tab = V.sine_table()
    assert tab.dtype == np.int32 and tab.shape == (1025,) and not tab.flags.writeable
    assert tab[0] == tab[512] == tab[1024] == 0 and tab[256] == 16384 and tab[768] == -16384 and np.abs(tab).max() == 16384
    assert np.array_equal(tab[:513], -tab[512:]) and np.abs(np.diff(tab)).max() <= 101          # odd about the half cycle; a step moves it by at most 16384 * 2 pi / 1024


def test_notes_of_tokens_on_a_hand_written_score():
    from visinger_amd import vibrato as V
    #            rest  C   C   D  rest  D   D  rest rest  E   pad pad
    tokens = [[0, 60, 60, 62, 0, 62, 62, 0, 0, 64, 0, 0],
              [61, 61, 0, 61, 63, 63, 61, 0, 0, 0, 0, 0]]
    want = [[0, 1, 1, 2, 0, 3, 3, 0, 0, 4, 0, 0],
            [1, 1, 0, 2, 3, 3, 4, 0, 0, 0, 0, 0]]                       # the same pitch on both sides of a rest: two notes
    got = V.notes_of_tokens(torch.tensor(tokens))
    assert got.dtype == torch.int32 and got.tolist() == want
    assert V.notes_of_tokens(np.array(tokens[0])).tolist() == want[0]
    assert V.notes_of_tokens(torch.tensor([[5, 5, 7]]), rest=5).tolist() == [[0, 0, 1]]
    assert V.REST == 0


def test_check_args_and_params_refuse_what_the_kernel_cannot_take():
    from visinger_amd import vibrato as V
    assert list(V.DEFAULTS) == ["depth_cents", "rate_hz", "delay_s", "attack_s", "release_s", "min_note_s"]
    d = V.check_args(SR, HOP)
    assert d == (800, round(5.5 * HOP / SR * 2 ** 32), 23, 19, 9, 38)
    assert V.check_args(sample_rate=SR, hop_size=HOP, attack_s=0.0, release_s=0.0)[3:5] == (1, 1)         # a ramp is at least one frame
    for bad in (dict(depth=3.0), dict(depth_cents=float("nan")), dict(depth_cents=-1.0), dict(depth_cents=1200.5), dict(rate_hz=float("inf")),
                dict(rate_hz=0.0), dict(rate_hz=1e-9), dict(rate_hz=SR / HOP / 2), dict(rate_hz=-3.0), dict(attack_s=4097 * HOP / SR),
                dict(release_s=50.0), dict(delay_s=-0.1), dict(delay_s=700.0), dict(min_note_s=float("nan")), dict(min_note_s=700.0), dict(rate_hz="5"),
                dict(depth_cents=True)):
        with pytest.raises(ValueError):
            V.check_args(SR, HOP, **bad)
    assert V.check_args(SR, HOP, attack_s=4096 * HOP / SR)[3] == 4096 and V.check_args(SR, HOP, rate_hz=SR / HOP / 2 - 0.01)[1] < 2 ** 31
    for bad in (dict(sample_rate=None, hop_size=HOP), dict(sample_rate=SR, hop_size=None), dict(sample_rate=SR, hop_size=0), dict(sample_rate=float("nan"), hop_size=HOP)):
        with pytest.raises(ValueError):
            V.check_args(**bad)
    rows = V.params_rows(3, SR, HOP, depth_cents=[0.0, 25.0, 100.0], rate_hz=6.0)
    assert [r[0] for r in rows] == [0, 400, 1600] and len({r[1] for r in rows}) == 1 and all(r[2:] == d[2:] for r in rows)
    with pytest.raises(ValueError):
        V.params_rows(3, SR, HOP, depth_cents=[1.0, 2.0])
    with pytest.raises(ValueError):
        V.params_rows(2, SR, HOP, depth_cents=[1.0, 2000.0])
    t = V.params(2, SR, HOP, "cpu", rate_hz=[5.0, 6.0])
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, 6) and t[:, 0].tolist() == [800, 800] and t[0, 1] < t[1, 1]
    assert V.depth_q_of_tokens([None, 0.0, float("nan"), 12.5], 6).tolist() == [-1, 0, -1, 200, -1, -1]
    with pytest.raises(ValueError):
        V.depth_q_of_tokens([1201.0])


def test_python_layer_refuses_cpu_tensors():
    from visinger_amd import _lib, vibrato as V
    x = torch.zeros(1, 4)
    with pytest.raises(_lib.VisingerHipError):
        V.vibrato(x, torch.ones(1, 4, dtype=torch.int64), torch.ones(1, 1, dtype=torch.int32), torch.zeros(1, 6, dtype=torch.int32))
    with pytest.raises(_lib.VisingerHipError):
        V.vibrato(None, None, None, None)
    with pytest.raises(_lib.VisingerHipError):
        V.vibrato(x, None, None, None, pred=x)


def test_entry_point_validates_its_arguments_before_anything_is_launched():
    from visinger_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below is refused on the host
    ok = [p, 1, p, None, p, None, p, p, ctypes.c_void_p(8192), ctypes.c_void_p(12288), 2, 8, 4, None]

    def call(**change):
        names = ["curve", "stride", "mel2ph", "lengths", "notes", "depth", "params", "sine", "offset_q", "curve_out", "B", "T", "T_ph", "stream"]
        a = list(ok)
        for k, v in change.items():
            a[names.index(k)] = v
        return L.vs_pitch_vibrato(*a)

    for bad in (dict(curve=None), dict(mel2ph=None), dict(notes=None), dict(params=None), dict(sine=None), dict(offset_q=None), dict(curve_out=None),
                dict(B=0), dict(T=0), dict(T_ph=0), dict(T=1 << 31), dict(stride=0), dict(stride=3), dict(stride=2, curve=ctypes.c_void_p(4100)),
                dict(B=1 << 62), dict(curve_out=p), dict(offset_q=p), dict(curve_out=ctypes.c_void_p(8192))):
        assert call(**bad) != _lib.VS_OK, bad
        assert b"vs_pitch_vibrato" in L.vs_last_error()


def test_driver_and_model_refusals_come_before_any_launch():
    from visinger_amd import synth
    from visinger_amd.models.visinger import VISinger
    assert list(synth.OPTIONS) == ["resample_to", "guide_dynamics", "limit", "guide_correct", "guide_align", "guide_track"]
    it = dict(text_tokens=np.array([3, 4, 5]), pitch_tokens=np.array([0, 60, 62]), dur_tokens=np.array([1, 2, 3]), mel2ph=np.array([1, 1, 2, 2, 3, 3]))

    class WithPitch(torch.nn.Linear):
        hparams = {"use_pitch_embed": True}

    class NoPitch(torch.nn.Linear):
        hparams = {"use_pitch_embed": False}
    model = WithPitch(2, 2)                        # never run: the arguments are checked first
    fps = SR / HOP
    for bad, match in ((dict(sample_rate=SR, depth=1.0), "vibrato takes"), (dict(depth_cents=10.0), "sample_rate"), ("on", "dict"),
                       (dict(sample_rate=SR, rate_hz=0.0), "rate_hz"), (dict(sample_rate=SR, rate_hz=fps / 2), "rate_hz"),
                       (dict(sample_rate=SR, attack_s=4097 / fps), "attack_s"), (dict(sample_rate=SR, depth_cents=[1.0, 2.0]), "batch of 1")):
        with pytest.raises(ValueError, match=match):
            synth.synthesize(model, [it], HOP, vibrato=bad)
    with pytest.raises(ValueError, match="use_pitch_embed"):
        synth.synthesize(NoPitch(2, 2), [it], HOP, vibrato=dict(sample_rate=SR))
    with pytest.raises(ValueError, match="one per token"):
        synth.synthesize(model, [dict(it, note_of_token=np.array([0, 1]))], HOP, vibrato=dict(sample_rate=SR))
    with pytest.raises(ValueError, match="vibrato_depth_cents"):
        synth.synthesize(model, [dict(it, vibrato_depth_cents=[0.0, 5000.0, 1.0])], HOP, vibrato=dict(sample_rate=SR))
    with pytest.raises(ValueError, match="voicing"):                     # an earlier refusal stays the first
        synth.synthesize(model, [it], HOP, voicing="tracker", vibrato=dict(depth=1.0))

    class Stub:
        hparams = {"use_pitch_embed": False}
    x = torch.zeros(1, 3)
    prm = torch.zeros(1, 6, dtype=torch.int32)
    with pytest.raises(ValueError, match="use_pitch_embed"):
        VISinger.forward(Stub(), x, x, x, x, infer=True, vibrato=prm)
    Stub.hparams = {"use_pitch_embed": True}
    with pytest.raises(ValueError, match="synthesis"):
        VISinger.forward(Stub(), x, x, x, x, infer=False, vibrato=prm)
    with pytest.raises(ValueError, match="vibrato"):
        VISinger.forward(Stub(), x, x, x, x, infer=True, note_of_token=prm)
