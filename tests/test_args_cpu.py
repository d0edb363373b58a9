"""The host-argument layer (visinger_amd/_args.py) on its host forms -- the GPU-tensor branch needs a GPU and is held by the graph-replay
tests of the control ops -- and the public functions that are written through it, held by value to what they returned before they were: every expected
value of RETURNS was produced by running the functions of the parent commit of the one that wrote them through the layer (the control ops first, the waveform
ops -- limiter, dynamics, resample -- later), and so were the exception types and the first refusals of REFUSED and REFUSED_PAIRS.  No GPU."""
import numpy as np
import pytest
import torch

from visinger_amd import _args, dynamics, guide_align, guide_correct, limiter, pitch, pitch_track, resample, synth, timing

INF, NAN = float("inf"), float("nan")

# per_item_f32(what, value, B, "cpu", positive): (value, B, positive, expected)
PER_ITEM = [
    (1.5, 1, False, [1.5]), (1.5, 3, False, [1.5] * 3), (-2, 3, False, [-2.0] * 3), (0, 1, False, [0.0]), (np.float32(0.25), 3, True, [0.25] * 3),
    ([4.0], 1, True, [4.0]), ([0, -100, 50.5], 3, False, [0.0, -100.0, 50.5]), ((1, 2, 3), 3, True, [1.0, 2.0, 3.0]),
    (np.array([7.0]), 1, False, [7.0]), (np.array([1, 2, 3]), 3, True, [1.0, 2.0, 3.0]), (np.array([0.1, 0.2, 0.3], np.float32), 3, True, [0.1, 0.2, 0.3]),
    (torch.tensor([3.0]), 1, False, [3.0]), (torch.tensor([1, 2, 3]), 3, True, [1.0, 2.0, 3.0]), (torch.tensor(2.5, dtype=torch.float64), 3, False, [2.5] * 3),
]
PER_ITEM_REFUSED = [
    ([1.0, 2.0], 3, False), ([1.0, 2.0, 3.0], 1, False), ([], 1, False), (np.zeros(2), 3, False), (torch.zeros(4), 3, False),
    (NAN, 1, False), (INF, 3, False), ([1.0, -INF, 2.0], 3, False), (np.array([NAN]), 1, False), (torch.tensor([1.0, NAN, 2.0]), 3, True),
    (0, 1, True), (0.0, 3, True), (-1.5, 3, True), ([1.0, 0.0, 2.0], 3, True), ([1.0, 2.0, -3.0], 3, True), (torch.tensor([-1.0]), 1, True),
    ("auto", 1, False), ("1.5", 3, False), ("123", 3, True), (["a"], 1, False),
]
# lengths_i64(who, name, value, B, upper, "cpu"): (value, B, upper, expected)
LENGTHS = [
    (None, 1, 10, None), (None, 3, 10, None), ([0], 1, 10, [0]), ([10], 1, 10, [10]), ([0, 5, 10], 3, 10, [0, 5, 10]), ((3, 2, 1), 3, 10, [3, 2, 1]),
    (np.array([4]), 1, 10, [4]), (np.array([1, 2, 3], np.int32), 3, 10, [1, 2, 3]), (torch.tensor([9]), 1, 10, [9]),
    (torch.tensor([0, 1, 2], dtype=torch.int32), 3, 2, [0, 1, 2]),
]
LENGTHS_REFUSED = [
    ([1, 2], 3, 10), ([1, 2, 3], 1, 10), ([], 1, 10), (np.array([1, 2]), 3, 10), (torch.tensor([1]), 3, 10),
    ([-1], 1, 10), ([0, -1, 3], 3, 10), ([11], 1, 10), ([0, 11, 3], 3, 10), (np.array([1, 2, 11]), 3, 10), (torch.tensor([-5]), 1, 10),
    ("ab", 1, 10), ("abc", 3, 10), (["x"], 1, 10),
]


@pytest.mark.parametrize("value,B,positive,want", PER_ITEM)
def test_per_item_f32_takes_every_host_form(value, B, positive, want):
    got = _args.per_item_f32("factors", value, B, "cpu", positive=positive)
    assert got.dtype == torch.float32 and got.shape == (B,) and got.device.type == "cpu"
    assert got.tolist() == torch.tensor(want, dtype=torch.float32).tolist()


@pytest.mark.parametrize("value,B,positive", PER_ITEM_REFUSED)
def test_per_item_f32_refuses(value, B, positive):
    with pytest.raises(ValueError):
        _args.per_item_f32("factors", value, B, "cpu", positive=positive)


@pytest.mark.parametrize("value,B,upper,want", LENGTHS)
def test_lengths_i64_takes_every_host_form(value, B, upper, want):
    got = _args.lengths_i64("op", "lengths", value, B, upper, "cpu")
    if want is None:
        assert got is None
    else:
        assert got.dtype == torch.int64 and got.shape == (B,) and got.device.type == "cpu" and got.tolist() == want


@pytest.mark.parametrize("value,B,upper", LENGTHS_REFUSED)
def test_lengths_i64_refuses(value, B, upper):
    with pytest.raises(ValueError):
        _args.lengths_i64("op", "lengths", value, B, upper, "cpu")


def test_predicates():
    for v, lo, hi, want in ((0, 0, 4, True), (4, 0, 4, True), (5, 0, 4, False), (-1, 0, 4, False), (np.int64(3), 0, 4, True), (True, 0, 4, False),
                            (2.0, 0, 4, False), ("2", 0, 4, False), (None, 0, 4, False)):
        assert bool(_args.is_int(v, lo, hi)) is want, (v, lo, hi)
    for v, lo, hi, want in ((0.0, 0, 2, True), (2, 0, 2, True), (2.5, 0, 2, False), (-0.5, 0, 2, False), (np.float32(1.5), 0, 2, True), (True, 0, 2, False),
                            (NAN, 0, 2, False), (INF, 0, INF, False), (1e30, 0, INF, True), ("1", 0, 2, False), (None, 0, 2, False)):
        assert bool(_args.is_real(v, lo, hi)) is want, (v, lo, hi)
    assert _args.is_real(-1e30) and not _args.is_real(NAN) and not _args.is_real(-INF)
    eight, nine = list(range(8)), list(range(9))
    assert _args.short(eight) is eight and _args.short(nine) == eight + ["..."] and len(nine) == 9
    assert _args.vp(None) is None
    with pytest.raises(_args.VisingerHipError, match="lengths"):          # a host tensor is no GPU tensor, whatever its dtype and shape
        _args.gpu_tensor("op", "lengths", torch.zeros(3, dtype=torch.int64), torch.int64, (3,))
    with pytest.raises(_args.VisingerHipError):
        _args.gpu_tensor("op", "lengths", [1, 2, 3], torch.int64, (3,))


def design4(*args, **kw):
    return resample.design(*args, **kw)[:4]


GAIN_TOP, GATE_TOP = dynamics.GAIN_LIMIT / dynamics.UNITS_PER_DB, dynamics.GATE_LIMIT / dynamics.UNITS_PER_DB
# (function, positional arguments, keywords, what the function returned at the parent commit); tensors are compared through .tolist()
RETURNS = [
    (pitch.cents_tensor, (1.5, 3, "cpu"), {}, [1.5, 1.5, 1.5]),
    (pitch.cents_tensor, ([0, -100, 50.5], 3, "cpu"), {}, [0.0, -100.0, 50.5]),
    (pitch.cents_tensor, (np.array([1, 2]), 2, "cpu"), {}, [1.0, 2.0]),
    (pitch.cents_tensor, (torch.tensor([3.0]), 1, "cpu"), {}, [3.0]),
    (pitch.cents_tensor, (True, 2, "cpu"), {}, [1.0, 1.0]),
    (pitch.cents_tensor, (np.float32(0.1), 1, "cpu"), {}, [0.10000000149011612]),
    (pitch.cents_tensor, ((7,), 1, "cpu"), {}, [7.0]),
    (timing.factor_tensor, (2, 2, "cpu"), {}, [2.0, 2.0]),
    (timing.factor_tensor, ([0.5, 1.25], 2, "cpu"), {}, [0.5, 1.25]),
    (timing.factor_tensor, (torch.tensor([1.0, 2.0, 3.0]), 3, "cpu"), {}, [1.0, 2.0, 3.0]),
    (timing.factor_tensor, (np.float64(1e-3), 1, "cpu"), {}, [0.0010000000474974513]),
    (timing.factor_tensor, (np.array([64.0, 0.015625]), 2, "cpu"), {}, [64.0, 0.015625]),
    (guide_align.check_args, (), {}, (64, 48, 24, 32, 64, 0, 0)),
    (guide_align.check_args, (), dict(octave_fold=True, cap=0, w_voiced_rest=4096, w_unvoiced_note=1, drift=2, drift_cap=3), (0, 4096, 1, 2, 3, 1, 0)),
    (guide_align.check_args, (), dict(octave_fold=1, drift=np.int64(7)), (64, 48, 24, 7, 64, 1, 0)),
    (guide_correct.check_args, (), {}, (1024, 256, 256, 4800, 0, 0)),
    (guide_correct.check_args, (), dict(window=0, strength=0.5, vibrato=2.0, wild_cents=16384.0, octave_fold=True), (0, 128, 512, 262144, 1, 0)),
    (guide_correct.check_args, (), dict(window=np.int32(7), strength=1, vibrato=0, wild_cents=0.03, octave_fold=0), (7, 256, 0, 0, 0, 0)),
    (guide_correct.check_args, (), dict(strength=0.001, vibrato=1.998, wild_cents=12.34), (1024, 0, 511, 197, 0, 0)),
    (pitch_track.check_args, (256, 22050), {}, 680),
    (pitch_track.check_args, (128, 16000, 80.0, 800.0, 512, 0.1, 0.0, 10), {}, 512),
    (pitch_track.check_args, (256, 44100), dict(f0_min=65.0), 1358),
    (pitch_track.check_args, (np.int64(300), 24000), dict(f0_min=50, f0_max=1100, window=480), 480),
    (limiter.check_args, (), {}, (0.8912509083747864, 128)),
    (limiter.check_args, (), dict(ceiling_db=0, window=0), (1.0, 0)),
    (limiter.check_args, (), dict(ceiling_db=-120.0, window=1024), (9.999999974752427e-07, 1024)),
    (limiter.check_args, (), dict(ceiling_db=np.float32(-6.0), window=np.int64(7)), (0.5011872053146362, 7)),
    (limiter.check_args, (), dict(ceiling_db=-3), (0.7079457640647888, 128)),
    (dynamics.check_args, (), {}, (1, 12, 256, 1020, 2041, -5953, True)),
    (dynamics.check_args, (), dict(half_width=0, window=0, depth=0, max_boost_db=0, max_cut_db=0, gate_db=-GATE_TOP, mode="absolute"), (0, 0, 0, 0, 0, -65536, False)),
    (dynamics.check_args, (), dict(half_width=8, window=1024, depth=1, max_boost_db=GAIN_TOP, max_cut_db=GAIN_TOP, gate_db=GATE_TOP), (8, 1024, 256, 4096, 4096, 65536, True)),
    (dynamics.check_args, (), dict(half_width=np.int32(2), window=np.int64(5), depth=np.float32(0.5), max_boost_db=np.float64(6.0), max_cut_db=np.float32(3.5),
                                   gate_db=np.float32(-40.0)), (2, 5, 128, 510, 298, -3402, True)),
    (dynamics.db_to_units, (0,), {}, 0),
    (dynamics.db_to_units, (12.0,), {}, 1020),
    (dynamics.db_to_units, (-70,), {}, -5953),
    (dynamics.db_to_units, (np.float32(1.5),), {}, 128),
    (dynamics.db_to_units, (0.5 / dynamics.UNITS_PER_DB,), {}, 0),                # (half a unit: rint goes to even)
    (resample.check_quality, (), {}, (32, 10.0, 0.9)),
    (resample.check_quality, (), dict(zeros=1, beta=1e-3, rolloff=1), (1, 0.001, 1.0)),
    (resample.check_quality, (), dict(zeros=1 << 16, beta=100, rolloff=1e-6), (65536, 100.0, 1e-06)),
    (resample.check_quality, (), dict(zeros=np.int64(16), beta=np.float32(8.5), rolloff=np.float64(0.95)), (16, 8.5, 0.95)),
    (resample.ratio, (24000, 44100), {}, (147, 80)),
    (resample.ratio, (1, 1), {}, (1, 1)),
    (resample.ratio, ((1 << 31) - 1, 1), {}, (1, 2147483647)),
    (resample.ratio, (np.int64(48000), np.int32(16000)), {}, (1, 3)),
    (resample.out_length, (0, 24000, 44100), {}, 0),
    (resample.out_length, (1, 24000, 44100), {}, 2),
    (resample.out_length, (1 << 40, 24000, 44100), {}, 2020352616039),
    (resample.out_length, (np.int64(4097), 48000, np.int64(24000)), {}, 2049),
    (design4, (24000, 44100), {}, (147, 80, 4704, 65)),
    (design4, (24000, 44100), dict(zeros=16), (147, 80, 2352, 33)),
    (design4, (1, 1), {}, (1, 1, 32, 65)),
    (design4, (np.int64(48000), np.int64(24000)), dict(zeros=np.int64(8), beta=np.float32(9.0), rolloff=np.float32(0.5)), (1, 2, 16, 33)),
    (dynamics._offset_tensor, (None, 3, "cpu"), {}, None),
    (dynamics._offset_tensor, (5, 3, "cpu"), {}, [5, 5, 5]),
    (dynamics._offset_tensor, (-dynamics.OFFSET_LIMIT, 2, "cpu"), {}, [-131072, -131072]),
    (dynamics._offset_tensor, ([0, -131072, 131072], 3, "cpu"), {}, [0, -131072, 131072]),
    (dynamics._offset_tensor, ((1, 2), 2, "cpu"), {}, [1, 2]),
    (dynamics._offset_tensor, (np.int64(-7), 2, "cpu"), {}, [-7, -7]),
    (dynamics._offset_tensor, (np.array([1, 2, 3]), 3, "cpu"), {}, [1, 2, 3]),
    (dynamics._offset_tensor, (np.array([4], np.int32), 1, "cpu"), {}, [4]),
    (dynamics._offset_tensor, (torch.tensor([9, -9]), 2, "cpu"), {}, [9, -9]),
    (dynamics._offset_tensor, (torch.tensor(3), 2, "cpu"), {}, [3, 3]),
]
# host forms the offset rule refused at the parent commit (ValueError): (value, B)
OFFSET_REFUSED = [(1.5, 2), (True, 2), (131073, 2), ([1], 2), ("12", 2), ([1.0, 2.0], 2), ([1, 1 << 18], 2), ([True, 1], 2), (torch.tensor([1.0, 2.0]), 2), ([], 1)]


@pytest.mark.parametrize("fn,args,kw,want", RETURNS, ids=[f"{fn.__module__.split('.')[-1]}.{fn.__name__}-{n}" for n, (fn, *_) in enumerate(RETURNS)])
def test_public_functions_return_what_they_did(fn, args, kw, want):
    got = fn(*args, **kw)
    if torch.is_tensor(got):
        assert got.dtype == (torch.int32 if fn is dynamics._offset_tensor else torch.float32) and got.device.type == "cpu"
        got = got.tolist()
    assert got == want and type(got) is type(want)


@pytest.mark.parametrize("value,B", OFFSET_REFUSED)
def test_offset_rule_refuses(value, B):
    with pytest.raises(ValueError, match="offset_units"):
        dynamics._offset_tensor(value, B, "cpu")


def test_align_items_names_the_item_of_a_bad_offset():
    item = dict(text_tokens=np.arange(1, 4), pitch_tokens=np.array([3, 4, 5]), dur_tokens=np.array([2, 2, 1]), mel2ph=np.array([1, 1, 2, 2, 3]),
                note_midi=np.array([60.0, 62.0, 0.0], np.float32), f0=np.full(7, 260.0, np.float32))
    plain = {k: v for k, v in item.items() if k not in ("f0", "note_midi")}
    for bad in (NAN, INF, "3"):
        with pytest.raises(ValueError, match="item 1"):
            synth.align_items([plain, dict(item, guide_offset_cents=bad)], "cpu")


ITEM = dict(text_tokens=np.arange(1, 4), pitch_tokens=np.array([3, 4, 5]), dur_tokens=np.array([2, 2, 1]), mel2ph=np.array([1, 1, 2, 2, 3]))
SUNG = dict(ITEM, guide_wav=np.zeros(4096, np.float32))                      # guide_track is looked at only when an item carries a recording
RATES, TRACK = dict(sample_rate=24000, output_rate=44100), dict(sample_rate=24000, f0_min=65, f0_max=1000)
# synthesize(None, [item], 8, **{option: bad}) is refused before the model is looked at: (option, bad value, item, exception type, pattern).  For each option
# dict: not a dict, an unknown key, a missing key where one is required, a value out of range.  Types and patterns are the parent commit's; its driver refused
# the values and keys of guide_correct, guide_align and guide_track in the pre-passes, behind its first look at the model -- the rows hold that it is a
# ValueError with the pre-pass's words, and now an early one.
REFUSED = [
    ("resample_to", [24000, 44100], ITEM, ValueError, "resample_to"), ("resample_to", dict(RATES, quality=3), ITEM, ValueError, "resample_to takes"),
    ("resample_to", dict(sample_rate=24000), ITEM, ValueError, "resample_to"), ("resample_to", dict(RATES, output_rate=0), ITEM, ValueError, "sr_out"),
    ("resample_to", dict(RATES, zeros=0), ITEM, ValueError, "zeros"), ("resample_to", dict(RATES, output_rate=8001), ITEM, ValueError, "budget"),
    ("guide_dynamics", 3, ITEM, ValueError, "guide_dynamics"), ("guide_dynamics", dict(bogus=1), ITEM, ValueError, "guide_dynamics takes"),
    ("guide_dynamics", dict(depth=1.5), ITEM, ValueError, "depth"), ("guide_dynamics", dict(mode="x"), ITEM, ValueError, "mode"),
    ("limit", 3, ITEM, ValueError, "limit|ceiling_db|window"), ("limit", dict(bogus=1), ITEM, ValueError, "limit|ceiling_db|window"),
    ("limit", dict(ceiling_db=1), ITEM, ValueError, "limit|ceiling_db|window"), ("limit", dict(window=2000), ITEM, ValueError, "limit|ceiling_db|window"),
    ("guide_correct", 3, ITEM, ValueError, "dict"), ("guide_correct", dict(bogus=1), ITEM, ValueError, "guide_correct takes"),
    ("guide_correct", dict(window=2000), ITEM, ValueError, "window"), ("guide_correct", dict(offset_cents="a"), ITEM, ValueError, "offset_cents"),
    ("guide_align", 3, ITEM, ValueError, "guide_align must be a dict"), ("guide_align", dict(bogus=1), ITEM, ValueError, "guide_align takes"),
    ("guide_align", dict(cap=-1), ITEM, ValueError, "cap"), ("guide_align", dict(offset_cents=INF), ITEM, ValueError, "offset_cents"),
    ("guide_track", 3, SUNG, ValueError, "guide_track"), ("guide_track", dict(TRACK, bogus=1), SUNG, ValueError, "guide_track takes"),
    ("guide_track", dict(f0_min=65), SUNG, ValueError, "sample_rate"), ("guide_track", dict(TRACK, f0_min=-1), SUNG, ValueError, "f0_min"),
    ("guide_track", dict(TRACK, recording_rate=0), SUNG, ValueError, "sr_in"), ("guide_track", None, SUNG, ValueError, "guide_track"),
]
# two bad options in one call: the first refusal, recorded from the parent commit (the order of OPTIONS, "level" without guide_dynamics behind guide_dynamics)
REFUSED_PAIRS = [
    (dict(resample_to=[1], guide_dynamics=3), ITEM, "resample_to must be a dict"),
    (dict(guide_dynamics=dict(bogus=1), limit=dict(window=-1)), ITEM, "guide_dynamics takes"),
    (dict(limit=dict(window=-1), guide_correct=3), ITEM, "window must be an integer"),
    (dict(guide_correct=3, guide_align=3), ITEM, "guide_correct must be a dict"),
    (dict(limit=3), dict(ITEM, level=np.ones(5, np.float32)), "an item carries 'level'"),
    (dict(resample_to=[1]), dict(ITEM, level=np.ones(5, np.float32)), "resample_to must be a dict"),
]


@pytest.mark.parametrize("option,bad,item,exc,pattern", REFUSED, ids=[f"{o}-{n}" for n, (o, *_) in enumerate(REFUSED)])
def test_synthesize_refuses_a_bad_option_before_it_looks_at_the_model(option, bad, item, exc, pattern):
    with pytest.raises(exc, match=pattern):
        synth.synthesize(None, [item], 8, **{option: bad})


@pytest.mark.parametrize("bad,item,pattern", REFUSED_PAIRS, ids=[f"pair-{n}" for n in range(len(REFUSED_PAIRS))])
def test_synthesize_refuses_the_first_of_two_bad_options(bad, item, pattern):
    with pytest.raises(ValueError, match=pattern):
        synth.synthesize(None, [item], 8, **bad)


def test_option_table_lists_the_six_option_dicts_in_the_order_they_are_checked():
    assert list(synth.OPTIONS) == ["resample_to", "guide_dynamics", "limit", "guide_correct", "guide_align", "guide_track"]
    assert synth._option("limit", None) is None and synth._option("limit", {}) == {}
    given = dict(ceiling_db=-3.0)
    got = synth._option("limit", given)
    assert got == given and got is not given                                 # a copy: the pre-passes pop from it
    with pytest.raises(ValueError, match="hop_size"):
        synth.synthesize(None, [ITEM], 4096, guide_dynamics={})
    assert synth.guide_items([ITEM], 8, "cpu", **TRACK)[0] is not ITEM       # no recording: a copy, nothing tracked, the keywords checked through the same row


ALLOWED = dict(a=1, b=2, c=3)


def test_key_check():
    assert _args.keys("opts", None, ALLOWED, none_ok=True) is None
    for given in ({}, dict(a=5), dict(ALLOWED), dict(c=None, a=0)):
        got = _args.keys("opts", given, ALLOWED, none_ok=True)
        assert got == given and got is not given and type(got) is dict
        assert _args.keys("opts", given, tuple(ALLOWED)) == given            # the allowed keys as any container of names
    for bad in (dict(d=1), dict(a=1, d=2), {1: 2}):
        with pytest.raises(ValueError, match="opts takes a, b, c"):
            _args.keys("opts", bad, ALLOWED)
    for bad in (3, "a", ["a"], ("a",), {"a"}, 1.5, True):
        with pytest.raises(ValueError, match="opts must be a dict"):
            _args.keys("opts", bad, ALLOWED, none_ok=True)
    with pytest.raises(ValueError, match="opts must be a dict"):                # None only where it is allowed
        _args.keys("opts", None, ALLOWED)


def test_waveform_and_out_checks_refuse_a_host_tensor():
    wav = torch.zeros(2, 100)
    for bad in (wav, wav.double(), wav.numpy(), None, wav[0]):
        with pytest.raises(_args.VisingerHipError, match="op: wav"):
            _args.waveform("op", bad)
    for bad in (wav, torch.zeros(2, 99), wav.double(), wav.numpy(), 3):
        with pytest.raises(_args.VisingerHipError, match="op: out"):
            _args.out_like("op", wav, bad)
    new = _args.out_like("op", wav, None)                                    # None: a new tensor of wav's kind
    assert new.shape == wav.shape and new.dtype == wav.dtype and new.data_ptr() != wav.data_ptr()


def test_item_seeds_expands_one_integer():
    from visinger_amd import sampling
    top = sampling.SEED_LIMIT
    assert sampling.item_seeds(11, 3) == [11, 12, 13] and sampling.item_seeds(top - 1, 3) == [top - 1, 0, 1] and sampling.item_seeds(5, 0) == []
    assert sampling.item_seeds([7, 7], 2) == [7, 7] and sampling.item_seeds(np.array([1, 2]), 2) == [1, 2]
    for bad, n, pattern in ((top, 1, "seed"), (-1, 2, "seed"), ([1], 2, "1 seeds for 2 items"), ([1, 2], 1, "2 seeds for 1 items"), ([1.5], 1, "seed")):
        with pytest.raises(ValueError, match=pattern):
            sampling.item_seeds(bad, n)


def test_pad_rows_copies_and_fills():
    rows = [np.array([1, 2, 3]), [4], np.array([], np.int64)]
    got = synth._pad_rows(rows, torch.long)
    assert got.dtype == torch.long and got.tolist() == [[1, 2, 3], [4, 0, 0], [0, 0, 0]]
    got[0, 0] = 9
    assert rows[0][0] == 1                                                   # a copy: the caller's arrays stay as they are
    assert synth._pad_rows([np.array([0.5, 2.0])], torch.float32, width=4, fill=1).tolist() == [[0.5, 2.0, 1.0, 1.0]]
