"""The host-argument layer (visinger_amd/_args.py) on its host forms -- the GPU-tensor branch needs a GPU and is held by the graph-replay
tests of the control ops -- and the public functions that are written through it, held by value to what they returned before they were: every expected
value of RETURNS was produced by running the functions of the parent commit, the last one without this layer.  No GPU."""
import numpy as np
import pytest
import torch

from visinger_amd import _args, guide_align, guide_correct, pitch, pitch_track, synth, timing

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
]


@pytest.mark.parametrize("fn,args,kw,want", RETURNS, ids=[f"{fn.__module__.split('.')[-1]}.{fn.__name__}-{n}" for n, (fn, *_) in enumerate(RETURNS)])
def test_public_functions_return_what_they_did(fn, args, kw, want):
    got = fn(*args, **kw)
    if torch.is_tensor(got):
        assert got.dtype == torch.float32 and got.device.type == "cpu"
        got = got.tolist()
    assert got == want and type(got) is type(want)


def test_align_items_names_the_item_of_a_bad_offset():
    item = dict(text_tokens=np.arange(1, 4), pitch_tokens=np.array([3, 4, 5]), dur_tokens=np.array([2, 2, 1]), mel2ph=np.array([1, 1, 2, 2, 3]),
                note_midi=np.array([60.0, 62.0, 0.0], np.float32), f0=np.full(7, 260.0, np.float32))
    plain = {k: v for k, v in item.items() if k not in ("f0", "note_midi")}
    for bad in (NAN, INF, "3"):
        with pytest.raises(ValueError, match="item 1"):
            synth.align_items([plain, dict(item, guide_offset_cents=bad)], "cpu")


def test_pad_rows_copies_and_fills():
    rows = [np.array([1, 2, 3]), [4], np.array([], np.int64)]
    got = synth._pad_rows(rows, torch.long)
    assert got.dtype == torch.long and got.tolist() == [[1, 2, 3], [4, 0, 0], [0, 0, 0]]
    got[0, 0] = 9
    assert rows[0][0] == 1                                                   # a copy: the caller's arrays stay as they are
    assert synth._pad_rows([np.array([0.5, 2.0])], torch.float32, width=4, fill=1).tolist() == [[0.5, 2.0, 1.0, 1.0]]
