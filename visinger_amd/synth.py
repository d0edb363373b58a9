"""Batched synthesis driver: what the reference does one utterance at a time in
``tasks/visinger.py:244-263`` (``test_step``) and ``inference/visinger.py:91-100``, done in length-bucketed batches on
the MI355X-native model, plus the reference's wav normalisation (``utils/audio/io.py:8-15``: peak-normalise, scale to
int16).  Host-side plumbing only."""
import numpy as np
import torch

from . import _args as A
from . import dynamics
from . import guide_align as guide_align_ops
from . import guide_correct as guide_correct_ops
from . import limiter, pitch, pitch_track, resample, sampling, timing
from . import loudness as loudness_ops
from . import vibrato as vibrato_ops


def bucket_by_length(lengths, max_frames_per_batch, max_items_per_batch=256, keys=None):
    """Sort by length (descending) and cut batches under a padded-frame budget (the reference's batch_by_size idea,
    utils/commons/dataset_utils.py:181-191, without its dataset plumbing).  Returns lists of item indices.
    keys (optional, one per item): items of different key never share a batch (batches are cut where the key changes)."""
    order = sorted(range(len(lengths)), key=lambda i: ((keys[i] if keys is not None else 0), -int(lengths[i])))
    batches, cur = [], []
    for i in order:
        longest = int(lengths[cur[0]]) if cur else int(lengths[i])
        if cur and (longest * (len(cur) + 1) > max_frames_per_batch or len(cur) >= max_items_per_batch or
                    (keys is not None and keys[i] != keys[cur[0]])):
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return batches


def _buckets(lengths, max_frames_per_batch):
    """bucket_by_length over {item index: length}: lists of item indices"""
    order = list(lengths)
    for idx in bucket_by_length([lengths[i] for i in order], max_frames_per_batch):
        yield [order[j] for j in idx]


def _pad_rows(rows, dtype, width=None, fill=0):
    """host tensor [len(rows), width] (default: the longest row) whose row b begins with a copy of rows[b]; the rest is `fill`"""
    out = torch.full((len(rows), max(len(r) for r in rows) if width is None else width), fill, dtype=dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = torch.as_tensor(np.asarray(r), dtype=dtype)
    return out


def _check_curve(i, item, key):
    """ValueError, naming item i, unless the item's curve item[key] -- "f0" or "level" -- is None (or missing) or holds one value per frame of its mel2ph"""
    if item.get(key) is not None and np.shape(item[key]) != (len(item["mel2ph"]),):
        what, unit = ("guide", "one value in Hz per frame") if key == "f0" else ("level", "one value per frame")
        raise ValueError(f"item {i}: the {what} curve has {np.shape(item[key])} values for {len(item['mel2ph'])} frames ({unit})")


def collate(items, device):
    """items: dicts with int64 1-D arrays text_tokens, pitch_tokens, dur_tokens (T_ph) and mel2ph (T_mel); 0-padded.
    An item may carry "f0": a guide curve in Hz, one value per frame of its mel2ph (0 = unvoiced) -> batch["f0_hz"], fp32 [B, T_mel], padded
    with 0.  Either every item of a batch has one or none (synthesize keeps them apart); a length mismatch is a ValueError."""
    guided = ["f0" in it and it["f0"] is not None for it in items]
    if any(guided) and not all(guided):
        raise ValueError("items with and without a guide curve ('f0') cannot share a batch")
    Tph = max(len(it["text_tokens"]) for it in items)
    T = max(len(it["mel2ph"]) for it in items)
    out = {k: _pad_rows([it[k] for it in items], torch.long, Tph if k != "mel2ph" else T)
           for k in ("text_tokens", "pitch_tokens", "dur_tokens", "mel2ph")}
    out["spk_id"] = torch.as_tensor([int(it.get("spk_id", 0)) for it in items], dtype=torch.long)
    if guided and guided[0]:
        for b, it in enumerate(items):
            _check_curve(b, it, "f0")
        out["f0_hz"] = _pad_rows([it["f0"] for it in items], torch.float32, T)
    return {k: v.to(device) for k, v in out.items()}


def to_int16(wav, norm=True):
    """utils/audio/io.py:8-15: optional peak normalisation, then * 32767 -> int16."""
    wav = np.asarray(wav)
    if not np.issubdtype(wav.dtype, np.floating):
        wav = wav.astype(np.float32)
    # (the arithmetic stays in the array's own float type, as in the reference: an fp64 waveform is scaled in fp64 -- the int16 truncation
    #  of the two differs in the last bit; pinned byte for byte by tests/golden/save_wav.npz)
    if norm and wav.size:
        peak = np.abs(wav).max()
        if peak > 0:
            wav = wav / peak
    return (wav * 32767).astype(np.int16)


def save_wav(wav, path, sr, norm=False):
    """utils/audio/io.py:8-12: write `wav` (float, nominally in [-1, 1]) as 16-bit PCM to path[:-4] + '.wav'."""
    from scipy.io import wavfile
    wavfile.write(path[:-4] + ".wav", sr, to_int16(wav, norm=norm))


class StreamRotation:
    """Consecutive batches on alternating HIP streams (round 6).  A synthesis step is a chain: the prior transformers and the flow -- ~250 short,
    latency-bound launches that leave most of the chip idle -- then the HiFi-GAN generator, whose launches fill it.  Batches are independent (no op of the path
    mixes utterances), so batch i + 1 issued on a second stream runs its transformers in the gaps of batch i's generator: measured on one
    MI355X, B = 32 x T_mel = 1024: 72.0 -> 69.3 ms a batch; BASELINE configs[1] (B = 8, T_mel = 512): 9.85 -> 8.31 ms; configs[4]: 56.7 -> 54.2 ms
    (profiles/r06_stream_rotation_ab.txt); a third stream adds nothing.  Every launch of the library goes to torch's current stream and every workspace is
    allocated through torch's stream-aware allocator, so two steps in flight share the parameters, which are read-only, and the conv handles' packed weights.
    Those are NOT read-only on a cold model or after a parameter change: a handle folds and packs lazily on whichever stream meets it first, and its host-side key
    is valid before the pack kernels have run.  The library orders that itself (csrc/vs_internal.h StreamOrder): a launch that reads a handle on
    a stream other than the one its planes were produced on first waits, once per weight version and stream, for the producing stream; a re-pack first waits for
    the streams that have read the previous version (tests/test_stream_order_gpu.py).  NOT for the flow's
    FORWARD direction with log-det (its partial sums live in the conv handle: INTEGRATION.md 2) nor for training."""

    def __init__(self, n=2, timing=False):
        self.streams = [torch.cuda.Stream() for _ in range(max(1, int(n)))]
        self.count = 0
        self.timing = bool(timing)                # (events that can be timed against each other: the benchmark's per-batch statistics)
        cur = torch.cuda.current_stream()
        for st in self.streams:
            st.wait_stream(cur)                  # (inputs prepared on the caller's stream so far are visible)

    def run(self, fn):
        """fn() with the next stream of the rotation current; returns (fn's result, an event recorded behind it on that stream)"""
        st = self.streams[self.count % len(self.streams)]
        self.count += 1
        with torch.cuda.stream(st):
            out = fn()
            ev = torch.cuda.Event(enable_timing=self.timing)
            ev.record(st)
        return out, ev

    def join(self):
        """the caller's current stream waits for everything issued through the rotation"""
        cur = torch.cuda.current_stream()
        for st in self.streams:
            cur.wait_stream(st)


class GraphedStep:
    """One synthesis step (VISinger.forward(infer=True)) of a FIXED shape captured into a HIP graph and replayed: what a serving
    loop with recurring batch shapes does.  Every launch of the step goes to torch's current stream through the C ABI, nothing
    allocates with hipMalloc or synchronises with the host after the warm-up, so the ~700 launches of a step replay as one graph
    (tests/test_model_gpu.py::test_synthesis_step_is_graph_capturable).  Inputs are copied into the graph's static buffers.
    With seeds= (int64 CUDA tensor [B]; `noise` is then None) the step samples from the items' seeded streams (sampling.prior_sample), `takes` per item:
    the kernel reads the seeds from a static device buffer, so a replay under other seeds is that buffer overwritten.  takes / first_take / noise_scale
    are launch arguments: fixed by the capture.
    Pitch control: a batch with "f0_hz" (collate) is synthesised on that guide curve -- it sits among the static inputs like the tokens, so a replay under
    another curve is that buffer overwritten; cents= (anything pitch.cents_tensor takes) becomes a static fp32 [B] buffer the kernel reads, overwritten by
    __call__(cents=).  `voicing` is fixed by the capture.  With either, `f0_hz_out` is the static [B, T] buffer of the sung curve in Hz.
    Tempo control: tempo= (anything timing.factor_tensor takes) and ph_stretch= (fp32 [B, T_ph]) become static device buffers the retiming kernels read,
    overwritten by __call__(tempo=, ph_stretch=); max_frames is required with either: the frame capacity fixed by the capture (the step runs max_frames
    frames wide, an item is cut at it, `noise` has that many frames).  `frame_lengths_out` is the static int64 [B] buffer of the retimed lengths and
    `mel2ph_out` the retimed alignment.
    Vibrato: vibrato= (the int32 [B, 6] tensor of vibrato.params) becomes a static buffer the vibrato kernel reads, overwritten by __call__(vibrato=); a batch's
    "note_of_token" / "note_depth_q" sit among the static inputs like the tokens.  `vibrato_q_out` is the static int32 [B, T] buffer of the offsets."""

    @staticmethod
    def fingerprint(model):
        """(data_ptr, in-place version) of every parameter: changes with optimizer steps, load_state_dict and copy_ (not with edits
        through `.data`, like the packed-weight caches: call hipconv.repack_weights AND drop the graphs after such an edit)"""
        return tuple((p.data_ptr(), p._version) for p in model.parameters())

    # the optional static control buffers: attribute -> the device tensor of a value, for a step of B items of T_ph tokens
    CONTROLS = dict(seeds=lambda v, B, T_ph, dev: sampling.seeds_tensor(v), cents=lambda v, B, T_ph, dev: pitch.cents_tensor(v, B, dev),
                    tempo=lambda v, B, T_ph, dev: timing.factor_tensor(v, B, dev), ph_stretch=timing.stretch_tensor,
                    vibrato=lambda v, B, T_ph, dev: vibrato_ops.params_tensor(v, B, dev))
    # what a replay is told whose optional inputs are not the capture's, in the order they are compared
    _SAMPLE = "a graph captured with noise is replayed with noise, one captured with seeds with seeds"
    _PITCH = "a graph is replayed with the inputs it was captured with (guide curve and pitch shift included)"
    _TEMPO = "a graph captured with a tempo / token stretch is replayed with one (and one captured without, without)"
    _VIBRATO = "a graph captured with vibrato settings is replayed with some (and one captured without, without)"
    REFUSALS = dict(seeds=_SAMPLE, noise=_SAMPLE, f0_hz=_PITCH, cents=_PITCH, tempo=_TEMPO, ph_stretch=_TEMPO, vibrato=_VIBRATO)

    def _controls(self, **given):
        """{attribute: device tensor, or None where no value is given}"""
        size = (self.static["mel2ph"].shape[0], self.static["text_tokens"].shape[1], self.static["mel2ph"].device)
        return {k: None if given[k] is None else make(given[k], *size) for k, make in self.CONTROLS.items()}

    def __init__(self, model, batch, noise, mask_decoder, seeds=None, takes=1, first_take=0, noise_scale=1.0, voicing="guide", cents=None, tempo=None,
                 ph_stretch=None, max_frames=None, vibrato=None):
        if seeds is not None and noise is not None:
            raise ValueError("seeds and noise are two sources of the same sample: give one of them")
        if (tempo is not None or ph_stretch is not None) != (max_frames is not None):
            raise ValueError("tempo / ph_stretch need max_frames (the frame capacity the capture fixes), and max_frames needs one of them")
        self.weights = self.fingerprint(model)       # a replay never re-folds / re-packs weights: the graph is only valid for these
        self.static = {k: v.clone() for k, v in batch.items()}
        self.noise = None if seeds is not None else noise.clone()
        for k, t in self._controls(seeds=seeds, cents=cents, tempo=tempo, ph_stretch=ph_stretch, vibrato=vibrato).items():
            setattr(self, k, None if t is None else t.clone())
        sample = dict(noise=self.noise) if seeds is None else dict(seeds=self.seeds, takes=takes, first_take=first_take, noise_scale=noise_scale)
        self.f0_hz_out = self.frame_lengths_out = self.mel2ph_out = self.vibrato_q_out = None
        if "f0_hz" in batch or self.cents is not None:
            sample.update(f0_hz=self.static.get("f0_hz"), voicing=voicing, pitch_shift_cents=self.cents)
        if self.vibrato is not None:
            sample.update(vibrato=self.vibrato, note_of_token=self.static.get("note_of_token"), note_depth_q=self.static.get("note_depth_q"))
        if max_frames is not None:
            sample.update(tempo=self.tempo, ph_stretch=self.ph_stretch, max_frames=int(max_frames))

        def run():
            b = self.static
            ret = model(b["text_tokens"], b["pitch_tokens"], b["dur_tokens"], b["mel2ph"], spk_id=b["spk_id"], infer=True,
                        mask_decoder=mask_decoder, **sample)
            self.f0_hz_out, self.vibrato_q_out = ret.get("f0_hz"), ret.get("vibrato_q")
            self.frame_lengths_out, self.mel2ph_out = ret.get("frame_lengths"), ret.get("mel2ph")
            return ret["wav_out"]

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):           # warm-up off the capture: packs weights, sizes every workspace
            run()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = run()

    def __call__(self, batch, noise, seeds=None, cents=None, tempo=None, ph_stretch=None, vibrato=None):
        given = dict(noise=noise, f0_hz=batch.get("f0_hz"), seeds=seeds, cents=cents, tempo=tempo, ph_stretch=ph_stretch, vibrato=vibrato)
        for k, refusal in self.REFUSALS.items():
            if (given[k] is None) != ((self.static.get(k) if k == "f0_hz" else getattr(self, k)) is None):
                raise ValueError(refusal)
        for k, v in batch.items():
            self.static[k].copy_(v)
        if noise is not None:
            self.noise.copy_(noise)
        for k, t in self._controls(**given).items():
            if t is not None:
                getattr(self, k).copy_(t)
        self.graph.replay()
        return self.out          # the graph's STATIC output buffer: the next replay overwrites it (clone to keep it)


def _check_dynamics(o, hop_size):
    dynamics.check_args(**o)
    dynamics._check_hop("guide_dynamics", hop_size, dynamics.HOP_LIMIT)


def _check_track(o, hop_size):
    pitch_track.check_args(hop_size, **{k: v for k, v in o.items() if k != "recording_rate"})
    if o.get("recording_rate") is not None:
        resample.design(o["recording_rate"], o["sample_rate"])       # (ValueError for a rate out of range or a ratio over the table budget)


def _check_guide_op(o, ops, auto):
    """the check of guide_align / guide_correct: the op's own keywords, and offset_cents a finite number (with `auto`: or 'auto')"""
    ops.check_args(**{k: v for k, v in o.items() if k in ops.DEFAULTS})
    offset = o.get("offset_cents", 0.0)
    if not (auto and isinstance(offset, str) and offset == "auto") and not (isinstance(offset, (int, float)) and abs(offset) < float("inf")):
        raise ValueError(f"offset_cents must be a finite number{' or auto' if auto else ''}, got {offset!r}")


# The option dicts of synthesize, in the order they are checked: name -> (the keys it must have, the keys it may have, the check of its values -- the op's own
# check_args or design -- called with the dict and hop_size).  guide_items, align_items and correct_items check their keywords through the same rows.
OPTIONS = dict(
    resample_to=(("sample_rate", "output_rate"), ("sample_rate", "output_rate", *resample.DEFAULTS),
                 lambda o, hop_size: resample.design(o["sample_rate"], o["output_rate"], **{k: o[k] for k in o if k in resample.DEFAULTS})),
    guide_dynamics=((), tuple(dynamics.DEFAULTS), _check_dynamics),
    limit=((), tuple(limiter.DEFAULTS), lambda o, hop_size: limiter.check_args(**o)),
    guide_correct=((), ("midi_of_token", "offset_cents", *guide_correct_ops.DEFAULTS), lambda o, hop_size: _check_guide_op(o, guide_correct_ops, True)),
    guide_align=((), ("midi_of_token", "offset_cents", *guide_align_ops.DEFAULTS), lambda o, hop_size: _check_guide_op(o, guide_align_ops, False)),
    guide_track=(("sample_rate",), ("sample_rate", "recording_rate", "f0_min", "f0_max", "window", "threshold", "silence", "path"), _check_track))


def _option(name, given, hop_size=None):
    """a checked copy of the option dict `name` (a row of OPTIONS), or None for None; ValueError: no dict, an unknown or missing key, a value its check refuses"""
    required, allowed, check = OPTIONS[name]
    opts = A.keys(name, given, allowed, none_ok=True)
    if opts is not None:
        if not all(k in opts for k in required):
            raise ValueError(f"{name} must contain {' and '.join(required)}, got {sorted(opts)}")
        check(opts, hop_size)
    return opts


def _check_vibrato(given, hop_size, items, model):
    """the check of synthesize(vibrato=): a dict of vibrato.DEFAULTS keys -- each a number or one value per item -- plus the required sample_rate; the items'
    "note_of_token" and "vibrato_depth_cents" hold one value per token; the model has a pitch condition.  Returns (the six integers of every item, {item index:
    its note_depth_q row} for the items with "vibrato_depth_cents"); ValueError otherwise.  Checked on its own, not through OPTIONS: that table's order is
    the order of the first refusals of a call, which this option leaves as it is."""
    opts = A.keys("vibrato", given, ("sample_rate", *vibrato_ops.DEFAULTS))
    if "sample_rate" not in opts:
        raise ValueError(f"vibrato must contain sample_rate (the model's), got {sorted(opts)}")
    rows = vibrato_ops.params_rows(len(items), opts.pop("sample_rate"), hop_size, **opts)
    depths = {}
    for i, it in enumerate(items):
        for key in ("note_of_token", "vibrato_depth_cents"):
            if it.get(key) is not None and np.shape(it[key]) != (len(it["text_tokens"]),):
                raise ValueError(f"item {i}: {key} has {np.shape(it[key])} values for {len(it['text_tokens'])} tokens (one per token)")
        if it.get("vibrato_depth_cents") is not None:
            depths[i] = vibrato_ops.depth_q_of_tokens(it["vibrato_depth_cents"])
    if not getattr(model, "hparams", {}).get("use_pitch_embed"):
        raise ValueError("vibrato needs a model with use_pitch_embed: this one has no pitch condition")
    return rows, depths


def _check_loudness(given, resample_to):
    """the check of synthesize(loudness=): a dict of loudness.DEFAULTS keys plus the required sample_rate, the model's; the rate the stage measures at --
    resample_to's output_rate when the call converts, else sample_rate -- is one loudness.check_rate takes.  Returns (the rate it measures at, the DEFAULTS keys
    given); ValueError otherwise.  Checked on its own like vibrato, not through OPTIONS, behind that table's refusals and before the model is looked at."""
    opts = A.keys("loudness", given, ("sample_rate", *loudness_ops.DEFAULTS))
    if "sample_rate" not in opts:
        raise ValueError(f"loudness must contain sample_rate (the model's), got {sorted(opts)}")
    loudness_ops.check_args(**opts)
    rate = opts.pop("sample_rate")
    if resample_to is not None:
        if resample_to["sample_rate"] != rate:
            raise ValueError(f"loudness: sample_rate = {rate!r} is not resample_to's sample_rate = {resample_to['sample_rate']!r} (both are the model's)")
        try:
            loudness_ops.check_rate(resample_to["output_rate"])
        except ValueError as e:
            raise ValueError(f"loudness measures at resample_to's output_rate: {e}") from None
        rate = resample_to["output_rate"]
    return rate, opts


def guide_items(items, hop_size, device, max_frames_per_batch=32768, fit=True, level=None, **track):
    """Copies of `items` in which a recording "guide_wav" -- a 1-D float array -- is replaced by "f0": its pitch curve, tracked on the device
    (pitch_track.extract_f0(**track), which needs sample_rate, the model's) in length buckets -- zero-padded, the lengths in a device tensor -- read back and fitted
    to the item's len(mel2ph): a longer curve is cut there, a shorter one padded with 0 (unvoiced: vs_f0_norm_interp bridges it like any gap).  Items without a
    recording are passed on as they are.  fit=False: the curve keeps its own frames, the recording's timeline (align_items takes it from there).
    The recordings are at track["recording_rate"] Hz (default: sample_rate), an item's own "guide_sr" going before it.  A bucket at another rate than sample_rate
    is converted on the device first (resample.resample) and tracked from there without a trip to the host: the converted lengths travel as the
    device tensor the converter wrote.  Such a recording of n samples counts out_length(n) = ceil(n sample_rate / rate) samples: buckets and the curve's own
    length are out_length(n) // hop_size frames.
    level: None, or the half width of dynamics.track_level (an integer in [0, 8]): each bucket's loudness contour is then tracked from the same device tensor
    the pitch is (after the rate conversion), fitted exactly as the f0 curve is and stored as the item's "level" -- fp32 mean-square power per
    frame, 0 = no level.  An item that brings its own "level" keeps it.
    track["path"]: None, or a dict of pitch_track.PATH_DEFAULTS keys (possibly empty): the curve is then the cheapest path through every frame's lag candidates
    (extract_f0(path=)) instead of a decision per frame -- no octave jumps on a weak fundamental, no flicker of the voicing; a recording may
    then have at most 32768 frames (ValueError naming the item).
    As synthesize's first pre-pass (guide_track: a dict of these keywords), on copies of the items: tempo and "ph_stretch" warp a tracked curve as they warp a given
    one; fit=False under guide_align, level = guide_dynamics' half_width.  "guide_wav" without guide_track: ValueError; no "guide_wav": guide_track is not looked at.
    ValueError: no sample_rate, an unknown keyword, a rate that is no integer >= 1 or that the converter's table budget does not admit, an item with both "f0" and "guide_wav", a
    recording that is not 1-D or shorter than a hop (after conversion)."""
    track = _option("guide_track", track, hop_size)
    sr, rec_rate = track["sample_rate"], track.pop("recording_rate", None)
    if level is not None:
        level = dynamics.check_args(half_width=level)[0]
    wavs, rates = {}, {}
    for i, it in enumerate(items):
        if it.get("guide_wav") is None:
            continue
        if it.get("f0") is not None:
            raise ValueError(f"item {i} carries both a guide curve ('f0') and a recording ('guide_wav'): give one of them")
        rates[i] = sr if it.get("guide_sr", rec_rate) is None else it.get("guide_sr", rec_rate)
        try:
            resample.design(rates[i], sr)
        except ValueError as e:
            raise ValueError(f"item {i}: guide_sr: {e}") from None
        w = np.asarray(it["guide_wav"])
        if w.ndim != 1 or not np.issubdtype(w.dtype, np.floating) or resample.out_length(len(w), rates[i], sr) < hop_size:
            raise ValueError(f"item {i}: guide_wav must be a 1-D float array of at least hop_size = {hop_size} samples at {sr} Hz, got {w.dtype} {w.shape}")
        wavs[i] = w.astype(np.float32, copy=False)
    out = [dict(it) for it in items]
    samples = {i: resample.out_length(len(w), rates[i], sr) for i, w in wavs.items()}          # at the model's rate
    if track.get("path") is not None:
        for i, n in samples.items():
            if n // hop_size > pitch_track.PATH_FRAMES_LIMIT:
                raise ValueError(f"item {i}: guide_wav has {n // hop_size} frames; path tracking takes at most {pitch_track.PATH_FRAMES_LIMIT} (split the recording)")
    buckets = [idx for r in sorted(set(rates.values()))               # (recordings of one rate share a bucket)
               for idx in _buckets({i: n // hop_size for i, n in samples.items() if rates[i] == r}, max_frames_per_batch)]
    for idx in buckets:
        rate = rates[idx[0]]
        wav = _pad_rows([wavs[i] for i in idx], torch.float32).to(device)
        lens = torch.tensor([len(wavs[i]) for i in idx], dtype=torch.int64).to(device)
        if rate != sr:
            wav, lens = resample.resample(wav, rate, sr, lengths=lens, return_lengths=True)
        f0 = pitch_track.extract_f0(wav, hop_size, lengths=lens, **track).cpu().numpy()
        lvl = None if level is None else dynamics.track_level(wav, hop_size, lengths=lens, half_width=level).cpu().numpy()
        for b, i in enumerate(idx):
            out[i].pop("guide_sr", None)
            own = samples[i] // hop_size
            T, have = (len(items[i]["mel2ph"]), min(own, len(items[i]["mel2ph"]))) if fit else (own, own)
            curve = np.zeros(T, np.float32)
            curve[:have] = f0[b, :have]
            del out[i]["guide_wav"]
            out[i]["f0"] = curve
            if lvl is not None and out[i].get("level") is None:
                out[i]["level"] = np.zeros(T, np.float32)
                out[i]["level"][:have] = lvl[b, :have]
    return out


def _token_pitches(items, table, curve_of):
    """({i: note_midi}, {i: curve}, {i: the item's own "guide_offset_cents" or None}) of the items that carry a guide curve "f0" and token pitches: "note_midi",
    or "pitch_tokens" through `table` (midi_of_token).  curve_of(i, item, n_tok) returns the item's checked curve.  A ValueError names the item."""
    table = None if table is None else np.asarray(table, dtype=np.float32)
    if table is not None and table.ndim != 1:
        raise ValueError(f"midi_of_token must be a 1-D sequence of MIDI numbers indexed by pitch token, got shape {table.shape}")
    notes, curves, offsets = {}, {}, {}
    for i, it in enumerate(items):
        if it.get("f0") is None or (it.get("note_midi") is None and table is None):
            continue
        n_tok = len(it["text_tokens"])
        if it.get("note_midi") is not None:
            nm = np.asarray(it["note_midi"], dtype=np.float32)
            if nm.shape != (n_tok,):
                raise ValueError(f"item {i}: note_midi has shape {nm.shape} for {n_tok} tokens (one MIDI number per token)")
        else:
            pt = np.asarray(it["pitch_tokens"]).astype(np.int64)
            if pt.shape != (n_tok,) or (pt < 0).any() or (pt >= len(table)).any():
                raise ValueError(f"item {i}: pitch_tokens must be {n_tok} ids in [0, {len(table)}) to go through midi_of_token")
            nm = table[pt]
        notes[i], curves[i], offsets[i] = nm, curve_of(i, it, n_tok), it.get("guide_offset_cents")
        if offsets[i] is not None and not (isinstance(offsets[i], (int, float)) and abs(offsets[i]) < float("inf")):
            raise ValueError(f"item {i}: guide_offset_cents must be a finite number, got {offsets[i]!r}")
    return notes, curves, offsets


def align_items(items, device, max_frames_per_batch=32768, **guide_align):
    """Copies of `items` in which an item that carries a guide curve "f0" -- any length >= 1, on the guide's own timeline -- and token pitches is timed to
    that curve (guide_align.align_guide): its "mel2ph" is replaced by timing.retime(dur=dur_new) -- exact, no stretch, no tempo -- so it has
    len(f0) frames and the curve is a guide on it as it is; "f0" is kept.  Token pitches: the item's "note_midi", one MIDI number per token (<= 0 or not finite
    = a rest), or its "pitch_tokens" mapped through guide_align["midi_of_token"] (a sequence indexed by token id).  Items without a curve or without token
    pitches are passed on as they are.  The other keywords are align_guide's: offset_cents (one number for the call; an item's "guide_offset_cents" goes
    before it), octave_fold and the weights.  Computed on the device in buckets of guide length and read back.
    As synthesize's alignment pre-pass (guide_align: a dict of these keywords, possibly empty; None: nothing changes): a recording's curve keeps its own
    len(guide_wav) // hop_size frames (guide_items(fit=False)), so the item is sung with the recording's timing and pitch.  It runs behind the guide pre-pass and
    before the tempo pre-pass, which acts on the aligned item; "dur_tokens" stay the caller's; a "level" curve is left alone (it is on "f0"'s timeline).
    ValueError: an unknown keyword, a curve that is not 1-D or longer than 65536 frames, an item of more than 1024 tokens, "note_midi" of another length than
    the tokens, a pitch token outside midi_of_token, and an item that cannot be aligned (status 1: no token with frames, or fewer guide frames than such
    tokens) -- named by its index."""
    guide_align = _option("guide_align", guide_align)
    table, offset = guide_align.pop("midi_of_token", None), guide_align.pop("offset_cents", 0.0)
    def curve_of(i, it, n_tok):
        f0 = np.asarray(it["f0"], dtype=np.float32)
        if f0.ndim != 1 or not 1 <= len(f0) <= guide_align_ops.TG_LIMIT or not 1 <= n_tok <= guide_align_ops.T_PH_LIMIT:
            raise ValueError(f"item {i}: a guide curve of 1 .. {guide_align_ops.TG_LIMIT} frames (1-D) and 1 .. {guide_align_ops.T_PH_LIMIT} tokens can be aligned, "
                             f"got {f0.shape} and {n_tok}")
        return f0

    notes, curves, offsets = _token_pitches(items, table, curve_of)
    out = [dict(it) for it in items]
    for idx in _buckets({i: len(f0) for i, f0 in curves.items()}, max_frames_per_batch):
        f0, nm = _pad_rows([curves[i] for i in idx], torch.float32), _pad_rows([notes[i] for i in idx], torch.float32)
        m2p = _pad_rows([items[i]["mel2ph"] for i in idx], torch.long, max(1, max(len(items[i]["mel2ph"]) for i in idx)))
        cents = [float(offset if offsets[i] is None else offsets[i]) for i in idx]
        dur_new, _, status = guide_align_ops.align_guide(f0.to(device), nm.to(device), mel2ph=m2p.to(device), guide_lengths=[len(curves[i]) for i in idx],
                                                         offset_cents=cents, **guide_align)
        status = status.cpu().tolist()
        if any(status):
            b = status.index(1)
            raise ValueError(f"item {idx[b]} cannot be aligned: a guide of {len(curves[idx[b]])} frames for a score whose alignment gives "
                             f"{len(set(np.asarray(items[idx[b]]['mel2ph']).tolist()) - {0})} tokens frames (at least one frame per such token is needed)")
        new, lens, _ = timing.retime(dur=dur_new)
        new, lens = new.cpu().numpy(), lens.cpu().tolist()
        for b, i in enumerate(idx):
            out[i]["mel2ph"] = new[b, :lens[b]].copy()
    return out


def correct_items(items, device, max_frames_per_batch=32768, **guide_correct):
    """Copies of `items` in which the guide curve "f0" of an item that carries one -- one value per frame of its mel2ph -- and token pitches is pulled onto the
    score (guide_correct.correct_guide): the slow part of its deviation from each note is taken out, vibrato and scoops stay.  Token pitches:
    the item's "note_midi", one MIDI number per token (<= 0 or not finite = a rest), or its "pitch_tokens" mapped through guide_correct["midi_of_token"] (a
    sequence indexed by token id), as in align_items.  Items without a curve or without token pitches are passed on as they are.  The other keywords are
    correct_guide's: window, strength, vibrato, wild_cents, octave_fold, and offset_cents -- one number for the call, or "auto" (each item in the key it was
    sung in); an item's "guide_offset_cents" goes before it.  Computed on the device in buckets of length and read back.
    As synthesize's correction pre-pass (guide_correct: a dict of these keywords, possibly empty; None: nothing changes), on curves given or tracked: it runs behind
    the alignment pre-pass (an aligned item has one value per frame) and before the tempo pre-pass, which warps the corrected curve.  The caller's items are not modified.
    ValueError: an unknown keyword, a value out of range, a curve that is not 1-D with len(mel2ph) values, an item of more than 65536 frames or 1024 tokens,
    "note_midi" of another length than the tokens, a pitch token outside midi_of_token -- named by the item's index."""
    guide_correct = _option("guide_correct", guide_correct)
    table, offset = guide_correct.pop("midi_of_token", None), guide_correct.pop("offset_cents", 0.0)
    auto = isinstance(offset, str)
    def curve_of(i, it, n_tok):
        _check_curve(i, it, "f0")
        f0, n_frames = np.asarray(it["f0"], dtype=np.float32), len(it["mel2ph"])
        if not 1 <= n_frames <= guide_correct_ops.T_LIMIT or not 1 <= n_tok <= guide_correct_ops.T_PH_LIMIT:
            raise ValueError(f"item {i}: a guide curve of 1 .. {guide_correct_ops.T_LIMIT} frames and 1 .. {guide_correct_ops.T_PH_LIMIT} tokens can be "
                             f"corrected, got {n_frames} and {n_tok}")
        return f0

    notes, curves, offsets = _token_pitches(items, table, curve_of)
    out = [dict(it) for it in items]
    for idx in _buckets({i: len(f0) for i, f0 in curves.items()}, max_frames_per_batch):
        f0, nm = _pad_rows([curves[i] for i in idx], torch.float32).to(device), _pad_rows([notes[i] for i in idx], torch.float32).to(device)
        m2p = _pad_rows([items[i]["mel2ph"] for i in idx], torch.long).to(device)
        lens = [len(curves[i]) for i in idx]
        own = [offsets[i] for i in idx]
        cents = torch.tensor([float(0.0 if auto else offset) if v is None else float(v) for v in own], dtype=torch.float32).to(device)
        if auto and any(v is None for v in own):                         # the key of every item that does not bring its own, never read back
            med, _ = guide_correct_ops.guide_deviation(f0, m2p, nm, lengths=lens, wild_cents=guide_correct.get("wild_cents", 300.0),
                                                       octave_fold=guide_correct.get("octave_fold", False))
            cents = torch.where(torch.tensor([v is None for v in own]).to(device), med.float() / 16, cents)
        new = guide_correct_ops.correct_guide(f0, m2p, nm, lengths=lens, offset_cents=cents, **guide_correct).cpu().numpy()
        for b, i in enumerate(idx):
            out[i]["f0"] = new[b, :len(curves[i])].copy()
    return out


def retime_items(items, tempo, device, max_frames_per_batch=32768):
    """Copies of `items` with "mel2ph" (and "f0" and "level", when present) retimed by the item's "ph_stretch" / its tempo (timing.retime), computed on the
    device in collated groups and read back; the copies carry no "ph_stretch".  A level curve is warped by a second timing.retime(curve=) call, only in
    groups where an item carries one.  tempo: None, a number, or one number per item, finite and > 0 (ValueError);
    "ph_stretch": one finite factor > 0 per token of the item (ValueError).
    As synthesize's tempo pre-pass, the last one (tempo in input order): mel2ph is retimed by ph_stretch[i] / tempo per token, on copies of the items.  Without
    tempo and without an item that carries "ph_stretch" there is no pre-pass."""
    n = len(items)
    tempos = [1.0] * n if tempo is None else timing.factor_tensor(tempo, n, "cpu").tolist()
    stretches = []
    for i, it in enumerate(items):
        st = it.get("ph_stretch")
        st = np.ones(len(it["text_tokens"]), np.float32) if st is None else np.asarray(st, dtype=np.float32)
        if st.shape != (len(it["text_tokens"]),):
            raise ValueError(f"item {i}: ph_stretch has shape {st.shape} for {len(it['text_tokens'])} tokens (one factor per token)")
        if not (np.isfinite(st).all() and (st > 0).all()):
            raise ValueError(f"item {i}: a stretch factor must be a finite number > 0")
        _check_curve(i, it, "f0")
        _check_curve(i, it, "level")
        stretches.append(st)
    out = [None] * n
    guided = [it.get("f0") is not None for it in items]
    for idx in bucket_by_length([len(it["mel2ph"]) for it in items], max_frames_per_batch, keys=guided):
        T = max(1, max(len(items[i]["mel2ph"]) for i in idx))
        m2p, st = _pad_rows([items[i]["mel2ph"] for i in idx], torch.long, T), _pad_rows([stretches[i] for i in idx], torch.float32, fill=1)
        curve = _pad_rows([items[i]["f0"] for i in idx], torch.float32, T) if guided[idx[0]] else None
        new, lens, warped = timing.retime(mel2ph=m2p.to(device), T_ph=st.shape[1], stretch=st.to(device), tempo=[tempos[i] for i in idx],
                                          curve=None if curve is None else curve.to(device))
        levels = None
        if any(items[i].get("level") is not None for i in idx):
            empty = np.zeros(0, np.float32)
            lv = _pad_rows([empty if items[i].get("level") is None else items[i]["level"] for i in idx], torch.float32, T)
            levels = timing.retime(mel2ph=m2p.to(device), T_ph=st.shape[1], stretch=st.to(device), tempo=[tempos[i] for i in idx], curve=lv.to(device))[2].cpu().numpy()
        new, lens = new.cpu().numpy(), lens.cpu().tolist()
        warped = None if warped is None else warped.cpu().numpy()
        for b, i in enumerate(idx):
            out[i] = {k: v for k, v in items[i].items() if k != "ph_stretch"}
            out[i]["mel2ph"] = new[b, :lens[b]].copy()
            if warped is not None:
                out[i]["f0"] = warped[b, :lens[b]].copy()
            if items[i].get("level") is not None:
                out[i]["level"] = levels[b, :lens[b]].copy()
    return out


class PostChain:
    """The device stages behind the generator, in their order -- guide dynamics, rate conversion, loudness normalisation, peak limiter: stages 5 to 8 of 8 in
    synthesize's list -- built once per synthesize call from its checked option dicts.  A stage whose dict is None is not asked for: nothing changes, it makes no tensor and launches nothing.  The stages run on the batch's own
    stream (behind a graph's replay, outside the capture), before the waveforms are copied to the host: rows B * takes, each frames * hop_size samples long.
    Each stage's result equals, bit for bit, its wrapper -- match_dynamics(), resample(), normalize(), limit_peaks(), which say what the keys mean -- applied to the waveform
    the call returns without that option.  ValueError (synthesize): an option that is not a dict, an unknown key, a value out of range.
    guide_dynamics -- a dict of dynamics.DEFAULTS keys, possibly empty -- makes every item with a level curve sing with that curve's dynamics.
    The curve is the item's "level" -- fp32 mean-square power, one value per frame, 0 = no level there -- given or tracked by the guide pre-pass; after the
    pre-passes it must have len(mel2ph) values.  The batch's waveforms are measured the same way and scaled per sample by the smoothed, limited gain; rows of
    items without a level come back bit for bit, and a batch in which no item carries one launches nothing.  ValueError also: hop_size over 2048, a level curve
    of another length than the item's frames, an item with "level" in a call without guide_dynamics.
    resample_to -- a dict with sample_rate (the model's) and output_rate, optionally the converter's quality keywords -- converts the waveforms:
    entry i of the result is then out_length(frames_i * hop_size) samples long (per take); a curve asked back with return_f0 stays per frame.  ValueError also:
    a missing key, a ratio over the converter's table budget.
    loudness -- (the rate it measures at, a dict of loudness.DEFAULTS keys), as _check_loudness returns it -- brings every row, so every take of
    an item on its own, to target_lufs: stage 7 of 8, measured at the output rate on what the converter wrote, with the rows' lengths at that rate.  A row
    shorter than 400 ms or without a block over the gates comes back bit for bit.
    limit -- a dict of limiter.DEFAULTS keys, possibly empty -- holds every waveform under the ceiling: the last step, behind a guide_dynamics
    boost, resample_to's conversion and a loudness gain, which all overshoot, with the rows' lengths at the output rate.  A whole quiet item comes back bit for
    bit.  Where the limiter reduces a normalised waveform, the delivered loudness is slightly below target_lufs: by what the reduction takes."""

    def __init__(self, resample_to, guide_dynamics, limit, hop_size, takes, loudness=None):
        self.dyn, self.lim, self.hop, self.takes, self.loud = guide_dynamics, limit, hop_size, takes, loudness
        self.rates = None if resample_to is None else (resample_to["sample_rate"], resample_to["output_rate"])
        self.quality = None if resample_to is None else {k: v for k, v in resample_to.items() if k in resample.DEFAULTS}

    def out_samples(self, frames):
        """the samples an item of `frames` frames comes back with (per take)"""
        return frames * self.hop if self.rates is None else resample.out_length(frames * self.hop, *self.rates)

    def batch(self, frames, levels, T, device):
        """The bundle (apply, tensors) of a batch T frames wide, of items of `frames` frames with the level curves `levels` (None: none).  tensors: what it has put on
        the device, per take -- the level rows, the rows' lengths at the model's rate (dynamics, converter) and at the output rate (loudness, limiter); apply(wav_dev) runs the stages"""
        rows = lambda per_item: torch.tensor([v for v in per_item for _ in range(self.takes)], dtype=torch.int64).to(device)
        level = samples = samples_out = None
        if self.dyn is not None and any(lv is not None for lv in levels):
            level = _pad_rows([() if lv is None else lv for lv in levels for _ in range(self.takes)], torch.float32, T).to(device)
        if level is not None or self.rates is not None:
            samples = rows(n * self.hop for n in frames)
        if self.lim is not None or self.loud is not None:
            samples_out = rows(self.out_samples(n) for n in frames)
        def apply(wav_dev):
            if level is not None:
                wav_dev = dynamics.match_dynamics(wav_dev.float(), level, self.hop, lengths=samples, **self.dyn)
            if self.rates is not None:
                wav_dev = resample.resample(wav_dev, *self.rates, lengths=samples, **self.quality)
            if self.loud is not None:
                wav_dev = loudness_ops.normalize(wav_dev.float().contiguous(), self.loud[0], lengths=samples_out, **self.loud[1])
            return wav_dev if self.lim is None else limiter.limit_peaks(wav_dev.float().contiguous(), lengths=samples_out, **self.lim)
        return apply, [t for t in (level, samples, samples_out) if t is not None]


@torch.no_grad()
def synthesize(model, items, hop_size, max_frames_per_batch=32768, noise_scale=1.0, generator=None, equal_tokens=False,
               graphs=None, streams=2, seeds=None, takes=1, first_take=0, voicing="guide", pitch_shift_cents=None, return_f0=False,
               tempo=None, guide_track=None, guide_align=None, guide_correct=None, resample_to=None, guide_dynamics=None, limit=None, vibrato=None,
               loudness=None):
    """Run VISinger.forward(infer=True) over length-bucketed batches.  Returns a list of float32 waveforms trimmed to
    each item's own length (frames * hop_size), in the input order.

    Against the item's one-at-a-time synthesis (the reference's test_step, tasks/visinger.py:244-263) on the same noise:
      * the prior, the flow and the attention are masked per item by the reference itself;
      * the HiFi-GAN generator -- which the reference runs unmasked, on one utterance -- is run with the frame mask at every stage
        (Generator.forward x_mask) whenever a batch holds items of different lengths, so nothing leaks from the padding into an
        item's last frames;
      * the reference's TextEncoder views its positional-embedding table by the PADDED token count (encoder.py:52-54, a `seq_len =
        hidden` mix-up restated literally): an item padded to a longer token sequence gets a different embedding than alone.
        `equal_tokens=True` lets only items of equal token count share a batch -- then every waveform EQUALS its one-at-a-time
        synthesis; the default batches by frames only and is exact for the items that define a batch's token length.

    graphs: a dict owned by the caller; when given, each batch shape (B, T_tokens, T_frames, ragged) is captured into a HIP graph
    on first use (GraphedStep) and replayed afterwards -- the launch chain of a small batch (B=1: ~700 dependent launches) then
    costs one graph launch instead of ~700 host-side launches.

    streams: consecutive batches go to alternating HIP streams (StreamRotation: the next batch's transformers run under this batch's generator); a batch's
    waveforms come back to the host when `streams` later batches have been issued.  The result is bit-identical to streams = 1 (same kernels, same inputs: the
    noise of every batch is drawn on the caller's stream, in batch order) -- on a cold model and right after a parameter change too: a batch that meets, on its
    stream, a handle the previous batch is still packing on the other waits for that pack (StreamRotation).  With `graphs` the batches replay on the caller's
    stream (one stream).
    Everything a batch puts on the device -- the collated tensors, noise or seeds, cents, the post chain's tensors -- is kept in one list as it is made, and
    that list is what is recorded on the batch's stream: the caching allocator reuses their memory only behind that stream's work.

    seeds: one integer in [0, 2^63) per item, in input order, or a single integer s (item i gets (s + i) mod 2^63: sampling.item_seeds).  The prior sample of
    item i is then drawn on the device from the item's own counter-based stream (sampling.prior_sample; noise_scale goes to the kernel) instead of the batch-wide
    torch.randn: the waveform depends on (model, item, seed) only -- not on the bucket, the row, the padding or what was synthesised before.
    takes > 1 (seeded path only): `takes` samples per item, take indices first_take .. first_take + takes - 1, from ONE pass of the text encoder, pitch
    predictor and frame prior; entry i of the result is then a float32 array [takes, frames_i * hop_size].  The padded-frame and item budgets count
    decoded rows: buckets are cut with max_frames_per_batch // takes and 256 // takes items.

    Pitch control (VISinger.forward f0_hz / voicing / pitch_shift_cents; needs use_pitch_embed): an item with "f0" -- a curve in Hz, one value per frame of
    its mel2ph, 0 = unvoiced -- is sung on that guide; voicing="guide" takes the voiced frames from it, "model" keeps the predictor's own decision over the
    gap-interpolated guide.  Items with and without a guide never share a batch.  pitch_shift_cents: a number, or one per item in input order; transposes the
    conditioning curve (guide or predicted), read on the device.  return_f0: the result is a list of (wav, f0_hz) with f0_hz the float32 curve the prior was
    conditioned on, in Hz (0 = unvoiced), trimmed to the item's frames.  Items without "f0" in a call without these arguments run exactly as before.

    Vibrato (VISinger.forward vibrato=, visinger_amd/vibrato.py; needs use_pitch_embed): vibrato is None or a dict of vibrato.DEFAULTS keys
    (depth_cents, rate_hz, delay_s, attack_s, release_s, min_note_s: a number, or one per item in input order) plus the required sample_rate, the model's.  The
    curve every item is sung on -- predicted or guided -- then gets a per-note modulation on the device, in front of the transposition; return_f0 shows it.  An
    item may carry "note_of_token" (one note id per token, 0 = a rest; default: vibrato.notes_of_tokens of its pitch tokens) and "vibrato_depth_cents" (one depth
    per token, read at a note's first token; NaN or None = the call's depth_cents).  Checked next to `voicing`, behind the option dicts below.

    The controls, in the order their stages run: four pre-passes on the device, on copies of the items -- the call runs on what they leave, so buckets, `ragged`,
    graphs and trimming see the new lengths and curves -- then four stages behind the generator, on the batch's own stream.  Each option is None (nothing changes, nothing is launched) or a dict, checked through OPTIONS before the model is looked at and before any launch
    (ValueError), in the order resample_to, guide_dynamics, limit, guide_correct, guide_align, guide_track.
      1. guide_track      the pitch (and level) curve of an item's recording "guide_wav" is tracked     -> guide_items
                          (with "path": {...} as a Viterbi path through every frame's lag candidates, pitch_track.extract_f0(path=))
      2. guide_align      the score is timed to the guide curve                                          -> align_items
      3. guide_correct    the guide curve is pulled onto the score                                       -> correct_items
      4. tempo            and an item's "ph_stretch": the alignment is retimed, the curves warped        -> retime_items
      5. guide_dynamics   items with a "level" curve are sung with its dynamics                          -> PostChain, dynamics.match_dynamics
      6. resample_to      the waveforms are converted to output_rate                                     -> PostChain, resample.resample
      7. loudness         every waveform is brought to a target programme loudness in LUFS               -> PostChain, loudness.normalize
      8. limit            the waveforms are held under a ceiling                                         -> PostChain, limiter.limit_peaks
    loudness (visinger_amd/loudness.py) is None or a dict of loudness.DEFAULTS keys (target_lufs, max_gain_db) plus the required sample_rate, the
    model's: mono BS.1770-4 integrated loudness, measured on the device at the rate the waveforms leave at (resample_to's output_rate when given), every take of
    an item on its own.  It is no row of OPTIONS: checked on its own behind that table's refusals, before the model is looked at.  The limiter stays last and
    catches what a boost pushes over the ceiling; its reduction then lowers the delivered loudness slightly below target_lufs."""
    sung = any(it.get("guide_wav") is not None for it in items)                  # (no recording: guide_track is not looked at)
    opts = {}
    for name, given in zip(OPTIONS, (resample_to, guide_dynamics, limit, guide_correct, guide_align, guide_track if sung else None)):
        opts[name] = _option(name, given, hop_size)
        if name == "guide_dynamics" and given is None and any(it.get("level") is not None for it in items):
            raise ValueError("an item carries 'level': give guide_dynamics, a dict of dynamics.DEFAULTS keys (possibly empty)")
    if sung and guide_track is None:
        raise ValueError("an item carries 'guide_wav': give guide_track, a dict of pitch_track.extract_f0 keywords with sample_rate")
    loud = None if loudness is None else _check_loudness(loudness, opts["resample_to"])
    device = next(model.parameters()).device
    if sung:
        level = None if opts["guide_dynamics"] is None else opts["guide_dynamics"].get("half_width", dynamics.DEFAULTS["half_width"])
        items = guide_items(items, hop_size, device, max_frames_per_batch, fit=guide_align is None, level=level, **opts["guide_track"])
    if guide_align is not None:
        items = align_items(items, device, max_frames_per_batch, **opts["guide_align"])
    if guide_correct is not None:
        items = correct_items(items, device, max_frames_per_batch, **opts["guide_correct"])
    if tempo is not None or any(it.get("ph_stretch") is not None for it in items):
        items = retime_items(items, tempo, device, max_frames_per_batch)
    if voicing not in ("guide", "model"):
        raise ValueError(f"voicing must be 'guide' or 'model', got {voicing!r}")
    vib_rows = vib_depths = None
    if vibrato is not None:
        vib_rows, vib_depths = _check_vibrato(vibrato, hop_size, items, model)
    if pitch_shift_cents is not None:
        pitch_shift_cents = pitch.cents_tensor(pitch_shift_cents, len(items), "cpu").tolist()      # (checked here; a batch's values travel with the batch)
    if seeds is not None:
        if generator is not None:
            raise ValueError("seeds and generator are two sources of the same noise: give one of them")
        seeds = sampling.item_seeds(seeds, len(items))
        takes, first_take = sampling.check_takes(takes, first_take)
    elif takes != 1 or first_take != 0:
        raise ValueError("takes / first_take select samples of the seeded streams: give seeds")
    for key in ("f0", "level"):
        for i, it in enumerate(items):
            _check_curve(i, it, key)
    lengths = [int((np.asarray(it["mel2ph"]) > 0).sum()) for it in items]
    out = [None] * len(items)
    guided = [it.get("f0") is not None for it in items]
    keys = [len(it["text_tokens"]) for it in items] if equal_tokens else None
    if any(guided):
        keys = [(g, k) for g, k in zip(guided, keys if keys is not None else [0] * len(items))]
    chain = PostChain(opts["resample_to"], opts["guide_dynamics"], opts["limit"], hop_size, takes, loudness=loud)
    rotation = StreamRotation(streams) if (graphs is None and streams and streams > 1) else None
    pending = []                                 # (item indices, device waveforms, device f0, event) of the batches in flight

    def collect(idx, wav_dev, f0_dev, ev=None):
        if ev is not None:
            ev.synchronize()
        wav = wav_dev.float().cpu().numpy()             # [B * takes, L], item-major
        f0 = f0_dev.float().cpu().numpy() if return_f0 else None      # [B, T]: the prior ran once per item
        for b, i in enumerate(idx):
            n = chain.out_samples(lengths[i])
            out[i] = wav[b, :n].copy() if takes == 1 else wav[b * takes:(b + 1) * takes, :n].copy()
            if return_f0:
                out[i] = (out[i], f0[b, :lengths[i]].copy())

    for idx in bucket_by_length(lengths, max(1, max_frames_per_batch // takes), max_items_per_batch=max(1, 256 // takes), keys=keys):
        batch = collate([items[i] for i in idx], device)
        record = list(batch.values())                # the batch record: every tensor this batch puts on the device, as it is made
        B, T = batch["mel2ph"].shape
        ragged = len({lengths[i] for i in idx}) > 1
        noise = seeds_dev = None
        if seeds is None:
            noise = torch.randn((B, model.hidden_size, T), device=device, generator=generator) * noise_scale
            sample, key_tail = dict(noise=noise), ()
        else:                                        # (the seeds travel with the batch; the kernel reads them on the device)
            seeds_dev = torch.tensor([seeds[i] for i in idx], dtype=torch.int64).to(device)
            sample = dict(seeds=seeds_dev, takes=takes, first_take=first_take, noise_scale=noise_scale)
            key_tail = ("seeded", takes, first_take, float(noise_scale))      # (launch arguments of the sampling kernel: fixed by a capture)
        record.append(noise if seeds is None else seeds_dev)
        # pitch control: a guided batch, a shift, or the curve asked back (a zero shift leaves the curve's bits alone and makes the model report it)
        cents_dev, pitch_kw = None, {}
        if "f0_hz" in batch or pitch_shift_cents is not None or return_f0:
            cents_dev = pitch.cents_tensor([pitch_shift_cents[i] for i in idx] if pitch_shift_cents is not None else 0.0, B, device)
            record.append(cents_dev)
            pitch_kw = dict(f0_hz=batch.get("f0_hz"), voicing=voicing, pitch_shift_cents=cents_dev)
        # vibrato: the six settings of every item, and the notes / per-note depths only where an item of the batch carries its own
        vib_dev = None
        if vib_rows is not None:
            T_ph = batch["text_tokens"].shape[1]
            vib_dev = torch.tensor([vib_rows[i] for i in idx], dtype=torch.int32).to(device)
            if any(items[i].get("note_of_token") is not None for i in idx):
                notes = [items[i]["note_of_token"] if items[i].get("note_of_token") is not None else
                         vibrato_ops.notes_of_tokens(np.asarray(items[i]["pitch_tokens"])).numpy() for i in idx]
                batch["note_of_token"] = _pad_rows(notes, torch.int32, T_ph).to(device)
            if any(i in vib_depths for i in idx):
                batch["note_depth_q"] = _pad_rows([vib_depths.get(i, ()) for i in idx], torch.int32, T_ph, fill=-1).to(device)
            record += [vib_dev] + [batch[k] for k in ("note_of_token", "note_depth_q") if k in batch]
            pitch_kw = dict(pitch_kw, vibrato=vib_dev, note_of_token=batch.get("note_of_token"), note_depth_q=batch.get("note_depth_q"))
        post, post_tensors = chain.batch([lengths[i] for i in idx], [items[i].get("level") for i in idx], T, device)
        record += post_tensors

        if graphs is not None:
            key = (B, batch["text_tokens"].shape[1], T, ragged) + key_tail + ("f0_hz" in batch, voicing, cents_dev is not None)
            if vib_dev is not None:
                key += ("vibrato", "note_of_token" in batch, "note_depth_q" in batch)
            if key not in graphs or graphs[key].weights != GraphedStep.fingerprint(model):      # (re-captured after a weight update)
                graphs[key] = GraphedStep(model, batch, noise, ragged, voicing=voicing, cents=cents_dev, vibrato=vib_dev,
                                          **{k: v for k, v in sample.items() if k != "noise"})

        def run():                                   # (called in this iteration, at once: it sees this batch's variables)
            if graphs is not None:                   # (the post chain runs behind the replay, outside the capture)
                return post(graphs[key](batch, noise, seeds=seeds_dev, cents=cents_dev, vibrato=vib_dev)), graphs[key].f0_hz_out
            ret = model(batch["text_tokens"], batch["pitch_tokens"], batch["dur_tokens"], batch["mel2ph"],
                        spk_id=batch["spk_id"], infer=True, mask_decoder=ragged, **sample, **pitch_kw)
            return post(ret["wav_out"]), ret.get("f0_hz")

        if rotation is None:
            collect(idx, *run())
            continue
        for st in rotation.streams:              # (this batch's inputs were made on the caller's stream)
            st.wait_stream(torch.cuda.current_stream())
        (wav_dev, f0_dev), ev = rotation.run(run)
        for t in record:
            t.record_stream(rotation.streams[(rotation.count - 1) % len(rotation.streams)])      # (their memory is reused only behind that stream's work)
        pending.append((idx, wav_dev, f0_dev, ev))
        if len(pending) > len(rotation.streams):
            collect(*pending.pop(0))
    for job in pending:
        collect(*job)
    if rotation is not None:
        rotation.join()
    return out
