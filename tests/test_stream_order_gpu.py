"""Cross-stream ordering of a conv handle's packed state.

synthesize(streams=2) sends consecutive batches to alternating HIP streams, and every handle folds and packs its weights lazily, on whichever
stream meets it first.  The host-side keys (ConvOp._wkey, the handle's arithmetic, its F(2,3) flag) change at once; the planes change when the
pack kernels run.  These tests make that gap wide and fixed instead of a matter of launch timing: the PRODUCER's stream is blocked by a bounded
delay (a calibrated torch.cuda._sleep, ~80 ms), the producing call is enqueued behind it, and the consumer is enqueued at once on a second stream
that has nothing else to wait for.  Without ordering inside the library the consumer then runs while the producer has not started, and the outcome
is fixed and wrong.  Every test asserts, right after the host has enqueued the consumer, that the delay is still running: if it is not, the test
fails as INCONCLUSIVE instead of passing by luck.  Every comparison is torch.equal against the same calls made on ONE stream on a second,
identically built handle or module -- the path the element-wise oracle tests hold.  All reads stay inside buffers the handle owns.

What the library without the ordering (the commit before this file) produced is written at each scenario."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from visinger_amd import _lib as L

pytestmark = pytest.mark.gpu

DELAY_MS = 80.0
C, K, T, B = 32, 3, 256, 2            # the smallest conv that reaches every arithmetic's matrix kernels: one 32-row tile, two 16-channel chunks


class Delay:
    """bounded device work that keeps a stream busy for about DELAY_MS: torch.cuda._sleep, timed once with events"""
    cycles = None

    @classmethod
    def calibrate(cls):
        if cls.cycles is None:
            torch.cuda._sleep(100000)                      # (first launch: code object load)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            probe = 2000000
            e0.record()
            torch.cuda._sleep(probe)
            e1.record()
            torch.cuda.synchronize()
            ms = max(e0.elapsed_time(e1), 1e-3)
            cls.cycles = int(min(probe * DELAY_MS / ms, 4e10))
        return cls.cycles

    @classmethod
    def block(cls, stream, times=1):
        """`stream` is busy for times * DELAY_MS from now on.  -> the event recorded behind the delay"""
        with torch.cuda.stream(stream):
            for _ in range(times):
                torch.cuda._sleep(cls.calibrate())
            done = torch.cuda.Event()
            done.record(stream)
        return done


def conclusive(done):
    """the consumer was enqueued while the producer's stream was still blocked: the ordering, not the timing, decides what the consumer reads"""
    assert not done.query(), ("inconclusive: the delay on the producer's stream had finished before the host had enqueued the consumer "
                              "(a host synchronisation inside an entry point, or a stalled host)")


@pytest.fixture(scope="module")
def ab():
    """two streams that run concurrently (torch's pool streams share a few hardware queues: a pair on one queue would be ordered by the hardware and
    could not show a missing dependency)"""
    Delay.calibrate()
    pool = [torch.cuda.Stream() for _ in range(4)]
    probe = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    for a, b in ((pool[0], pool[1]), (pool[1], pool[2]), (pool[2], pool[3])):
        done = Delay.block(a)
        with torch.cuda.stream(b):
            probe.add_(1.0)
        b.synchronize()
        free = not done.query()
        torch.cuda.synchronize()
        if free:
            return a, b
    pytest.fail("inconclusive: no pair of streams ran concurrently (work on one stream waited for a delay on the other)")


def tensors(seed, *shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).cuda() for s in shapes]


@pytest.fixture(scope="module")
def data():
    w0, w1, b, x, gy = tensors(41, (C, C, K), (C, C, K), (C,), (B, C, T), (B, C, T))
    scale = 1.0 / np.sqrt(C * K)
    w0, w1 = w0 * scale, w1 * (1.5 * scale)
    torch.cuda.synchronize()
    return dict(w0=w0, w1=w1, b=b, x=x, gy=gy)


def conv(math, flags=0):
    from visinger_amd.ops import ConvOp
    return ConvOp(L.CONV1D, C, C, K, 1, (K - 1) // 2, flags).set_math(math)


_ONE_STREAM = {}


def one_stream(math, d):
    """(result for w0, result for w1) of the test conv in `math`: one handle, one stream.  Computed once and shared; the handle is kept, so that the
    allocation of a later fresh handle is not this one's freed buffers with w1's planes still in them."""
    if math in _ONE_STREAM:
        return _ONE_STREAM[math][1:]
    op = conv(math)
    op.set_weights(d["w0"], None, d["b"])
    y0 = op.forward(d["x"])
    op.set_weights(d["w1"], None, d["b"])
    y1 = op.forward(d["x"])
    torch.cuda.synchronize()
    assert not torch.equal(y0, y1)
    _ONE_STREAM[math] = (op, y0, y1)
    return y0, y1


def which(y, **named):
    """for a failure message: which of the named results `y` is"""
    hit = [k for k, v in named.items() if v.shape == y.shape and torch.equal(y, v)]
    return f"got {'the result for ' + ' / '.join(hit) if hit else 'neither of ' + ', '.join(named)}"


MATHS = [L.MATH_SPLIT3, L.MATH_BF16, L.MATH_SPLIT6, L.MATH_F32]
MATH_IDS = ["split3", "bf16", "split6", "f32"]


# ---- (a) re-pack, read after write

@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
def test_repack_on_one_stream_is_seen_by_a_forward_on_another(math, ab, data, vs_option):
    """A: delay, set_weights(w1).  B at once: forward(x).  The forward was issued after the re-pack: it computes with w1.
    Without the ordering it returned the result for w0 in all four arithmetics (the old planes, read before the pack kernels ran)."""
    vs_option("VS_NO_WINO", 1)
    sa, sb = ab
    y0, y1 = one_stream(math, data)
    op = conv(math)
    op.set_weights(data["w0"], None, data["b"])
    assert torch.equal(op.forward(data["x"]), y0)
    torch.cuda.synchronize()
    done = Delay.block(sa)
    with torch.cuda.stream(sa):
        op.set_weights(data["w1"], None, data["b"])
    with torch.cuda.stream(sb):
        y = op.forward(data["x"])
    conclusive(done)
    torch.cuda.synchronize()
    assert torch.equal(y, y1), which(y, w0=y0, w1=y1)


# ---- (b) first pack, read after write

@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
def test_first_pack_on_one_stream_is_seen_by_a_forward_on_another(math, ab, data, vs_option):
    """As (a) on a fresh handle: the forward on B would read planes no kernel has written yet (inside the handle's own buffers: wrong numbers, no fault).
    Without the ordering: neither result in all four arithmetics (whatever the fresh allocation held)."""
    vs_option("VS_NO_WINO", 1)
    sa, sb = ab
    y0, y1 = one_stream(math, data)
    op = conv(math)
    torch.cuda.synchronize()
    done = Delay.block(sa)
    with torch.cuda.stream(sa):
        op.set_weights(data["w1"], None, data["b"])
    with torch.cuda.stream(sb):
        y = op.forward(data["x"])
    conclusive(done)
    torch.cuda.synchronize()
    assert torch.equal(y, y1), which(y, w0=y0, w1=y1)


# ---- (c) write after read

@pytest.mark.parametrize("math", [L.MATH_SPLIT3, L.MATH_BF16], ids=["split3", "bf16"])
def test_repack_waits_for_a_forward_issued_before_it_on_another_stream(math, ab, data):
    """B: delay, forward(x).  A at once: set_weights(w1).  The forward was issued first: it computes with w0, and the next one with w1.
    Without the ordering the forward returned the result for w1 (the re-pack overtook it)."""
    sa, sb = ab
    y0, y1 = one_stream(math, data)
    op = conv(math)
    op.set_weights(data["w0"], None, data["b"])
    op.forward(data["x"])
    torch.cuda.synchronize()
    done = Delay.block(sb)
    with torch.cuda.stream(sb):
        y = op.forward(data["x"])
    with torch.cuda.stream(sa):
        op.set_weights(data["w1"], None, data["b"])
    conclusive(done)
    torch.cuda.synchronize()
    assert torch.equal(y, y0), which(y, w0=y0, w1=y1)
    assert torch.equal(op.forward(data["x"]), y1)


# ---- (d) arithmetic switch: the dispatch decision is host-side and immediate, the planes it reads are not

def math_switch_reference(d):
    """split-f16, then the set_math re-pack to plain bf16, then back: one handle, one stream"""
    op = conv(L.MATH_SPLIT3)
    op.set_weights(d["w0"], None, d["b"])
    y3 = op.forward(d["x"])
    y1 = op.set_math(L.MATH_BF16).forward(d["x"])
    y3b = op.set_math(L.MATH_SPLIT3).forward(d["x"])
    torch.cuda.synchronize()
    assert torch.equal(y3, y3b) and not torch.equal(y3, y1)
    return y3, y1


def test_set_math_on_one_stream_is_seen_by_a_forward_on_another(ab, data):
    """(a) with set_math in place of set_weights, SPLIT3 -> BF16 and back: the forward on B is dispatched to the new arithmetic's kernel at once and must
    read the new arithmetic's planes.  Without the ordering: neither result (the bf16 kernel over the split-f16 planes; seen for SPLIT3 -> BF16, where the
    test ends at its first failure)."""
    sa, sb = ab
    y3, y1 = math_switch_reference(data)
    op = conv(L.MATH_SPLIT3)
    op.set_weights(data["w0"], None, data["b"])
    assert torch.equal(op.forward(data["x"]), y3)
    torch.cuda.synchronize()
    for math, want in ((L.MATH_BF16, y1), (L.MATH_SPLIT3, y3)):
        done = Delay.block(sa)
        with torch.cuda.stream(sa):
            op.set_math(math)
        with torch.cuda.stream(sb):
            y = op.forward(data["x"])
        conclusive(done)
        torch.cuda.synchronize()
        assert torch.equal(y, want), f"-> math {math}: " + which(y, split3=y3, bf16=y1)


def test_set_math_waits_for_a_forward_issued_before_it_on_another_stream(ab, data):
    """(c) with set_math: the forward on B was dispatched to the old arithmetic's kernel and must still find the old arithmetic's planes.
    Without the ordering: neither result (the split-f16 kernel over planes already re-packed as bf16; seen for SPLIT3 -> BF16, where the test ends)."""
    sa, sb = ab
    y3, y1 = math_switch_reference(data)
    op = conv(L.MATH_SPLIT3)
    op.set_weights(data["w0"], None, data["b"])
    op.forward(data["x"])
    torch.cuda.synchronize()
    for math, want in ((L.MATH_BF16, y3), (L.MATH_SPLIT3, y1)):
        done = Delay.block(sb)
        with torch.cuda.stream(sb):
            y = op.forward(data["x"])
        with torch.cuda.stream(sa):
            op.set_math(math)
        conclusive(done)
        torch.cuda.synchronize()
        assert torch.equal(y, want), f"forward before -> math {math}: " + which(y, split3=y3, bf16=y1)


# ---- (e) the F(2,3) fragments of the fp32 engine are built inside the first launch that uses them

def test_winograd_fragments_built_by_a_launch_on_one_stream_are_seen_on_another(ab):
    """(2, 128, 128, 1024, 3, 1) of test_conv_gpu.WINO_CASES cut to T = 512.  Freshly packed; the first forward -- which transforms the weights -- on A
    behind the delay, the second on B at once.  Both equal the one-stream output.
    Without the ordering the second forward returned neither (fragments not yet written)."""
    from visinger_amd.ops import ConvOp
    sa, sb = ab
    Bw, Cw, Tw, k = 2, 128, 512, 3
    w, bias, x = tensors(43, (Cw, Cw, k), (Cw,), (Bw, Cw, Tw))
    w = w / np.sqrt(Cw * k)
    ops = [ConvOp(L.CONV1D, Cw, Cw, k, 1, 1).set_math(L.MATH_F32) for _ in range(2)]
    for op in ops:
        op.set_weights(w, None, bias)
    ref = ops[1].forward(x)
    assert ops[1].kernel_instance().startswith("conv_wino_kernel"), ops[1].kernel_instance()
    torch.cuda.synchronize()
    done = Delay.block(sa)
    with torch.cuda.stream(sa):
        ya = ops[0].forward(x)
    with torch.cuda.stream(sb):
        yb = ops[0].forward(x)
    conclusive(done)
    torch.cuda.synchronize()
    assert ops[0].kernel_instance().startswith("conv_wino_kernel"), ops[0].kernel_instance()
    assert torch.equal(ya, ref), "the launch that built the fragments"
    assert torch.equal(yb, ref), "the launch on the other stream"


# ---- (f) fused launches that read several handles

@pytest.mark.parametrize("math,dtype,kernel", [(L.MATH_SPLIT3, torch.float32, "resblock_f16_kernel"), (L.MATH_BF16, torch.bfloat16, "resblock_bf16_kernel"),
                                               (L.MATH_SPLIT6, torch.float32, "respair_split_kernel")], ids=["split3", "bf16-resident", "split6-pairs"])
def test_fused_resblock_launch_sees_a_repack_of_one_of_its_handles(math, dtype, kernel, ab):
    """ResBlock1(32, 3, (1, 3, 5))._run_fused: one launch over its 6 handles (ops.resblock_forward), or one per pair (ops.respair_forward) in the
    split-bf16 arithmetic.  One conv's parameters change; its handle is re-packed on A behind the delay; the fused launch goes to B at once.
    Without the ordering: the output for the old parameters."""
    from visinger_amd.modules.hipconv import set_conv_math
    from visinger_amd.modules.visinger.decoder import ResBlock1
    sa, sb = ab
    torch.manual_seed(47)
    # (two modules built alike, the second given the first's state below: a weight-normed module has no deepcopy)
    blocks = [set_conv_math(ResBlock1(C, 3, (1, 3, 5)), math).cuda().eval() for _ in range(2)]
    with torch.no_grad():
        for p in blocks[0].parameters():
            p.mul_(3.0)                                  # (N(0, 0.01) initialisation: make the convs count beside the residual)
        blocks[1].load_state_dict(blocks[0].state_dict())
        x = tensors(48, (B, C, T))[0].to(dtype)

        def run(m):
            return m._run_fused(x, torch.empty_like(x))

        old = [run(m) for m in blocks]
        assert torch.equal(old[0], old[1])
        assert blocks[0].convs1[0]._op().kernel_instance().startswith(kernel), blocks[0].convs1[0]._op().kernel_instance()
        for m in blocks:
            m.convs2[1].weight_g.mul_(1.75)
        ref = run(blocks[1])
        torch.cuda.synchronize()
        assert not torch.equal(ref, old[1])
        done = Delay.block(sa)
        with torch.cuda.stream(sa):
            blocks[0].convs2[1]._op()                    # (binds the changed parameters: fold + pack)
        with torch.cuda.stream(sb):
            y = run(blocks[0])
        conclusive(done)
        torch.cuda.synchronize()
    assert torch.equal(y, ref), which(y, old=old[1], new=ref)


# ---- (g) the paired and the batched pack

def test_paired_pack_orders_the_grad_input_handle_too(ab, data):
    """bind(..., adjoint=) packs a conv and its VS_CONV_ADJOINT handle in one pair of launches (vs_conv_set_weights_pair) and both carry the key at once;
    the grad-input handle is then read on another stream.  Without the ordering: the grad-input for w0."""
    from visinger_amd.ops import ConvOp
    sa, sb = ab

    def pair():
        return conv(L.MATH_SPLIT3), ConvOp(L.CONV1D, C, C, K, 1, (K - 1) - (K - 1) // 2, L.CONV_ADJOINT).set_math(L.MATH_SPLIT3)

    ref = []
    op, adj = pair()
    for i, w in enumerate((data["w0"], data["w1"])):
        assert op.bind(("w", i), lambda: (w, None, data["b"]), adjoint=adj)
        ref.append(adj.forward(data["gy"]))
    op, adj = pair()
    op.bind(("w", 0), lambda: (data["w0"], None, data["b"]), adjoint=adj)
    assert torch.equal(adj.forward(data["gy"]), ref[0]) and not torch.equal(ref[0], ref[1])
    torch.cuda.synchronize()
    done = Delay.block(sa)
    with torch.cuda.stream(sa):
        assert op.bind(("w", 1), lambda: (data["w1"], None, data["b"]), adjoint=adj)
    with torch.cuda.stream(sb):
        assert adj.has_weights_of(("w", 1))
        gx = adj.forward(data["gy"])
    conclusive(done)
    torch.cuda.synchronize()
    assert torch.equal(gx, ref[1]), which(gx, w0=ref[0], w1=ref[1])


def test_batched_pack_orders_each_of_its_handles(ab, data):
    """ConvOp.set_weights_batch packs a list of handles in two launches; every one of them is then readable from another stream.
    Without the ordering: the results for w0."""
    from visinger_amd.ops import ConvOp
    sa, sb = ab
    y0, y1 = one_stream(L.MATH_SPLIT3, data)
    ops = [conv(L.MATH_SPLIT3), conv(L.MATH_SPLIT3)]
    ConvOp.set_weights_batch([(op, data["w0"], data["b"], ("w", 0)) for op in ops])
    assert all(torch.equal(op.forward(data["x"]), y0) for op in ops)
    torch.cuda.synchronize()
    done = Delay.block(sa)
    with torch.cuda.stream(sa):
        ConvOp.set_weights_batch([(op, data["w1"], data["b"], ("w", 1)) for op in ops])
    with torch.cuda.stream(sb):
        ys = [op.forward(data["x"]) for op in ops]
    conclusive(done)
    torch.cuda.synchronize()
    for y in ys:
        assert torch.equal(y, y1), which(y, w0=y0, w1=y1)


# ---- (h) the fused q | k | v handle of an attention layer (and every other handle of a cold encoder)

def test_cold_attention_layer_first_used_on_one_stream_is_right_on_another(ab):
    """RelativeEncoder(64, 128, 2, 1, kernel_size=3, window_size=4), T = 40, cold: the first call -- which packs the fused q | k | v projection, conv_o and
    the FFN convs -- on A behind the delay, the second on B at once.  Without the ordering the second call returned other numbers (unwritten planes)."""
    from visinger_amd.modules.rel_transformer import RelativeEncoder
    sa, sb = ab
    torch.manual_seed(53)
    enc = RelativeEncoder(64, 128, 2, 1, kernel_size=3, window_size=4).cuda().eval()
    twin = copy.deepcopy(enc)                          # (a copy's handle tables are empty: its own, cold, handles)
    x = tensors(54, (B, 64, 40))[0]
    mask = torch.ones(B, 1, 40, device="cuda")
    mask[1, :, 33:] = 0
    with torch.no_grad():
        ref = [twin(x, mask), twin(x, mask)]
        torch.cuda.synchronize()
        assert torch.equal(ref[0], ref[1])
        done = Delay.block(sa)
        with torch.cuda.stream(sa):
            ya = enc(x, mask)
        with torch.cuda.stream(sb):
            yb = enc(x, mask)
        conclusive(done)
        torch.cuda.synchronize()
    assert torch.equal(ya, ref[0]), "the call that packed"
    assert torch.equal(yb, ref[1]), "the call on the other stream"


# ---- (i) the whole model, cold, through synthesize(streams=2)

def test_cold_model_two_streams_first_then_one_stream(ab):
    """The tiny model, every key forgotten (hipconv.repack_weights), the caller's stream blocked while the host enqueues: synthesize(streams=2) over several
    batches runs BEFORE any one-stream call, so batch 1 meets on its stream the handles batch 0 is packing on the other.  Then the streams=1 reference on the
    same seeds: equal bit for bit.  Once more after an in-place parameter change and a second repack_weights.  (synthesize returns host arrays, so it ends
    with a synchronisation: this test cannot assert that the delay was still running, and both streams start together behind it -- it holds the ordered
    path; the scenarios above are the ones that detect a missing dependency.)"""
    from visinger_amd import synth
    from visinger_amd.models.visinger import VISinger
    from visinger_amd.modules.hipconv import repack_weights
    w, a = load_golden("visinger_tiny")
    hp = json.load(open(os.path.join(GOLDEN, "visinger_tiny_hparams.json")))
    m = VISinger(13, 9, 7, hp)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m = m.cuda().eval()
    hop = int(np.prod(hp["upsample_rates"]))
    items = []
    for rep in range(3):
        for b in range(2):
            n = int((a["mel2ph"][b] > 0).sum()) - rep
            nph = int((a["text"][b] > 0).sum())
            items.append(dict(text_tokens=a["text"][b][:nph], pitch_tokens=a["pitch"][b][:nph], dur_tokens=a["dur"][b][:nph], mel2ph=a["mel2ph"][b][:n]))
    budget = 2 * max(len(it["mel2ph"]) for it in items)
    assert len(synth.bucket_by_length([len(it["mel2ph"]) for it in items], budget)) >= 2

    def run(streams):
        return synth.synthesize(m, items, hop, max_frames_per_batch=budget, generator=torch.Generator(device="cuda").manual_seed(5), streams=streams)

    for change in (False, True):
        if change:
            with torch.no_grad():
                for p in m.decoder.parameters():
                    p.data.mul_(1.03)                    # (through .data: the keys cannot see it)
        repack_weights(m)
        torch.cuda.synchronize()
        Delay.block(torch.cuda.current_stream(), times=2)
        got = run(2)
        ref = run(1)
        assert len(got) == len(ref) == len(items)
        assert all(np.array_equal(x, y) for x, y in zip(ref, got)), f"after {'the parameter change' if change else 'the cold start'}"
