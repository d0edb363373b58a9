"""Every plain-bf16 (VS_MATH_BF16) attention instance, element by element, against the bf16-operand reference of tests/attn_bf16_reference.py:
|got - ref| <= 2e-5 * (1 + |ref|) + extra, the fp32-class bound plus the exactly bounded bf16 midpoint flips of the probabilities -- the reference
rounds q / sqrt(dk), k, v and p where the device rounds them and streams over the device's key tiles and key ranges, so only the order of the fp32 sums
is left.  The other tests of these kernels are rms bounds of 1e-2 against the exact-fp32 kernel (which a key dropped from one tile, or a window slot
taken from its neighbour, passes: tests/test_attn_bf16_reference_cpu.py) or kernel against kernel (which a defect in the shared Q fragments, window
bookkeeping, mask fill, pack order or finishing loop passes).
Each case names the instance it must reach (vs_last_kernel_name) and has a ragged mask: item 0 whole, item 1 cut at ~2/3 off every tile edge, a third
item (B = 3) all padding.  Relative tables of unit variance per element (a wrong slot is then seen on >= 0.98 of the outputs); one case keeps the model's
dk ** -0.5.  The key-split cases also read the partial buffer (ops.rel_attention(work=)): every range's row maxima and in-window scores within
F_SCORE * 2^-24 * S, its row sums l_k within 2e-5 * l_k + the margin of the exponentials' arguments -- only l_k shows a row sum built from the rounded p.
Every check prints `ATTNREF <instance> <case>: scaled <(|err| - extra) / (2e-5 (1 + |ref|))> of_bound <|err| / bound> marked <p near a midpoint>`; the
key-split cases print the score figures F_SCORE is derived from."""
import numpy as np
import pytest
import torch

import attn_bf16_reference as A
from visinger_amd import _lib as L

pytestmark = pytest.mark.gpu

MEASURED = {"score": 0.0}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def attn_case(oracle, vs_option, opts, expect, dk, nh, T, ws, share, B, *, unit=True, ksplit=1):
    """one plain-bf16 launch against the reference built for the instance's key tile and the launch's key ranges"""
    from visinger_amd.ops import rel_attention
    for name, v in opts.items():
        vs_option(name, v)
    qkv, rel_k, rel_v, mask = A.inputs(B, nh, dk, T, ws, share, unit)
    nrel = 0 if ws is None else 2 * ws + 1
    work = None
    if ksplit > 1:
        vs_option("VS_ATTN_KSPLIT", ksplit)
        work = torch.zeros((B * nh * ksplit * (dk + 2 + nrel) * T,), device="cuda", dtype=torch.float32)
    got = rel_attention(dev(qkv), nh, dev(rel_k), dev(rel_v), dev(mask), ws, math=L.MATH_BF16, ksplit_auto=ksplit > 1, work=work)
    torch.cuda.synchronize()
    inst = L.lib().vs_last_kernel_name().decode()
    assert inst == expect, (inst, expect)
    akt = 64 if dk <= 128 else 32
    ref, extra, parts = A.expected(oracle, qkv, nh, rel_k, rel_v, mask, ws, akt=akt, ksplit=ksplit)
    what = f"{inst} dk{dk} nh{nh} T{T} ws{ws} {'shared' if share else 'per-head'} B{B}" + ("" if unit else " dk^-0.5 tables") + (f" ksplit{ksplit}" if ksplit > 1 else "")
    if ksplit > 1:
        fig = A.check_partials(A.partials(work, B, nh, dk, T, nrel, ksplit), parts, what=what)
        MEASURED["score"] = max(MEASURED["score"], fig)
        print(f"ATTNREF measured score figure so far: {MEASURED['score']:.3f} (F_SCORE {A.F_SCORE})")
    A.check(got, ref, extra, parts, what=what)
    # the padded queries of a cut item and an all-padding item see the exact -1e4 everywhere: p = 1 exactly, nothing to flip
    assert not extra[np.broadcast_to((mask == 0)[:, None, :], extra.shape)].any()


def reg(dt):
    return "relattn_bf16_kernel<%d, %d, 1>" % (dt, 64 if dt <= 4 else 32)


def packed(dt):
    return "relattn_bf16_kernel<%d, %d, 1, true>" % (dt, 64 if dt <= 4 else 32)


DT_OF = {32: 2, 48: 2, 64: 2, 80: 3, 96: 3, 128: 4, 136: 6, 160: 6, 192: 6, 224: 8, 256: 8}
WS = [None, 1, 4, 7]

# ---- register-staged tiles (T < 1024), <2, 64, 1> <3, 64, 1> <4, 64, 1> <6, 32, 1> <8, 32, 1>: every dk x T of dk = 32, 48 / 80 / 160 (off the 32-channel
# tile), 128, 256 and T = 4, 36 (under one tile), 132 (one past the 128-query block, ragged last tile), 260; the window rotates so that every dk and every T
# meets None, 1, 4 and 7 (7 at T = 4: wider than the sequence), tables shared or per head, one or two heads, every third case with an all-padding item
REG_CASES = [(dk, 1 if (share and b % 2) else 2, T, WS[(a + b) % 4], share, 3 if (a + b) % 3 == 0 else 2)
             for a, dk in enumerate([32, 48, 80, 128, 160, 256]) for b, T in enumerate([4, 36, 132, 260]) for share in [(b + a // 2) % 2 == 0]]


@pytest.mark.parametrize("dk,nh,T,ws,share,B", REG_CASES)
def test_register_staged_attention(oracle, vs_option, dk, nh, T, ws, share, B):
    attn_case(oracle, vs_option, {}, reg(DT_OF[dk]), dk, nh, T, ws, share, B)


def test_register_staged_attention_with_the_models_table_scale(oracle, vs_option):
    attn_case(oracle, vs_option, {}, reg(8), 256, 2, 260, 4, True, 2, unit=False)


# ---- pre-packed tile images (attn_pack_kv_kernel + relattn_bf16_kernel<.., true>) at T = 1028: the last tile holds 4 keys; wide heads with the DMA kernel off
NO_DMA = {"VS_NO_ATTN_DMA": 1}
PACKED_CASES = [(64, 2, 4, False, 2, {}), (64, 1, None, True, 2, {}), (96, 1, 7, True, 3, {}), (96, 2, 1, False, 2, {}), (128, 1, None, True, 2, {}), (128, 2, 4, True, 2, {}),
                (160, 1, 4, True, 2, NO_DMA), (160, 2, 7, False, 2, NO_DMA), (256, 1, 7, True, 2, NO_DMA), (256, 1, None, True, 3, NO_DMA)]


@pytest.mark.parametrize("dk,nh,ws,share,B,opts", PACKED_CASES, ids=lambda v: ("nodma" if v else "") if isinstance(v, dict) else str(v))
def test_packed_tile_attention(oracle, vs_option, dk, nh, ws, share, B, opts):
    attn_case(oracle, vs_option, opts, packed(DT_OF[dk]), dk, nh, 1028, ws, share, B)


# ---- relattn_dma_kernel<6 | 8, 1 | 2> at T = 1028: dk = 136, 192 (<6, .>), 224, 256 (<8, .>) x ws = None, 4, 7 x one wave / a wave pair per query group; then
# two heads with per-head tables and an all-padding item in both forms, and B * heads = 8, which takes the XCD-aware workgroup numbering (the others: the plain one)
DMA_CASES = [(dk, 1, ws, True, 2, wpq) for dk in (136, 192, 224, 256) for ws in (None, 4, 7) for wpq in (1, 2)] + \
            [(256, 2, 4, False, 3, 2), (192, 2, 7, False, 3, 1), (136, 4, 7, False, 2, 2)]


@pytest.mark.parametrize("dk,nh,ws,share,B,wpq", DMA_CASES)
def test_dma_attention(oracle, vs_option, dk, nh, ws, share, B, wpq):
    attn_case(oracle, vs_option, {"VS_ATTN_DMA_ONE_WAVE": int(wpq == 1)}, "relattn_dma_kernel<%d, %d>" % (DT_OF[dk], wpq), dk, nh, 1028, ws, share, B)


# ---- key split (VS_ATTN_KSPLIT) + relattn_combine_kernel: range counts that do not divide the tile count (5 tiles of 64 at T = 260, 17 / 33 at T = 1028) and
# one that does (9 tiles of 32 in 3 ranges); the wide heads stay on the packed register-staged kernel (the DMA kernel takes no key split)
KSPLIT_CASES = [(256, 1, 260, 4, 3, reg(8)), (96, 2, 260, 7, 3, reg(3)), (48, 2, 260, 1, 3, reg(2)), (96, 1, 1028, 4, 3, packed(3)), (96, 1, 1028, 4, 5, packed(3)),
                (256, 1, 1028, 4, 3, packed(8)), (256, 1, 1028, 7, 5, packed(8)), (160, 1, 1028, 7, 3, packed(6)), (128, 1, 1028, None, 5, packed(4))]


@pytest.mark.parametrize("dk,nh,T,ws,ksplit,expect", KSPLIT_CASES, ids=lambda v: v.split("<")[1].rstrip(">").replace(", ", "_") if isinstance(v, str) else str(v))
def test_key_split_attention_and_its_partials(oracle, vs_option, dk, nh, T, ws, ksplit, expect):
    attn_case(oracle, vs_option, {}, expect, dk, nh, T, ws, nh == 1, 2, ksplit=ksplit)


def test_a_work_buffer_that_is_too_small_is_refused(vs_option):
    from visinger_amd.ops import rel_attention
    vs_option("VS_ATTN_KSPLIT", 3)
    qkv = torch.zeros((1, 3 * 64, 260), device="cuda")
    with pytest.raises(ValueError, match="work must be"):
        rel_attention(qkv, 1, math=L.MATH_BF16, work=torch.zeros((3 * 66 * 260 - 1,), device="cuda"))


