"""Every split-f16 (VS_MATH_SPLIT3, the default arithmetic of the attention core) instance relattn_bf16_kernel<2 | 3 | 4, 32, 3>, and relattn_combine_kernel
behind a key split, element by element against the plane-exact reference of tests/attn_split3_reference.py:
|got - ref| <= F_OUT3 * 2^-24 * So + extra on EVERY element -- the reference holds the device's own f16 planes of q / sqrt(dk), k, v and p under the
device's own power-of-two scales (per query, per 32-key K tile, running per V tile, 2^14 for p) and streams over the device's key tiles and key ranges, so
only the order of the fp32 sums and the derived allowance for the exponentials' arguments are left.  Neither F comes from a device: both are the error of
the reference's own serial fp32 restatement, measured on the CPU (tests/test_attn_split3_reference_cpu.py, which also shows which seeded defects the bound
flags and which it does not).  The other tests of these kernels (tests/test_conv_split_gpu.py) are max |err| <= 2e-5 on data that does not move the scales,
one shape with moving scales relative to the head's largest output, and kernel against kernel for the key split.
Each case names the instance it must reach (vs_last_kernel_name) and has the ragged mask of inputs(): item 0 whole (the plain and, near the diagonal, the
plain near-diagonal score loop), item 1 cut at ~2/3 off every tile edge (the masked loop), a third item (B = 3) all padding on every third case.  Every
check prints `ATTN3REF <instance> <case>: per_S <worst |err| / (2^-24 So)> of_bound <worst |err| / bound>`; the key-split cases also read the partial
buffer (ops.rel_attention(work=)): row maxima and in-window scores within F_SCORE3 * 2^-24 * S, l_k and the rows O_k within their bounds relative to
the range.  VS_MATH_SPLIT6 runs a short table on the same three tile shapes against the unsplit fp32 operands (its planes are exact), the three dropped
cross products added to both F; the shapes the split kernels refuse (T % 4 != 0, dk > 128) name the kernel that takes them and hold it to 2e-5."""
import numpy as np
import pytest
import torch

import attn_split3_reference as R
from visinger_amd import _lib as L

pytestmark = pytest.mark.gpu

WORST = {}                      # instance -> the largest per_S printed so far


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def inst_of(dk, terms=3):
    return "relattn_bf16_kernel<%d, 32, %d>" % (R.DT_OF[dk], terms)


def attn_case(vs_option, inp, nh, ws, expect, case, *, ksplit=1, math=L.MATH_SPLIT3):
    """one launch against the reference built for the launch's key ranges"""
    from visinger_amd.ops import rel_attention
    qkv, rel_k, rel_v, mask = inp
    B, C3, T = qkv.shape
    dk = C3 // 3 // nh
    nrel = 0 if ws is None else 2 * ws + 1
    work = None
    if ksplit > 1:
        vs_option("VS_ATTN_KSPLIT", ksplit)
        work = torch.zeros((B * nh * ksplit * (dk + 2 + nrel) * T,), device="cuda", dtype=torch.float32)
    got = rel_attention(dev(qkv), nh, dev(rel_k), dev(rel_v), dev(mask), ws, math=math, ksplit_auto=ksplit > 1, work=work)
    torch.cuda.synchronize()
    inst = L.lib().vs_last_kernel_name().decode()
    assert inst == expect, (inst, expect)
    six = math == L.MATH_SPLIT6
    Fs, Fo = R.F_SCORE3 + (R.DROP6 if six else 0.0), R.F_OUT3 + (R.DROP6 if six else 0.0)
    ref, So, extra, parts = R.expected(qkv, nh, rel_k, rel_v, mask, ws, ksplit=ksplit, F=Fs, exact=six)
    what = f"{inst} {case}"
    if ksplit > 1:
        R.check_partials(R.partials(work, B, nh, dk, T, nrel, ksplit), parts, what=what, F=Fs, F_out=Fo)
    per_s, _ = R.check(got, ref, So, extra, what=what, F=Fo)
    WORST[inst] = max(WORST.get(inst, 0.0), per_s)
    print(f"ATTN3REF largest per_S so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.mark.parametrize("dk,nh,T,ws,share,B", R.SHAPE_CASES)
def test_split_f16_attention(vs_option, dk, nh, T, ws, share, B):
    attn_case(vs_option, R.inputs(B, nh, dk, T, ws, share), nh, ws, inst_of(dk), f"dk{dk} nh{nh} T{T} ws{ws} {'shared' if share else 'per-head'} B{B}")


def test_split_f16_attention_with_the_models_table_scale(vs_option):
    dk, nh, T, ws, share, B = R.MODEL_TABLE_CASE
    attn_case(vs_option, R.inputs(B, nh, dk, T, ws, share, unit=False), nh, ws, inst_of(dk), f"dk{dk} nh{nh} T{T} ws{ws} dk^-0.5 tables")


@pytest.mark.parametrize("kind,dk,T,B", R.MOVING_CASES)
def test_split_f16_attention_with_moving_scales(vs_option, kind, dk, T, B):
    """the element-wise bound where every scale moves: the six cases of test_split_f16_attention_scales_follow_the_data, tiles of zeros (the exponent floor), a
    zero query, the largest channel in alternating lane halves, masked keys that set their tile's exponents, an ev jump that flushes the accumulators"""
    attn_case(vs_option, R.moving_inputs(kind, dk, T, B=B), 1, 4, inst_of(dk), f"{kind} dk{dk} T{T} B{B}")


@pytest.mark.parametrize("dk,T,ws,ksplit,kind,B", R.KSPLIT_CASES)
def test_key_split_split_f16_attention_and_its_partials(vs_option, dk, T, ws, ksplit, kind, B):
    """every key range restarts its running V exponent: range counts that do and do not divide the 9 / 17 tiles, on unit data and on data that moves the scales"""
    attn_case(vs_option, R.moving_inputs(kind, dk, T, ws, B=B), 1, ws, inst_of(dk), f"ksplit{ksplit} {kind} dk{dk} T{T} ws{ws} B{B}", ksplit=ksplit)


@pytest.mark.parametrize("dk,nh,T,ws,share,B", R.SPLIT6_CASES)
def test_split_bf16_x6_attention(vs_option, dk, nh, T, ws, share, B):
    attn_case(vs_option, R.inputs(B, nh, dk, T, ws, share), nh, ws, inst_of(dk, 6), f"dk{dk} nh{nh} T{T} ws{ws} B{B}", math=L.MATH_SPLIT6)


@pytest.mark.parametrize("dk,T,ws", [(64, 130, 4), (160, 132, 7)], ids=["T_not_a_multiple_of_4", "dk_above_128"])
def test_shapes_the_split_kernels_refuse_run_the_fp32_kernel(dk, T, ws):
    """attn_bf16_supported() says no to T % 4 != 0 and to dk > 128 in both split arithmetics: VS_MATH_SPLIT3 then runs the exact-fp32 MFMA kernel
    relattn_kernel<DT, 4, WIDE> (csrc/transformer_ops.hip) -- named here, and held to the fp64 restatement of the fp32 operands at the 2e-5 it has in
    tests/test_conv_split_gpu.py"""
    from visinger_amd.ops import rel_attention
    qkv, rel_k, rel_v, mask = R.inputs(2, 1, dk, T, ws, True)
    got = rel_attention(dev(qkv), 1, dev(rel_k), dev(rel_v), dev(mask), ws, math=L.MATH_SPLIT3)
    torch.cuda.synchronize()
    inst = L.lib().vs_last_kernel_name().decode()
    print(f"ATTN3REF fallback dk{dk} T{T}: {inst}")
    assert inst == "relattn_kernel<%d, 4, %s>" % (-(-dk // 32), "true" if dk > 128 else "false"), inst
    ref, So, extra, _ = R.expected(qkv, 1, rel_k, rel_v, mask, ws, exact=True)
    err = np.abs(R.to_np(got) - ref)
    print(f"ATTN3REF {inst} dk{dk} T{T}: per_S {float((err / (R.EPS32 * So)).max()):.3f} max |err| {float(err.max()):.2e}")
    assert float(err.max()) <= 2e-5
