"""The weight-gradient kernels of the training step (csrc/conv_backward.hip: conv_wgrad_split_kernel<KT, TS>, conv_wgrad_kernel, wgrad_finish_kernel), element by
element, against the fp64 sum of the device's own operand planes (tests/wgrad_reference.py): |got - ref| <= F * 2^-24 * S over ALL elements, S = sum |gy| |x|; an
element with S = 0 exactly 0.  The other tests of these kernels compare with aten on the same GPU under max-norm bounds (3e-6 max|ref| + 2.5 aten's own error;
2e-5 (1 + max|ref|)) that one dropped small cross product passes on most outputs (tests/test_wgrad_reference_cpu.py).  The library reports no kernel name for
these launches: each case asserts that vs_conv_wgrad_planes equals the restated plane count of the kernel it means to reach (the two kernels' counts differ
at every shape but the two of wgrad_reference.COUNTS_COINCIDE) and names the instance the `switch` of wgrad_launch picks from K.
Inputs are randn (one variant per group with per-channel gains 2^-6 .. 2^6 on both operands: the bound is relative to S per element); the references are numpy
matmuls in fp64 (the `oracle` fixture is taken for its cap on the BLAS threads).  Every comparison prints `WGRADREF <kernel by rule> <case>: per_S <|err| / (2^-24 S)> scaled <|err| / (2e-5 (1 + |ref|))>`."""
import numpy as np
import pytest
import torch

import wgrad_reference as R
from visinger_amd import _lib as L

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def reach(vs_option, B, Cout, Cin, Tout, K, split):
    """set the dispatch for the kernel the case means, assert by the plane count that the library agrees; -> the kernel's name by the rule"""
    ok = R.wgrad_split_ok(B, Cout, Tout, K)
    assert ok or not split, "the case means the split kernel at a shape the rule sends to the fp32 one"
    if ok and not split:
        vs_option("VS_NO_WGRAD_SPLIT", 1)
    want = R.split_slices(B, Cout, Cin, Tout) if split else R.f32_planes(B, Cout, Cin, Tout, K)
    other = R.f32_planes(B, Cout, Cin, Tout, K) if split else R.split_slices(B, Cout, Cin, Tout)
    assert L.require_gpu().vs_conv_wgrad_planes(B, Cout, Cin, Tout, K) == want, (B, Cout, Cin, Tout, K, split)
    assert (want != other) or (B, Cout, Cin, Tout, K) in R.COUNTS_COINCIDE or not ok
    return R.kernel_by_rule(B, Cout, Cin, Tout, K, split)


def wgrad_case(vs_option, c, *, impulse=None, bias=False, F=None):
    """one ops.conv_wgrad launch of a table case against the plane reference (split kernel) / the plain fp64 gradient (fp32 kernel)"""
    from visinger_amd.ops import conv_wgrad
    name = reach(vs_option, c.B, c.Cout, c.Cin, c.Tout, c.K, c.split)
    gy, x, pad = R.inputs(c, impulse=impulse)
    got = conv_wgrad(dev(gy), dev(x), c.K, c.dil, pad, bias=bias)
    torch.cuda.synchronize()
    ref, S = R.expected(gy, x, c.K, c.dil, pad, rounded=c.split)
    what = "%s %s%s" % (name, R.case_id(c), "" if impulse is None else " col %r" % (impulse,))
    if F is None:
        F = R.F_WGRAD if c.split else R.F_WGRAD_F32
    if bias:
        got, gb = got
        bref, bS = R.expected_bias(gy)
        R.assert_close(gb, bref, bS, what + " bias", F=R.F_BIAS)
    assert tuple(got.shape) == ref.shape
    R.assert_close(got, ref, S, what, F=F)
    return got, gy, x, pad, ref, S


# ---- A. split kernel, every tap count (every <KT, TS> of the switch), shortest reduction; valid and full padding; per-channel gains
@pytest.mark.parametrize("c", R.A_CASES, ids=R.case_id)
def test_split_kernel_every_tap_count(oracle, vs_option, c):
    wgrad_case(vs_option, c)


@pytest.mark.parametrize("c", R.EDGE_CASES, ids=R.case_id)
def test_dispatch_edge(oracle, vs_option, c):
    """B T_out = 512 exactly runs the split kernel; 508, and T_out % 4 != 0, the fp32 one -- by the plane count -- each within its own bound"""
    wgrad_case(vs_option, c)


# ---- B. workgroups that walk several units (36 on 29 slices), the five staging variants; 36 planes through wgrad_finish_kernel
@pytest.mark.parametrize("c", R.B_CASES, ids=R.case_id)
def test_split_kernel_several_units_per_workgroup(oracle, vs_option, c):
    wgrad_case(vs_option, c)


# ---- C. impulse group: one nonzero column of gy, one nonzero product per output, the DERIVED bounds
@pytest.mark.parametrize("split", [True, False], ids=["split", "f32"])
@pytest.mark.parametrize("c", R.C_CASES + [R.C_GAINS], ids=R.case_id)
def test_impulse(oracle, vs_option, c, split):
    c = c._replace(split=split)
    for col in R.C_COLS:
        got, gy, x, pad, ref, S = wgrad_case(vs_option, c, impulse=col, F=R.F_IMPULSE if split else R.F_IMPULSE_F32)
        n = col[1] + np.arange(c.K) * c.dil - pad
        outside = (n < 0) | (n >= x.shape[2])
        assert np.all(S[:, :, outside] == 0) and not got.cpu().numpy()[:, :, outside].any()          # x position in the padding: exactly 0


# ---- D. the callers' layouts
@pytest.mark.parametrize("Cin,Cout,K,u,B,T,with_gains", R.D_TRANSPOSED)
def test_transposed_conv_role_swap(oracle, vs_option, monkeypatch, Cin, Cout, K, u, B, T, with_gains):
    """autograd.conv_backward on a HipConvTranspose1d: x in the place of gy over the de-interleaved phases of gy, taps padded to Q u and the gradient cut back to K"""
    from visinger_amd import autograd as A
    from visinger_amd.modules.hipconv import HipConvTranspose1d
    calls = []
    real = A.conv_wgrad
    monkeypatch.setattr(A, "conv_wgrad", lambda gy_, x_, k, dil=1, pad=0, bias=False: (calls.append((tuple(gy_.shape), tuple(x_.shape), k, dil, pad, bias)), real(gy_, x_, k, dil, pad, bias))[1])
    rB, rCo, rCi, rT, Q = R.transposed_role(Cin, Cout, K, u, B, T)
    name = reach(vs_option, rB, rCo, rCi, rT, Q, True)
    x, gy, p = R.transposed_inputs(Cin, Cout, K, u, B, T, with_gains)
    m = HipConvTranspose1d(Cin, Cout, K, u, padding=p).cuda()
    w = torch.zeros(Cin, Cout, K, device="cuda")
    _, gw = A.conv_backward(m, dev(x), w, dev(gy), False, True)
    torch.cuda.synchronize()
    assert calls == [((rB, rCo, rT), (rB, rCi, rT + Q - 1), Q, 1, 0, False)], calls
    ref, S = R.expected_transposed(gy, x, K, u, p)
    assert tuple(gw.shape) == ref.shape == (Cin, Cout, K)
    R.assert_close(gw, ref, S, "%s tconv %d->%d k%d u%d B%d T%d%s" % (name, Cin, Cout, K, u, B, T, " gains" if with_gains else ""))


def test_strided_dense_conv_with_bias(oracle, vs_option, monkeypatch):
    """StridedConv1dFn.backward at a shape its own rule sends to conv_wgrad(gyF, XF, Q, 1, 0, bias=True): the items end to end with zero columns between them"""
    from visinger_amd import autograd as A
    N, C, Cout, K, stride, pad, T = R.D_STRIDED
    calls = []
    real = A.conv_wgrad
    monkeypatch.setattr(A, "conv_wgrad", lambda gy_, x_, k, dil=1, pad=0, bias=False: (calls.append((tuple(gy_.shape), tuple(x_.shape), k, dil, pad, bias)), real(gy_, x_, k, dil, pad, bias))[1])
    rB, rCo, rCi, rT, Q = R.strided_role(*R.D_STRIDED)
    name = reach(vs_option, rB, rCo, rCi, rT, Q, True)
    x, gy = R.strided_inputs(*R.D_STRIDED)
    holder = torch.nn.Conv1d(C, Cout, K, stride, padding=pad).cuda()
    w, b = holder.weight, holder.bias
    y = A.StridedConv1dFn.apply(dev(x), w, b, stride, pad, holder)
    assert tuple(y.shape) == gy.shape
    gw, gb = torch.autograd.grad(y, (w, b), dev(gy))
    torch.cuda.synchronize()
    assert calls == [((1, rCo, rT), (1, rCi, rT + Q - 1), Q, 1, 0, True)], calls
    ref, S = R.expected_strided(gy, x, K, stride, pad)
    what = "%s strided conv N%d %d->%d k%d s%d T%d" % (name, N, C, Cout, K, stride, T)
    assert tuple(gw.shape) == ref.shape == (Cout, C, K)
    R.assert_close(gw, ref, S, what)
    bref, bS = R.expected_bias(gy)
    R.assert_close(gb, bref, bS, what + " bias", F=R.F_BIAS)


# ---- E. exact-fp32 kernel: the plain fp64 gradient, F_WGRAD_F32
@pytest.mark.parametrize("c", R.E_CASES, ids=R.case_id)
def test_fp32_kernel(oracle, vs_option, c):
    wgrad_case(vs_option, c)


# ---- F. fused bias gradient (gw bit-identical to the plain call: tests/test_train_gpu.py::test_wgrad_with_fused_bias_gradient)
@pytest.mark.parametrize("c", R.F_CASES, ids=R.case_id)
def test_fused_bias_gradient(oracle, vs_option, c):
    wgrad_case(vs_option, c, bias=True)
