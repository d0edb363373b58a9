"""Seeded per-item sampling, the part that needs no GPU: the two exports exist and validate their arguments before anything is launched,
the Python layer refuses bad seeds, and the noise stream restated here in numpy / fp64 FROM ITS DEFINITION (DESIGN.md "Seeded sampling":
Philox4x32-10 keyed by the item seed, counter (frame, channel // 4, take, 0), two Box-Muller pairs per call) reproduces the Random123 known
answers.  tests/test_sampling_gpu.py compares the kernel with `stream_ref` below."""
import ctypes

import numpy as np
import pytest
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two -> four uint32 arrays.  All arithmetic in uint64, reduced mod 2^32."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK32 for x in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return [x.astype(np.uint32) for x in c]


def stream_ref(seed, take, H, T):
    """fp64 [H, T]: the item's noise for one take, straight from the definition"""
    q = np.arange((H + 3) // 4, dtype=np.uint64)[:, None]
    t = np.arange(T, dtype=np.uint64)[None, :]
    x = philox4x32_10((t, q, np.uint64(take), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))
    n = np.empty((len(q), 4, T), np.float64)
    for pair in range(2):
        u1 = ((x[2 * pair] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (x[2 * pair + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        n[:, 2 * pair], n[:, 2 * pair + 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return n.reshape(-1, T)[:H]


def noise_ref(seeds, H, T, takes=1, first_take=0):
    """fp64 [B * takes, H, T], item-major like sampling.item_noise"""
    return np.stack([stream_ref(int(s), first_take + k, H, T) for s in seeds for k in range(takes)])


def test_numpy_philox_reproduces_the_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in philox4x32_10(ctr, key)) == want


def test_restated_stream_has_the_documented_figures():
    """the orientation figures of the stream's definition at seed 0x0123456789abcdef, H = 192, T = 1024, take 0"""
    n = stream_ref(0x0123456789abcdef, 0, 192, 1024)
    assert abs(n.mean() - 0.0054) < 5e-5 and abs(n.std() - 1.0004) < 5e-5 and abs(np.abs(n).max() - 4.66) < 5e-3
    assert np.abs(n[0, :3] - [0.110069, -0.381040, -0.254700]).max() < 1e-6
    assert np.abs(n).max() <= np.sqrt(48 * np.log(2))
    # a value depends on (seed, take, channel, frame) only
    assert np.array_equal(stream_ref(7, 3, 6, 24), stream_ref(7, 3, 8, 40)[:6, :24])
    assert not np.array_equal(stream_ref(7, 3, 6, 24), stream_ref(7, 4, 6, 24))


def test_library_exports_the_sampling_entry_points():
    from visinger_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "vs_normal_fill") and hasattr(lib, "vs_prior_sample")
    assert _lib.lib().vs_abi_version() == _lib.EXPECTED_ABI == 7


def test_sampling_arguments_are_validated_before_anything_is_launched():
    """every VS_EINVAL case returns 1 with a message.  The pointers are HOST memory and no call here is valid, so nothing may reach the
    device: without a GPU a launch would come back as VS_EHIP (2), with one it would fault."""
    from visinger_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    two32 = 1 << 32

    def fill(seeds=p, take0=0, K=1, out=p, B=2, H=6, T=5):
        return L.vs_normal_fill(seeds, take0, K, out, B, H, T, None)

    def prior(mu=p, logs=p, bs=None, mask=None, seeds=p, take0=0, K=1, z=p, eps=None, B=2, H=6, T=5):
        return L.vs_prior_sample(mu, logs, 2 * H * T if bs is None else bs, mask, seeds, take0, K, 0.5, z, eps, B, H, T, None)

    bad = [dict(seeds=None), dict(B=0), dict(H=0), dict(T=0), dict(B=-1), dict(H=-3), dict(T=-7), dict(K=0), dict(K=-2), dict(take0=-1),
           dict(take0=two32 - 1, K=2), dict(take0=two32, K=1), dict(take0=0, K=two32 + 1), dict(T=two32 + 1)]
    for kw in bad + [dict(out=None)]:
        assert fill(**kw) == 1, kw
        assert b"vs_normal_fill" in L.vs_last_error(), kw
    for kw in bad + [dict(z=None), dict(mu=None), dict(logs=None), dict(bs=6 * 5 - 1), dict(bs=0), dict(bs=-60)]:
        assert prior(**kw) == 1, kw
        assert b"vs_prior_sample" in L.vs_last_error(), kw


def test_bad_seeds_and_takes_are_refused_on_the_host():
    from visinger_amd import sampling, synth
    for seeds in ([-1], [0, 1 << 63], [1.5], ["7"]):
        with pytest.raises(ValueError, match="seed"):
            sampling.item_noise(seeds, 4, 4)
    for takes, first in ((0, 0), (1, -1), (2, (1 << 32) - 1)):
        with pytest.raises(ValueError, match="takes"):
            sampling.item_noise([1], 4, 4, takes=takes, first_take=first)
    assert sampling.check_seeds([0, (1 << 63) - 1, np.int64(5)]) == [0, (1 << 63) - 1, 5]
    model = torch.nn.Linear(2, 2)               # never reached: the arguments are checked first
    item = dict(text_tokens=np.array([1, 2]), pitch_tokens=np.array([1, 2]), dur_tokens=np.array([1, 2]), mel2ph=np.array([1, 1, 2]))
    with pytest.raises(ValueError, match="seed"):
        synth.synthesize(model, [item], 8, seeds=[-1])
    with pytest.raises(ValueError, match="seed"):
        synth.synthesize(model, [item], 8, seeds=1 << 63)
    with pytest.raises(ValueError, match="1 seeds for 2 items|2 seeds for 1 items"):
        synth.synthesize(model, [item], 8, seeds=[1, 2])
    with pytest.raises(ValueError, match="generator"):
        synth.synthesize(model, [item], 8, seeds=[3], generator=torch.Generator())
    with pytest.raises(ValueError, match="takes"):
        synth.synthesize(model, [item], 8, seeds=[3], takes=0)
    with pytest.raises(ValueError, match="give seeds"):
        synth.synthesize(model, [item], 8, takes=2)


def test_cpu_tensors_are_refused():
    from visinger_amd import _lib, sampling
    with pytest.raises(_lib.VisingerHipError):
        sampling.item_noise(torch.zeros(2, dtype=torch.int64), 4, 4)
    with pytest.raises(_lib.VisingerHipError):
        sampling.prior_sample(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), None, [1])
