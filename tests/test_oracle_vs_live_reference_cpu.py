"""The oracle against the reference at the production width (hidden 192, gin 256, 512 initial generator channels): the other golden
vectors pin the oracle at small sizes; this closes the gap to full size ("Full-size parity on the GPU box is against the
build's own CPU restatement, which is validated against the live oracle here at full size").  The reference's outputs at full width are
stored in tests/golden/full_width.npz (tests/golden/make_golden.py: gen_full_width); its ~30 M seeded weights are not: they are rebuilt
here with the generator's seeded `randomize` on the package's own modules (same state-dict keys and order as the reference's) and checked
against the sha256 recorded with the outputs.  Only the checkpoint test below runs the reference itself, where a checkout of it exists."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

REF = os.environ.get("VISINGER_REFERENCE", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "modules")), reason="reference checkout not present")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    """the golden-vector generator's import shim (mocks the audio front-end packages the hot path never touches)"""
    import sys
    import torch
    before_modules, before_path = set(sys.modules), list(sys.path)
    grad, threads = torch.is_grad_enabled(), torch.get_num_threads()
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(__file__), "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    yield mod
    # leave the session as it was: the shim puts the reference's top-level packages (modules, models, utils) on sys.path and
    # switches autograd off process-wide
    torch.set_grad_enabled(grad)
    torch.set_num_threads(threads)
    sys.path[:] = before_path
    for name in set(sys.modules) - before_modules:
        del sys.modules[name]


@pytest.fixture(scope="module")
def full_width():
    z = np.load(os.path.join(GOLDEN, "full_width.npz"))
    return {k: z[k] for k in z.files}


def randomize(module, seed, scale=1.0):
    """tests/golden/make_golden.py `randomize`, the rule the fixture's weights were drawn by (the sha256 check below holds the two together)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("weight_g"):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif name.endswith("gamma"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("beta") or name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "emb_rel" in name:
                p.copy_(torch.randn(p.shape, generator=g) * (p.shape[-1] ** -0.5))
            else:
                fan = max(1, int(np.prod(p.shape[1:])))
                p.copy_(scale * torch.randn(p.shape, generator=g) / np.sqrt(fan))
    return module


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).tobytes())
    return h.hexdigest()


def _seeded(module, seed, scale, want_sha):
    """the fixture's weights, rebuilt: refuses to compare against outputs of other weights"""
    randomize(module.eval(), seed, scale)
    assert _sha(*module.state_dict().values()) == str(want_sha), f"seeded weights differ from the fixture's ({type(module).__name__}, seed {seed})"
    return module


def _sd(m):
    return {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


def _close(got, want, tol):
    want = want.detach().numpy() if hasattr(want, "detach") else np.asarray(want)
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    assert err <= tol, err


def test_full_width_flow_and_generator(full_width, oracle):
    import torch
    from visinger_amd.modules.visinger.decoder import Generator
    from visinger_amd.modules.visinger.flow import ResidualCouplingBlock
    fw = full_width
    B, T = 1, 12
    flow = _seeded(ResidualCouplingBlock(192, 192, 5, 1, 4, gin_channels=256), 201, 0.5, fw["flow.sha"])
    gen = _seeded(Generator(192, "1", [3, 7, 11], [[1, 3, 5]] * 3, [8, 8, 2, 2], 512, [16, 16, 4, 4], gin_channels=256), 202, 1.0, fw["gen.sha"])
    gen300 = _seeded(Generator(192, "1", [3, 7, 11], [[1, 3, 5]] * 3, [5, 5, 3, 2, 2], 512, [11, 11, 7, 4, 4], gin_channels=256), 203, 1.0,
                     fw["gen300.sha"])
    g = torch.Generator().manual_seed(7)
    z = torch.randn(B, 192, T, generator=g)
    cond = torch.randn(B, 256, 1, generator=g)
    mask = torch.ones(B, 1, T)
    mask[0, :, 10:] = 0
    assert _sha(z, cond, mask) == str(fw["in1.sha"])
    kw = dict(channels=192, hidden_channels=192, kernel_size=5, dilation_rate=1, n_layers=4)
    for reverse, key in ((False, "flow.fwd"), (True, "flow.inv")):
        _close(oracle.flow_block(_sd(flow), z.numpy(), mask.numpy(), cond.numpy(), reverse, **kw), fw[key], 5e-5)
    _close(oracle.generator(_sd(gen), z.numpy(), cond.numpy(), resblock="1", resblock_kernel_sizes=[3, 7, 11],
                            resblock_dilation_sizes=[[1, 3, 5]] * 3, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4]),
           fw["gen.y"], 5e-5)
    _close(oracle.generator(_sd(gen300), z.numpy(), cond.numpy(), resblock="1", resblock_kernel_sizes=[3, 7, 11],
                            resblock_dilation_sizes=[[1, 3, 5]] * 3, upsample_rates=[5, 5, 3, 2, 2],
                            upsample_kernel_sizes=[11, 11, 7, 4, 4]), fw["gen300.y"], 5e-5)


def test_full_width_transformers_and_posterior(full_width, oracle):
    import torch
    from visinger_amd.modules.rel_transformer import RelativeEncoder
    from visinger_amd.modules.visinger.encoder import PosteriorEncoder
    fw = full_width
    B, T = 2, 70
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, 192, T, generator=g)
    mask = torch.ones(B, 1, T)
    mask[1, :, 50:] = 0
    enc = _seeded(RelativeEncoder(192, 768, 2, 4, kernel_size=9, gin_channels=1), 204, 1.0, fw["enc.sha"])
    cond = torch.randn(B, 1, T, generator=g)
    post = _seeded(PosteriorEncoder(1025, 192, 192, 5, 1, 16, gin_channels=256), 205, 0.5, fw["post.sha"])
    spec = torch.randn(B, 1025, T, generator=g).abs()
    spk = torch.randn(B, 256, 1, generator=g)
    assert _sha(x, mask, cond, spec, spk) == str(fw["in2.sha"])
    _close(oracle.rel_encoder(_sd(enc), x.numpy(), mask.numpy(), cond.numpy(), n_heads=2, n_layers=4, kernel_size=9),
           fw["enc.y"], 1e-4)
    z = fw["post.z"]
    zo, muo, logso = oracle.posterior_encoder(_sd(post), spec.numpy(), mask.numpy(), spk.numpy(), fw["post.noise"], out_channels=192,
                                              hidden_channels=192, kernel_size=5, dilation_rate=1, n_layers=16)
    _close(muo, fw["post.mu"], 1e-4)
    _close(logso, fw["post.logs"], 1e-4)
    assert float(np.abs(zo - z).max() / (1.0 + np.abs(z).max())) <= 1e-4


@needs_reference
def test_reference_ckpt_utils_reads_our_checkpoint(ref, tmp_path):
    """SURVEY 8f-4 pinned against the reference rather than against ourselves: a file written by visinger_amd.ckpt.save_checkpoint
    is found and loaded by the reference's own utils/commons/ckpt_utils.py (get_all_ckpts: newest first; load_ckpt(strict=True),
    ckpt_utils.py:17-63) into the REFERENCE's modules, whose forward then equals the golden output of the weights we saved; and a
    legacy-serialised file laid out as the reference's Trainer writes it (trainer.py:473-492) loads into ours."""
    import torch
    from conftest import load_golden
    from visinger_amd import ckpt
    from visinger_amd.modules.visinger.flow import ResidualCouplingBlock as OurFlow
    spec = importlib.util.spec_from_file_location("ref_ckpt_utils", os.path.join(REF, "utils", "commons", "ckpt_utils.py"))
    ref_ckpt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_ckpt)

    w, a = load_golden("flow_block")
    C, H, k, dr, n_layers, n_flows, gin = (int(v) for v in a["cfg"])
    ctor = (C, H, k, dr, n_layers)
    ours = OurFlow(*ctor, n_flows=n_flows, gin_channels=gin)
    ours.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()}, strict=True)
    opt = torch.optim.AdamW(ours.parameters(), lr=2e-4, betas=(0.8, 0.99), eps=1e-9)
    ckpt.save_checkpoint(tmp_path / "model_ckpt_steps_100.ckpt", {"model": ours}, [opt], epoch=1, global_step=100)
    ckpt.save_checkpoint(tmp_path / "model_ckpt_steps_2500.ckpt", {"model": ours}, [opt], epoch=9, global_step=2500)

    found = ref_ckpt.get_all_ckpts(str(tmp_path))
    assert [os.path.basename(p) for p in found] == ["model_ckpt_steps_2500.ckpt", "model_ckpt_steps_100.ckpt"]
    theirs = ref.ResidualCouplingBlock(*ctor, n_flows=n_flows, gin_channels=gin).eval()
    ref_ckpt.load_ckpt(theirs, str(tmp_path), model_name="model", strict=True)          # the reference's loader, directory form
    for (k1, v1), (k2, v2) in zip(theirs.state_dict().items(), ours.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    x, mask, g = torch.from_numpy(a["x"]), torch.from_numpy(a["mask"]), torch.from_numpy(a["g"])
    np.testing.assert_allclose(theirs(x, mask, g=g).numpy(), a["y"], atol=1e-6)      # the golden output of the weights we saved
    raw, path = ref_ckpt.get_last_checkpoint(str(tmp_path))
    assert path.endswith("2500.ckpt") and raw["global_step"] == 2500 and len(raw["optimizer_states"]) == 1

    # the other direction: the layout the reference's Trainer.save_checkpoint writes (legacy pickle of this dict)
    theirs2 = ref.randomize(ref.ResidualCouplingBlock(*ctor, n_flows=n_flows, gin_channels=gin), 77)
    their_file = tmp_path / "theirs" / "model_ckpt_steps_40.ckpt"
    os.makedirs(their_file.parent)
    torch.save({"epoch": 0, "global_step": 40, "checkpoint_callback_best": 1e9, "optimizer_states": [],
                "state_dict": {"model": theirs2.state_dict()}}, their_file, _use_new_zipfile_serialization=False)
    mine = OurFlow(*ctor, n_flows=n_flows, gin_channels=gin)
    step, _ = ckpt.load_model(mine, str(their_file.parent), child="model", strict=True)
    assert step == 40
    for (k1, v1), (k2, v2) in zip(theirs2.state_dict().items(), mine.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
