"""The fused encoder forward (csrc/pm_conv_stack.hip: a ConvEncoder's first four layers in one launch) against the
layer-wise launches it replaces: the same bits in all four outputs, the same gradients and parameters after training steps,
and the layer-wise path for stacks the planner does not accept."""
import pytest
import torch

from posterior_matching_amd import ops
from posterior_matching_amd.models.core import Feat, ParamStore, Workspace
from posterior_matching_amd.models.networks import ConvEncoder

pytestmark = pytest.mark.gpu

MNIST_LAYERS = [(32, 5, 1), (32, 5, 2), (64, 5, 1), (64, 5, 2), (128, 7, 1)]


def dev():
    return torch.device("cuda:0")


def build_encoder(c0, layers=MNIST_LAYERS, seed=11):
    store, ws = ParamStore(), Workspace(dev())
    enc = ConvEncoder(layers)
    enc.ws = ws
    enc.build(store, "enc", (28, 28, c0))
    store.allocate(dev(), seed)
    gen = torch.Generator().manual_seed(seed)
    vals = {}
    for n, t in store.to_dict("p").items():       # weights of both signs, biases that move the pre-activations across zero
        vals[n] = 0.05 * torch.randn(t.shape, generator=gen) if n.endswith("/b") else t.cpu() * 1.5
    store.load_dict(vals)
    return enc, store


def encoder_outs(enc, x, fused, monkeypatch):
    if fused:
        monkeypatch.delenv("PM_NO_CONV_STACK", raising=False)
    else:
        monkeypatch.setenv("PM_NO_CONV_STACK", "1")
    ops.coverage_begin()
    try:
        enc(Feat(x))
        torch.cuda.synchronize()
    finally:
        names = ops.coverage_end()
    return [o.clone() for o in enc._outs], names


def images(B, c0, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 28, 28, c0), generator=gen)
    x[:, :, :3] = -x[:, :, :3].abs()                   # negative values at the zero-padded borders
    x[:, -2:] = 4.0 * x[:, -2:]
    return x.to(dev())


@pytest.mark.parametrize("c0", [1, 2])
@pytest.mark.parametrize("B", [128, 256])
def test_fused_encoder_forward_is_bit_identical(c0, B, monkeypatch):
    enc, _ = build_encoder(c0)
    x = images(B, c0, 100 + B + c0)
    want, n_ref = encoder_outs(enc, x, False, monkeypatch)
    got, n_fused = encoder_outs(enc, x, True, monkeypatch)
    assert any(n.startswith("conv_stack_fwd_bf16_kernel") for n in n_fused), n_fused
    assert not any(n.startswith("conv_stack_fwd_bf16_kernel") for n in n_ref), n_ref
    assert not any(n.startswith("thin_conv_lane_kernel") or n.startswith("image_conv_bf16_kernel") for n in n_fused), n_fused
    assert len(got) == len(want) == 5
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (i, (a - b).abs().max().item())


@pytest.mark.parametrize("c0", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
def test_fused_launch_at_small_batches(c0, B, monkeypatch):
    """Below 128 images the dispatch keeps the layer-wise path (its other kernel forms); the fused launch itself computes every
    image on its own, so its B images equal the first B of a layer-wise run at 128."""
    enc, store = build_encoder(c0)
    x = images(128, c0, 7 + c0)
    want, _ = encoder_outs(enc, x, False, monkeypatch)
    geoms = enc.geoms[:4]
    assert ops.conv_stack_lds(geoms, B) is not None and not ops.conv_stack_applies(geoms, B)
    outs = [torch.full((B, g.OH, g.OW, g.CO), float("nan"), device=dev()) for g in geoms]
    ws = [store.split_view(enc._ws[i][0]) for i in range(1, 4)]
    ops.conv_stack_fwd(geoms, x[:B].contiguous(), enc.P("conv_0/w"), enc.P("conv_0/b"), ws,
                       [enc.P(f"conv_{i}/b") for i in range(1, 4)], outs)
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(outs[i], want[i][:B]), (i, (outs[i] - want[i][:B]).abs().max().item())


def test_non_qualifying_stack_runs_layer_wise(monkeypatch):
    layers = [(32, 3, 1), (32, 5, 2), (64, 5, 1), (64, 5, 2), (128, 7, 1)]      # a 3x3 first layer
    enc, _ = build_encoder(1, layers)
    assert not ops.conv_stack_applies(enc.geoms[:4], 256)
    x = images(256, 1, 3)
    got, names = encoder_outs(enc, x, True, monkeypatch)
    want, _ = encoder_outs(enc, x, False, monkeypatch)
    assert not any(n.startswith("conv_stack_fwd_bf16_kernel") for n in names), names
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_train_steps_bit_identical_with_the_fused_encoders(monkeypatch):
    """PM-VAE training at the benchmarked batch: both encoders on the fused launch against both on the layer-wise path -
    gradients and parameters equal bit for bit after three steps."""
    from posterior_matching_amd import optim
    from posterior_matching_amd.engine import PMVAETrainStep
    from posterior_matching_amd.models import PosteriorMatchingVAE
    from tests.ref_configs import pm_vae_mnist

    cfg, B, xs = pm_vae_mnist(), 256, (28, 28, 1)
    gen = torch.Generator().manual_seed(21)
    batches = [(torch.rand((B,) + xs, generator=gen), (torch.rand((B,) + xs, generator=gen) < 0.5).float(),
                torch.randn((B, 32), generator=gen)) for _ in range(3)]
    res = {}
    for fused in (False, True):
        if fused:
            monkeypatch.delenv("PM_NO_CONV_STACK", raising=False)
        else:
            monkeypatch.setenv("PM_NO_CONV_STACK", "1")
        model = PosteriorMatchingVAE.from_config(cfg["model"], device="cuda:0", seed=3)
        model.init(xs)
        opt = optim.chain(optim.scale_by_adam(), optim.add_decayed_weights(0.0),
                          optim.scale_by_schedule(optim.exponential_decay(**cfg["lr_schedule"])), optim.scale(-1.0))
        ts = PMVAETrainStep(model, cfg, opt, B, xs, use_graph=False, external_eps=True)
        ops.coverage_begin()
        try:
            for x, b, eps in batches:
                ts.set_batch(x.cuda(), b.cuda(), eps.cuda())
                ts.step()
            torch.cuda.synchronize()
        finally:
            names = ops.coverage_end()
        launched = sum(n.startswith("conv_stack_fwd_bf16_kernel") for n in names)
        assert launched == (2 if fused else 0), names            # <1, ...> and <2, ...>: both encoders
        res[fused] = ({n: t.clone() for n, t in model.params_dict().items()},
                      {n: t.clone() for n, t in model.grads_dict().items()}, ts.read_metrics())
    for n, p in res[False][0].items():
        assert torch.equal(res[True][0][n], p), n
    for n, g in res[False][1].items():
        assert torch.equal(res[True][1][n], g), n
    assert res[True][2] == res[False][2]
