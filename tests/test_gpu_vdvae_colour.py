"""GPU parity of the colour PM-VDVAE: LogisticMixture(num_channels = C > 1) with autoregressive channel coefficients
(reference posterior_matching/models/vdvae.py:331-476) through pm_dmol_mc_* and through the whole model, train step and
evaluation paths.

The float64 restatement of the multi-channel log_prob / mean lives here (oracle/vdvae_oracle.py states the one-channel case
only); the whole-model tests patch it into the oracle's two likelihood names, which every oracle call site goes through."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import vdvae_oracle as DO

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NOUT = {1: 3, 2: 6, 3: 10, 4: 15}        # 2C + C(C-1)/2 + 1 fields per mixture component


def dev():
    return torch.device("cuda:0")


def rel_err(a, b):
    from tests import conftest

    conftest.confirm_compared()
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def f32d(t):
    return t.float().to(dev()).contiguous()


# ----------------------------------------------------------------------------------------------
# float64 restatement of _LogisticMixtureDist with coefficients
# ----------------------------------------------------------------------------------------------
def _channels(params, nm):
    no = params.shape[-1] // nm
    return {v: k for k, v in _NOUT.items()}[no], no


def _split(params, nm):
    C, no = _channels(params, nm)
    pr = params.reshape(*params.shape[:-1], nm, no)
    K = C * (C - 1) // 2
    return C, pr[..., 0], pr[..., 1:C + 1], pr[..., C + 1:2 * C + 1], pr[..., 2 * C + 1:2 * C + 1 + K]


def mc_log_prob(params, value, num_mixtures, low=0.0, high=255.0, independent=True):
    """log_prob (:351-394): loc_i += sum_{j<i} coef_ij * (2 (x_j - low) / (high - low) - 1) in the [-1, 1] space, raw
    coefficients, then the quantised logistic of every channel, Independent over channels, MixtureSameFamily."""
    B, H, W, _ = params.shape
    C, logits, locs, raw, coefs = _split(params, num_mixtures)
    value = value.reshape(B, H, W, C).to(params.dtype)
    xt = (2.0 * (value - low) / (high - low) - 1.0).unsqueeze(-2)          # [B,H,W,1,C], unclamped
    cols, q = [], 0
    for i in range(C):
        li = locs[..., i]
        for j in range(i):
            li = li + coefs[..., q] * xt[..., j]
            q += 1
        cols.append(li)
    loc = low + 0.5 * (high - low) * (torch.stack(cols, -1) + 1.0)
    sc = (DO.softplus(raw) + math.exp(-7.0)) * 0.5 * (high - low)
    y = value.clamp(low, high).unsqueeze(-2)
    up, dn = (y + 0.5 - loc) / sc, (y - 0.5 - loc) / sc
    lsig = DO._log_sigmoid
    logcdf_y, logsf_y, logcdf_ym1, logsf_ym1 = lsig(up), lsig(-up), lsig(dn), lsig(-dn)
    ninf, zero = torch.full_like(up, -float("inf")), torch.zeros_like(up)
    logcdf_y = torch.where(y >= high, zero, logcdf_y)
    logsf_y = torch.where(y >= high, ninf, logsf_y)
    logcdf_ym1 = torch.where(y <= low, ninf, logcdf_ym1)
    logsf_ym1 = torch.where(y <= low, zero, logsf_ym1)
    use_sf = logsf_y < logcdf_y
    big = torch.where(use_sf, logsf_ym1, logcdf_y)
    small = torch.where(use_sf, logsf_y, logcdf_ym1)
    comp = (big + torch.log1p(-torch.exp(torch.clamp(small - big, max=0.0)))).sum(-1)   # Independent over channels
    lp = torch.logsumexp(torch.log_softmax(logits, -1) + comp, dim=-1)
    return lp.reshape(B, -1).sum(1) if independent else lp


def mc_mean_unrounded(params, num_mixtures, low=0.0, high=255.0):
    """mean (:396-435) before jnp.round: weighted locs AND coeffs, channel by channel, each clipped before it conditions"""
    C, logits, locs, _, coefs = _split(params, num_mixtures)
    w = torch.softmax(logits, -1).unsqueeze(-1)
    lb, cb = (locs * w).sum(-2), (coefs * w).sum(-2)
    ms, q = [], 0
    for i in range(C):
        v = lb[..., i]
        for j in range(i):
            v = v + cb[..., q] * ms[j]
            q += 1
        ms.append(v.clamp(-1.0, 1.0))
    return low + 0.5 * (high - low) * (torch.stack(ms, -1) + 1.0)


def mc_mean(params, num_mixtures, low=0.0, high=255.0):
    return torch.round(mc_mean_unrounded(params, num_mixtures, low, high))


def _assert_mean_exact(got, params64, nm):
    """exact, except at a pixel whose float64 value before rounding lies within 1e-4 of a .5 tie (counted, <= 1 apart)"""
    pre = mc_mean_unrounded(params64, nm)
    want = torch.round(pre)
    got = got.detach().cpu().double().reshape(want.shape)
    tie = ((pre - pre.floor()) - 0.5).abs() < 1e-4
    diff = (got - want).abs()
    assert diff.max().item() <= 1.0
    assert torch.equal(got[~tie], want[~tie]), int((diff[~tie] > 0).sum())
    return int(tie.sum())


# ----------------------------------------------------------------------------------------------
# the kernels against the restatement
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("nm", [1, 10, 16])
@pytest.mark.parametrize("B,H", [(3, 7), (2, 11), (5, 3)])
def test_dmol_mc_log_prob_mean_and_grads(C, nm, B, H):
    """rows B*H*H = 147 / 242 / 45: not multiples of 64 or 256; examples of 49 / 121 / 9 pixels straddle waves"""
    from posterior_matching_amd import ops

    gen = torch.Generator().manual_seed(100 * C + nm + H)
    no = _NOUT[C]
    params = torch.randn((B, H, H, nm * no), generator=gen, dtype=F64)
    pv = params.view(B, H, H, nm, no)
    pv[..., C + 1:2 * C + 1] -= 1.5                                          # some sharp components
    x = torch.randint(0, 256, (B, H, H, C), generator=gen).double()
    for c in range(C):                                                       # the open edge bins in every channel
        x[0, 0, c, c] = 0.0
        x[-1, -1, c, c] = 255.0
    x[0, 1, 0] = 0.0
    x[0, 1, 1] = 255.0
    P = H * H
    prr = params.clone().requires_grad_(True)
    ll = mc_log_prob(prr, x, nm)
    (0.3 * ll.sum()).backward()
    lld = torch.empty(B, device=dev())
    ops.dmol_mc_ll_fwd(f32d(params), f32d(x), lld, nm, P)
    torch.cuda.synchronize()
    assert rel_err(lld, ll) < 1e-5
    pix = torch.empty(B * P, device=dev())
    ops.dmol_mc_ll_fwd(f32d(params), f32d(x), pix, nm, 1)
    assert rel_err(pix, mc_log_prob(params, x, nm, independent=False).reshape(-1)) < 1e-5
    dp = torch.full((B, H, H, nm * no), float("nan"), device=dev())          # every element must be written
    ops.dmol_mc_ll_bwd(f32d(params), f32d(x), 0.3, dp, nm, P)
    assert torch.isfinite(dp).all()
    assert rel_err(dp, prr.grad) < 2e-5
    mean = torch.empty((B, H, H, C), device=dev())
    ops.dmol_mc_mean(f32d(params), mean, nm)
    torch.cuda.synchronize()
    f32_params = params.float().double()                                     # the kernel reads the f32 rounding
    assert _assert_mean_exact(mean, f32_params, nm) <= max(1, mean.numel() // 1000)


def test_dmol_mc_unaligned_slab_and_four_channels():
    """a params view that starts off a 16-B boundary (is_log_probs reads params[B:]) and C = 4, nm = 16 (largest slab)"""
    from posterior_matching_amd import ops

    gen = torch.Generator().manual_seed(9)
    for C, nm, R in ((3, 10, 67), (4, 16, 130), (2, 3, 65)):
        no = _NOUT[C]
        params = torch.randn((R, nm * no), generator=gen, dtype=F64).float().double()    # what the kernel reads
        x = torch.randint(0, 256, (R, C), generator=gen).double()
        bar = 2e-5 if C < 4 else 5e-5                       # C = 4: four channel terms (and 6 coefficients) per component
        big = torch.zeros(R * nm * no + 1, device=dev())
        view = big[1:].view(R, nm * no)                                     # 4-B offset
        view.copy_(params.float().to(dev()))
        pix = torch.empty(R, device=dev())
        ops.dmol_mc_ll_fwd(view, f32d(x), pix, nm, 1)
        torch.cuda.synchronize()
        assert rel_err(pix, mc_log_prob(params.view(R, 1, 1, -1), x, nm, independent=False).reshape(-1)) < 1e-5
        dbig = torch.full((R * nm * no + 1,), 7.0, device=dev())
        prr = params.clone().requires_grad_(True)
        mc_log_prob(prr.view(R, 1, 1, -1), x, nm).sum().backward()
        ops.dmol_mc_ll_bwd(view, f32d(x), 1.0, dbig[1:].view(R, nm * no), nm, 1)
        torch.cuda.synchronize()
        assert dbig[0].item() == 7.0                                         # nothing written outside the view
        assert rel_err(dbig[1:].view(R, nm * no), prr.grad) < bar, C


def test_dmol_mc_normalises_over_all_values():
    """C = 2: for one parameter row, sum of exp(ll) over all 256 x 256 pixel values is 1 (the coefficient conditioning
    shifts channel 1's location by the observed channel 0)"""
    from posterior_matching_amd import ops

    gen = torch.Generator().manual_seed(4)
    nm = 10
    row = torch.randn((1, nm * _NOUT[2]), generator=gen)
    row.view(nm, _NOUT[2])[:, 5] = torch.randn(nm, generator=gen) * 0.8         # non-trivial coefficients
    params = row.repeat(65536, 1).to(dev()).contiguous()
    v = torch.arange(256, dtype=torch.float32)
    vals = torch.stack(torch.meshgrid(v, v, indexing="ij"), -1).reshape(65536, 2).to(dev()).contiguous()
    ll = torch.empty(65536, device=dev())
    ops.dmol_mc_ll_fwd(params, vals, ll, nm, 1)
    torch.cuda.synchronize()
    from tests import conftest

    conftest.confirm_compared()
    assert abs(torch.exp(ll.double()).sum().item() - 1.0) < 1e-5


# ----------------------------------------------------------------------------------------------
# the model, against the patched float64 oracle
# ----------------------------------------------------------------------------------------------
COLOUR = {"model": {"image_shape": (16, 16, 3), "encoder_blocks": "16x1,16d2,8x1,8d2,4x1,4d4,1x1",
                    "decoder_blocks": "1x1,4m1,4x1,8m4,8x1,16m8,16x1", "latent_dim": 4, "width": 32,
                    "bottleneck_multiple": 0.25, "no_bias_above": 64, "num_mixtures": 10, "custom_width_string": None},
          "ema_rate": 0.999, "gradient_clip": 200.0, "lr": 0.00015}


@pytest.fixture
def patched(monkeypatch):
    monkeypatch.setattr(DO, "logistic_mixture_log_prob", mc_log_prob)
    monkeypatch.setattr(DO, "logistic_mixture_mean", mc_mean)


def _setup(cfg, B, seed=5, bf16x3=False, perturb=True):
    from posterior_matching_amd.models.vdvae import PosteriorMatchingVDVAE

    m = PosteriorMatchingVDVAE(**cfg["model"], device="cuda:0", seed=seed)
    m.init()
    m.store.use_bf16 = bf16x3
    if perturb:
        gen = torch.Generator().manual_seed(seed)
        m.load_params({n: t.cpu() + 0.05 * torch.randn(t.shape, generator=gen) for n, t in m.params_dict().items()})
    p64 = {n: t.cpu().double() for n, t in m.params_dict().items()}
    H, _, C = cfg["model"]["image_shape"]
    x, b, eps = _batch(np.random.default_rng(seed), m, B, H, C)
    return m, p64, x, b, eps


def _batch(rng, m, B, H, C):
    x = torch.tensor(np.round(rng.uniform(size=(B, H, H, C)) * 255.0))
    b = torch.tensor((rng.uniform(size=(B, H, H, 1)) < 0.5).astype(np.float64))
    eps = [torch.tensor(rng.normal(size=s)) for s in m.eps_shapes(B)]
    return x, b, eps


@pytest.mark.parametrize("bf16x3", [False, True])
def test_colour_vdvae_forward_and_grads(patched, bf16x3):
    B, C, W, nm = 3, 3, 32, 10
    m, p64, x, b, eps = _setup(COLOUR, B, bf16x3=bf16x3)
    assert tuple(p64["masked_encoder/stem/w"].shape) == (3, 3, C + 1, W)
    assert tuple(p64["encoder/stem/w"].shape) == (3, 3, C, W)
    assert tuple(p64["decoder/out_net/w"].shape) == (1, 1, W, nm * _NOUT[C])
    leaves = {n: t.clone().requires_grad_(True) for n, t in p64.items()}
    loss, aux, out = DO.vdvae_loss(leaves, COLOUR, x, b, eps)
    grads = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    got = m(f32d(x), f32d(b), [f32d(e) for e in eps])
    m.zero_grad()
    m.backward()
    torch.cuda.synchronize()
    tol = 2e-5 if not bf16x3 else 2e-4
    for k in ("reconstruction_ll", "kl", "pm_kl"):
        assert rel_err(got[k], out[k]) < tol, k
    met = m.metrics.cpu().double()
    assert abs(met[0].item() - loss.item()) < tol * abs(loss.item())
    assert abs(met[4].item() - aux["bpd"].item()) < tol * abs(aux["bpd"].item())
    rec = m.reconstruction()
    assert rec.shape == (B, 16, 16, C)
    diff = (rec.cpu().double() - out["reconstruction"]).abs()
    assert diff.max().item() <= 1.0 and (diff > 0).float().mean().item() < (0.01 if bf16x3 else 0.002)
    gd = m.grads_dict()
    worst = max((rel_err(gd[n], grads[n]), n) for n in grads)
    assert worst[0] < (1e-4 if not bf16x3 else 1e-2), worst


def test_colour_vdvae_train_steps_match_oracle(patched):
    """four VDVAETrainStep steps (the launch plan is recorded at step 3 and replayed at step 4) against DO.train_step"""
    from posterior_matching_amd.engine import VDVAETrainStep

    B = 4
    cfg = dict(COLOUR, gradient_clip=30.0)
    m, p64, _, _, _ = _setup(cfg, B)
    ts = VDVAETrainStep(m, cfg["lr"], B, gradient_clip=cfg["gradient_clip"], ema_rate=cfg["ema_rate"], external_eps=True)
    mo, vo = {k: torch.zeros_like(v) for k, v in p64.items()}, {k: torch.zeros_like(v) for k, v in p64.items()}
    ema = {k: v.clone() for k, v in p64.items()}
    p32 = {k: v.float().clone() for k, v in p64.items()}
    m32, v32 = {k: torch.zeros_like(v) for k, v in p32.items()}, {k: torch.zeros_like(v) for k, v in p32.items()}
    rng = np.random.default_rng(11)
    for step in range(4):
        xb, bb, ee = _batch(rng, m, B, 16, 3)
        loss, aux, g = DO.train_step(p64, mo, vo, ema, cfg, xb, bb, ee, step)
        DO.train_step(p32, m32, v32, None, cfg, xb.float(), bb.float(), [e.float() for e in ee], step)
        gn = math.sqrt(sum(float((t ** 2).sum()) for t in g.values()))
        ts.set_batch(f32d(xb), f32d(bb), [f32d(e) for e in ee])
        ts.step()
        met = ts.read_metrics()
        from tests import conftest

        conftest.confirm_compared()
        assert abs(met["loss"] - loss.item()) < 1e-4 * abs(loss.item()), (step, met)
        assert abs(met["grad_norm"] - gn) < 1e-3 * gn
        pd, ed = m.params_dict(), ts.ema_params()
        for n in p64:
            e, e32 = rel_err(pd[n], p64[n]), rel_err(p32[n], p64[n])
            assert e < max(3e-4, 20 * e32) and e < 5e-3, (step, n, e, e32)
            assert rel_err(ed[n], ema[n]) < max(3e-4, 20 * e32), (step, n)
    assert getattr(ts, "_plan", None) is not None and ts.opt_count.item() == 4 and ts.step_dev.item() == 4


def test_colour_vdvae_impute_and_psnr_match_oracle(patched):
    from posterior_matching_amd.models.vdvae import vdvae_imputation_psnr

    B, S = 3, 2
    m, p64, x, b, _ = _setup(COLOUR, B, seed=12)
    rng = np.random.default_rng(4)
    eps = [[torch.tensor(rng.normal(size=s)) for s in m.eps_shapes(B)] for _ in range(S)]
    want = DO.vdvae_impute(p64, COLOUR["model"], x, b, eps)
    got = m.impute(f32d(x), f32d(b), num_samples=S, eps=[[f32d(e) for e in es] for es in eps])
    psnr = vdvae_imputation_psnr(got, f32d(x))
    torch.cuda.synchronize()
    assert got.shape == (B, S, 16, 16, 3)
    diff = (got.cpu().double() - want).abs()
    assert (diff > 0).float().mean().item() < 0.01 and diff.max().item() <= 1.0
    assert rel_err(psnr, DO.imputation_psnr(want, x)) < 1e-2
    obs = b.bool().expand(B, 16, 16, 3)
    assert torch.equal(got.cpu()[:, 0][obs], x.float()[obs])


def test_colour_vdvae_is_log_probs_and_sample_match_oracle(patched):
    B, S = 3, 3
    m, p64, x, b, _ = _setup(COLOUR, B, seed=14)
    rng = np.random.default_rng(5)
    eps = [[torch.tensor(rng.normal(size=s)) for s in m.eps_shapes(B)] for _ in range(S)]
    eps_m = [[torch.tensor(rng.normal(size=s)) for s in m.eps_shapes(B)] for _ in range(S)]
    want_px, want_pxu = DO.vdvae_is_log_probs(p64, COLOUR["model"], x, b, eps, eps_m)
    p32 = {n: t.float() for n, t in p64.items()}
    f32_px, f32_pxu = DO.vdvae_is_log_probs(p32, COLOUR["model"], x.float(), b.float(),
                                            [[e.float() for e in es] for es in eps], [[e.float() for e in es] for es in eps_m])
    got_px, got_pxu = m.is_log_probs(f32d(x), f32d(b), num_samples=S, eps=[[f32d(e) for e in es] for es in eps],
                                     eps_masked=[[f32d(e) for e in es] for es in eps_m])
    torch.cuda.synchronize()
    from tests import conftest

    conftest.confirm_compared()
    scale = max(1.0, want_px.abs().max().item())
    tol_px = max(1e-4 * scale, 20 * (f32_px.double() - want_px).abs().max().item())
    tol_pxu = max(1e-4 * scale, 20 * (f32_pxu.double() - want_pxu).abs().max().item())
    assert (got_px.cpu().double() - want_px).abs().max().item() < tol_px
    assert (got_pxu.cpu().double() - want_pxu).abs().max().item() < tol_pxu
    N = 5
    eps_p = [torch.tensor(rng.normal(size=s)) for s in m.eps_shapes(N)]
    want = DO.vdvae_sample(p64, COLOUR["model"], eps_p)
    got = m.sample(N, eps=[f32d(e) for e in eps_p])
    diff = (got.cpu().double() - want).abs()
    assert got.shape == (N, 16, 16, 3) and (diff > 0).float().mean().item() < 0.02 and diff.max().item() <= 1.0


def test_colour_vdvae_state_is_bit_reproducible():
    """two fresh models from the same seed, 4 steps each (default arithmetic, launch-plan replay): parameters, Adam moments
    and EMA equal bit for bit"""
    from posterior_matching_amd.engine import VDVAETrainStep

    finals = []
    for _ in range(2):
        m, _, x, b, eps = _setup(COLOUR, 4, seed=8, bf16x3=True)
        ts = VDVAETrainStep(m, COLOUR["lr"], 4, gradient_clip=COLOUR["gradient_clip"], ema_rate=COLOUR["ema_rate"], seed=5,
                            external_eps=True)
        ts.set_batch(f32d(x), f32d(b), [f32d(e) for e in eps])
        for _ in range(4):
            ts.step()
        ts.synchronize()
        s = m.store
        finals.append([t.clone() for t in (s.flat_p, s.flat_m, s.flat_v, ts.ema)])
        del ts, m
    for a, c in zip(*finals):
        assert torch.equal(a, c)


def test_one_channel_step_launches_no_multichannel_kernel():
    from posterior_matching_amd import ops
    from tests.test_gpu_vdvae import TINY

    seen = {}
    for name, cfg in (("grey", TINY), ("colour", COLOUR)):
        m, _, x, b, eps = _setup(cfg, 2, seed=3)
        ops.coverage_begin()
        try:
            m(f32d(x), f32d(b), [f32d(e) for e in eps])
            m.zero_grad()
            m.backward()
            m.reconstruction()
            torch.cuda.synchronize()
        finally:
            seen[name] = ops.coverage_end()
    assert not any("_mc_" in k for k in seen["grey"]), sorted(seen["grey"])
    assert any("dmol_kernel" in k or k.startswith("pm_dmol_ll") for k in seen["grey"]), sorted(seen["grey"])
    mc = {k for k in seen["colour"] if "_mc_" in k}
    assert len(mc) == 3, sorted(seen["colour"])                     # fwd, bwd, mean


def test_colour_scripts_end_to_end(tmp_path):
    """train_pm_vdvae.py on configs/pm_vdvae_celeb_a.py (narrow, short block strings at 64 x 64 x 3), then both evaluation
    scripts on its checkpoint"""
    import json
    import pickle
    import subprocess
    import sys

    def run(script, *argv):
        out = subprocess.run([sys.executable, os.path.join(ROOT, script), *argv], cwd=tmp_path, capture_output=True,
                             text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        return out.stdout

    run("train_pm_vdvae.py", "--config", os.path.join(ROOT, "configs", "pm_vdvae_celeb_a.py"), "--config.steps=4",
        "--config.validation_freq=2", "--config.seed=2", "--config.model.width=32", "--config.model.latent_dim=4",
        "--config.data.train_batch_size=4", "--config.data.val_batch_size=4",
        "--config.model.encoder_blocks=64x1,64d4,16x1,16d4,4x1,4d4,1x1",
        "--config.model.decoder_blocks=1x1,4m1,4x1,16m4,16x1,64m16,64x1")
    rd = os.path.join(tmp_path, "runs", os.listdir(os.path.join(tmp_path, "runs"))[0])
    lines = [json.loads(l) for l in open(os.path.join(rd, "tb", "scalars.jsonl"))]
    assert [l["step"] for l in lines] == [2, 4]
    assert all(np.isfinite(l["train_loss"]) and np.isfinite(l["val_loss"]) for l in lines)
    imp = np.load(os.path.join(rd, "tb", "imputations_4.npy"))
    assert imp.dtype == np.uint8 and imp.shape == (4, 64, 64 * 10, 3)
    rec = np.load(os.path.join(rd, "tb", "reconstructions_4.npy"))
    assert rec.dtype == np.uint8 and rec.shape == (4, 64, 64 * 2, 3)
    sys.path.insert(0, ROOT)
    st = pickle.load(open(os.path.join(rd, "train_state.pkl"), "rb"))
    assert st.step == 4 and tuple(st.params["masked_encoder/stem/w"].shape) == (3, 3, 4, 32)
    data = ("--dataset", "celeb_a", "--mask_generator", "CelebAMaskGenerator")
    out = run("eval_pm_vdvae_imputation.py", "--run_dir", rd, *data, "--num_instances", "4", "--batch_size", "4",
              "--num_samples", "2")
    res = json.loads(out.strip().splitlines()[-1])
    assert res["num_instances"] == 4 and np.isfinite(res["mean_psnr"]) and 0.0 < res["mean_psnr"] < 60.0
    out = run("eval_pm_vdvae_likelihood.py", "--run_dir", rd, *data, "--num_instances", "4", "--batch_size", "4",
              "--num_samples", "2", "--num_trials", "1")
    assert "BPD:" in out
    bpd = np.load(os.path.join(rd, "likelihood_results", "bpd.npy"))
    assert np.isfinite(bpd).all() and (bpd > 0).all()
