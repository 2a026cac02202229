"""Colour PM-VDVAE (LogisticMixture with num_channels > 1) - the parts that need no GPU: the model accepts 1 to 4 channels,
the C ABI of the multi-channel likelihood rejects bad arguments before any launch, the synthetic CelebA data in raw-pixel
form, and the CelebA config."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_TINY = dict(encoder_blocks="16x1,16d2,8x1,8d2,4x1,4d4,1x1", decoder_blocks="1x1,4m1,4x1,8m4,8x1,16m8,16x1", latent_dim=4,
             width=32, num_mixtures=10)


def test_vdvae_accepts_one_to_four_channels_and_rejects_five():
    from posterior_matching_amd.models.vdvae import PosteriorMatchingVDVAE

    for C_ in (1, 2, 3, 4):
        m = PosteriorMatchingVDVAE(image_shape=(16, 16, C_), **_TINY)
        assert m.config["image_shape"] == (16, 16, C_)
        assert m.dmol_fields == {1: 3, 2: 6, 3: 10, 4: 15}[C_]     # 2C + C(C-1)/2 + 1
    with pytest.raises(NotImplementedError):
        PosteriorMatchingVDVAE(image_shape=(16, 16, 5), **_TINY)


def test_dmol_mc_argument_checks_without_a_gpu():
    """every bad argument of the three entry points returns PM_EINVAL before anything is launched (no device needed)"""
    from posterior_matching_amd import _lib

    lib = _lib.load()
    p = C.c_void_p(1 << 20)          # never dereferenced: the checks return first
    EINVAL = -1
    rows, Cc, nm, P = 512, 3, 10, 256

    def fwd(params=p, value=p, ll=p, rows=rows, Cc=Cc, nm=nm, P=P):
        return lib.pm_dmol_mc_ll_fwd(None, params, value, ll, rows, Cc, nm, P, 0.0, 255.0)

    def bwd(params=p, value=p, dparams=p, rows=rows, Cc=Cc, nm=nm, P=P):
        return lib.pm_dmol_mc_ll_bwd(None, params, value, 0.5, dparams, rows, Cc, nm, P, 0.0, 255.0)

    def mean(params=p, out=p, rows=rows, Cc=Cc, nm=nm):
        return lib.pm_dmol_mc_mean(None, params, out, rows, Cc, nm, 0.0, 255.0)

    for f, ptrs in ((fwd, ("params", "value", "ll")), (bwd, ("params", "value", "dparams")), (mean, ("params", "out"))):
        for name in ptrs:
            assert f(**{name: None}) == EINVAL, (f.__name__, name)
        for r in (0, -64):
            assert f(rows=r) == EINVAL, (f.__name__, r)
        for c in (-1, 0, 1, 5, 8):
            assert f(Cc=c) == EINVAL, (f.__name__, c)
        for m in (-1, 0, 17, 64):
            assert f(nm=m) == EINVAL, (f.__name__, m)
    for f in (fwd, bwd):
        for bad_p in (0, -1):
            assert f(P=bad_p) == EINVAL, (f.__name__, bad_p)
    assert fwd(rows=500, P=256) == EINVAL           # rows not a multiple of P
    assert fwd(rows=3, P=2) == EINVAL


def test_synthetic_celeb_a_raw_pixels_and_cifar10_shape():
    import numpy as np

    from posterior_matching_amd.data import SyntheticDataset, data_shape

    assert data_shape("cifar10") == (32, 32, 3)
    assert data_shape("celeb_a") == (64, 64, 3)
    ds = SyntheticDataset({"dataset": "celeb_a", "mask_generator": "CelebAMaskGenerator"}, 4, num_batches=2, seed=3,
                          normalize_images=False)
    for batch in ds.batches:
        x = batch["image"].numpy()
        assert x.shape == (4, 64, 64, 3) and x.dtype == np.float32
        assert np.array_equal(x, np.round(x)) and x.min() >= 0 and x.max() <= 255
        assert x.max() > 200 and x.min() < 50                  # spans the range, not U[0, 1]
        assert batch["mask"].shape == (4, 64, 64, 1)
    norm = SyntheticDataset({"dataset": "celeb_a"}, 4, num_batches=1, seed=3).batches[0]["image"]
    assert float(norm.max()) <= 1.0                            # the normalised form is unchanged


def test_celeb_a_config_loads_and_its_block_strings_chain():
    from posterior_matching_amd.config_dict import load_config_file
    from posterior_matching_amd.models.vdvae import parse_layer_string

    cfg = load_config_file(os.path.join(ROOT, "configs", "pm_vdvae_celeb_a.py"))
    m = cfg.model
    assert tuple(m.image_shape) == (64, 64, 3)
    assert cfg.data.dataset == "celeb_a" and cfg.data.mask_generator == "CelebAMaskGenerator"
    res, seen = 64, []
    for r, down in parse_layer_string(m.encoder_blocks):
        assert r == res, (r, res)
        seen.append(r)
        if down is not None:
            res //= down
    assert res == 1 and sorted(set(seen), reverse=True) == [64, 32, 16, 8, 4, 1]
    enc_res = set(seen)
    done = set()
    spec = parse_layer_string(m.decoder_blocks)
    for r, mixin in spec:
        assert r in enc_res, r                                 # every decoder resolution has encoder activations
        if mixin is not None:
            assert mixin in done and mixin < r, (r, mixin)      # mixes in a coarser state that already exists
        done.add(r)
    assert spec[0][0] == 1 and spec[-1][0] == 64
