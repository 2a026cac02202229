"""PM-VDVAE on CelebA 64 x 64 x 3.  Not a reference config: the reference ships a PM-VDVAE config for MNIST only.  This is
configs/pm_vdvae_mnist.py with the image shape, dataset and mask generator of the CelebA models and block strings over
the resolution chain 64 / 32 / 16 / 8 / 4 / 1."""
from posterior_matching_amd.config_dict import ConfigDict


def get_config():
    config = ConfigDict()

    config.data = ConfigDict()
    config.data.dataset = "celeb_a"
    config.data.train_split = "train"
    config.data.validation_split = "test"
    # Per-device batch size (one process per GPU here).  The paper's models used 8 accelerators,
    # i.e. a global batch of 128.
    config.data.train_batch_size = 16
    config.data.val_batch_size = 16
    config.data.mask_generator = "CelebAMaskGenerator"

    config.model = ConfigDict()
    config.model.image_shape = (64, 64, 3)
    config.model.encoder_blocks = "64x3,64d2,32x3,32d2,16x3,16d2,8x3,8d2,4x3,4d4,1x2"
    config.model.decoder_blocks = "1x2,4m1,4x3,8m4,8x3,16m8,16x3,32m16,32x3,64m32,64x3"
    config.model.latent_dim = 16
    config.model.width = 192
    config.model.bottleneck_multiple = 0.25
    config.model.no_bias_above = 64
    config.model.num_mixtures = 10
    config.model.custom_width_string = None

    config.ema_rate = 0.999
    config.gradient_clip = 200.0
    config.lr = 0.00015

    config.steps = 500000
    config.validation_freq = 5000

    return config
