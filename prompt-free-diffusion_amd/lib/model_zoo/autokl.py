"""AutoencoderKL ('autoencoderkl') on the HIP path.

Surface of the reference's lib/model_zoo/autokl.py:14-60: ctor `(ddconfig, lossconfig,
embed_dim)`, sub-modules `encoder / decoder / quant_conv / post_quant_conv` (state-dict keys),
`encode(x, out_posterior=False)` (x in [0,1] -> x*2-1 -> moments -> sample) and `decode(z)`
((dec+1)/2 clamped to [0,1]).  The LPIPS/discriminator loss (autokl_utils.py) is training-only
and not built (`lossconfig: null`, autokl.yaml:21).

decode: the `1/scale * z` of pfd.vae_decode (pfd.py:277-281) rides on the NCHW->NHWC boundary
kernel and `(x+1)/2` + clamp on the NHWC->NCHW one, so the decoder body is 100 % fused
GN+swish / MFMA conv kernels.
"""
import torch
import torch.nn as nn

from ..hip import layers as L
from ..hip import ops
from .autokl_modules import Decoder, Encoder
from .common.get_model import register


class DiagonalGaussianDistribution(object):
    """posterior of the VAE encoder (reference distributions.py:24-62); [B, 2*zc, h, w] moments.
    A few KB of fp32 elementwise math on the host-visible result, not a kernel."""

    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if deterministic:
            self.var = self.std = torch.zeros_like(self.mean)

    def sample(self):
        return self.mean + self.std * torch.randn(self.mean.shape).to(device=self.parameters.device,
                                                                      dtype=self.mean.dtype)

    def mode(self):
        return self.mean


@register('autoencoderkl')
class AutoencoderKL(nn.Module):
    def __init__(self, ddconfig, lossconfig, embed_dim):
        super().__init__()
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        if lossconfig is not None:
            raise NotImplementedError("LPIPSWithDiscriminator is training-only and out of scope")
        assert ddconfig["double_z"]
        self.quant_conv = L.Conv2d(2 * ddconfig["z_channels"], 2 * embed_dim, 1)
        self.post_quant_conv = L.Conv2d(embed_dim, ddconfig["z_channels"], 1)
        self.embed_dim = embed_dim

    @torch.no_grad()
    def encode(self, x, out_posterior=False):
        return self.encode_trainable(x, out_posterior)

    def encode_trainable(self, x, out_posterior=False):
        moments = ops.to_nchw(self.encode_moments_nhwc(x, layout='nchw'), x.dtype)
        posterior = DiagonalGaussianDistribution(moments)
        return posterior if out_posterior else posterior.sample()

    def encode_moments_nhwc(self, x, layout=None):
        """picture in [0, 1] -> the posterior's moments as the quant_conv GEMM leaves them: f16 NHWC [B, H/8, W/8, 2*zc],
        per pixel the zc means, then the zc logvars (what ops.latent_start reads; `encode` is this + ops.to_nchw).
        x: NCHW float [B, 3, H, W], or -- layout 'nhwc' -- the f16 NHWC [B, H, W, 3] of ops.image_from_u8(...,
        layout='nhwc').  layout None: 'nhwc' for an f16 tensor with 3 channels last and not 3 second.  A deterministic
        function of x and the weights: capturable."""
        if layout is None:
            layout = 'nhwc' if (x.dtype == torch.float16 and x.dim() == 4 and x.shape[3] == 3 and x.shape[1] != 3) else 'nchw'
        if layout == 'nhwc':
            if not (x.dtype == torch.float16 and x.dim() == 4 and x.shape[3] == 3 and x.is_contiguous()):
                raise ValueError("encode_moments_nhwc: an NHWC picture must be a dense f16 tensor [B, H, W, 3]")
            # x*2-1 without a change of layout: the boundary kernel on the picture seen as one row of one channel
            xin = ops.to_nhwc(x.reshape(1, 1, 1, -1), mul=2.0, add=-1.0).reshape(x.shape)
        elif layout == 'nchw':
            xin = ops.to_nhwc(x, mul=2.0, add=-1.0)
        else:
            raise ValueError(f"encode_moments_nhwc: layout must be 'nchw' or 'nhwc', got {layout!r}")
        return self.quant_conv.hip(self.encoder.hip(xin))

    @torch.no_grad()
    def decode(self, z, in_scale=1.0, out_uint8=False):
        """z NCHW latent (already multiplied by in_scale inside) -> image NCHW in [0, 1];
        out_uint8: packed uint8 [B, H, W, 3] instead (the bytes `ToPILImage` would produce, app.py:273-275)"""
        h = self.decode_nhwc(ops.to_nhwc(z, mul=float(in_scale)))
        if out_uint8:
            return ops.image_u8(h, mul=0.5, add=0.5, f16_image=z.dtype == torch.float16)
        return ops.to_nchw(h, z.dtype, mul=0.5, add=0.5, lo=0.0, hi=1.0)

    def decode_nhwc(self, z_nhwc):
        return self.decoder.hip(self.post_quant_conv.hip(z_nhwc))

    def decode_trainable(self, z):
        h = self.decode_nhwc(ops.to_nhwc(z))
        return ops.to_nchw(h, z.dtype, mul=0.5, add=0.5)
