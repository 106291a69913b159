"""AutoencoderKL (the KL first stage of latent diffusion) with the Diffusers interface, executed by the HIP engine.

Mirrors the reference's `diffusers.models.AutoencoderKL` (autoencoder_kl.py:34-330) and `DiagonalGaussianDistribution`
(vae.py:384-428) for the configuration family `vq.VQModel` builds: DownEncoderBlock2D / UpDecoderBlock2D levels, the mid block of two
resnets around one single-head attention, an encoder head of 2 * latent_channels (`double_z`), quant_conv 2L -> 2L and
post_quant_conv L -> L.  Same constructor arguments, `.config`, state-dict keys and order; the parameter holders are vq.py's.
The network runs on `KLEngine`, which is `vq.VQEngine` without the quantizer; the posterior arithmetic (clamp, exp, sample, KL) is
one launch of csrc/vae.hip, and tiled encode / decode blend each tile into its neighbours and into the canvas with one launch of
the same file.  Forward only, fp32, no grad; there is no CPU / PyTorch fallback.

Tiling is what carries an image past the engine's reach: every activation must stay below the 2 GiB of 32-bit buffer offsets
(ops._extent_bytes), and the mid block's attention scores are 4 (h w)^2 bytes per image -- 1 GiB for a 1024 x 1024 image at f = 8,
16 GiB for a 2048 x 2048 one, where no micro-batch helps.  With tiling the largest tensor is a tile's.
"""
import torch
import torch.nn as nn

from . import ops
from .model_base import BaseOutput
from .vq import Decoder, DecoderOutput, Encoder, FirstStage, VQEngine, autoencoder_config

_NO_FALLBACK = 'runs on the MI355X HIP kernels only (no CPU / PyTorch fallback)'


class AutoencoderKLOutput(BaseOutput):
    """autoencoder_kl.py:27-31: `.latent_dist`."""


# ---- tile geometry (host arithmetic of tiled_encode / tiled_decode, autoencoder_kl.py:222-298) --------------------------
def tile_spans(size, tile, overlap_size):
    """[(start, length)] of the tiles along one axis: `range(0, size, overlap_size)` and the slice `[s : s + tile]`."""
    return [(s, min(int(tile), size - s)) for s in range(0, size, overlap_size)]


def tile_geometry(tile_in, tile_out, overlap_factor):
    """(overlap_size, blend_extent, row_limit): the stride of the tiles on the input side (tile size `tile_in`), and the blend
    extent and crop on the output side (tile size `tile_out`), as the reference forms them."""
    overlap_size = int(tile_in * (1 - overlap_factor))
    blend_extent = int(tile_out * overlap_factor)
    return overlap_size, blend_extent, tile_out - blend_extent


def canvas_layout(lengths, row_limit):
    """Offsets of the cropped tiles along one axis and the canvas length: each tile contributes min(length, row_limit)."""
    offs, at = [], 0
    for n in lengths:
        offs.append(at)
        at += max(0, min(n, row_limit))
    return offs, at


def blend_tiles(rows, blend_extent, row_limit, blend=None):
    """The second loop of tiled_encode / tiled_decode over `rows[i][j]` [N, C, h_i, w_j], in raster order: tile (i, j) takes the
    bottom rows of the blended tile above and the right columns of the blended tile to its left -- in place, so later tiles read
    what earlier ones wrote -- and its top-left row_limit x row_limit corner lands in the canvas.  `blend`: ops.tile_blend, or a
    stand-in with its signature."""
    blend = blend or ops.tile_blend
    oys, Hout = canvas_layout([r[0].shape[2] for r in rows], row_limit)
    oxs, Wout = canvas_layout([t.shape[3] for t in rows[0]], row_limit)
    for r in rows:
        assert [t.shape[3] for t in r] == [t.shape[3] for t in rows[0]] and len({t.shape[2] for t in r}) == 1
    first = rows[0][0]
    out = torch.empty((first.shape[0], first.shape[1], Hout, Wout), dtype=first.dtype, device=first.device)
    for i, row in enumerate(rows):
        for j, tile in enumerate(row):
            blend(tile, rows[i - 1][j] if i > 0 else None, row[j - 1] if j > 0 else None, blend_extent, out, oys[i], oxs[j], row_limit)
    return out


# ---- the posterior --------------------------------------------------------------------------------------------------
class DiagonalGaussianDistribution:
    """vae.py:384-428.  `.mean` is a view of the parameters; `.logvar` (clamped), `.std` and `.var` are filled on first use by one
    launch; `sample` and `kl` are one launch (and its combine) each."""

    def __init__(self, parameters, deterministic=False):
        if parameters.dim() != 4 or parameters.shape[1] % 2:
            raise ValueError('DiagonalGaussianDistribution: parameters [N, 2C, H, W]')
        if parameters.device.type != 'cuda':
            raise RuntimeError('DiagonalGaussianDistribution ' + _NO_FALLBACK)
        if parameters.dtype != torch.float32:
            raise NotImplementedError('DiagonalGaussianDistribution runs in fp32 only')
        self.parameters = parameters
        self.deterministic = deterministic
        self.mean = parameters[:, :parameters.shape[1] // 2]
        self._stats = None

    def _fill(self):
        if self._stats is None:
            with torch.no_grad():
                s = ops.gaussian_posterior(self.parameters.detach(), logvar=True, std=not self.deterministic, var=not self.deterministic)
                if self.deterministic:                           # vae.py:392-395
                    s['std'] = s['var'] = torch.zeros_like(s['logvar'])
            self._stats = s
        return self._stats

    logvar = property(lambda self: self._fill()['logvar'])
    std = property(lambda self: self._fill()['std'])
    var = property(lambda self: self._fill()['var'])

    @torch.no_grad()
    def sample(self, generator=None, host_noise=False, scale=1.0):
        """mean + std * noise (times `scale`, rounded on its own: ddpm.py's `self.scale_factor * z`).  The noise is drawn as the
        Diffusers class draws it, on the parameters' device (a host generator draws on the host); host_noise=True is the ldm_exp
        form `torch.randn(mean.shape).to(device)` (distributions.py:43-45)."""
        from .diffusion import randn_tensor
        p = self.parameters
        shape = tuple(self.mean.shape)
        if host_noise:
            noise = torch.randn(shape, generator=generator, dtype=p.dtype).to(p.device)
        else:
            noise = randn_tensor(shape, generator=generator, device=p.device, dtype=p.dtype)
        if self.deterministic:                                   # std is zero: the mean (times scale)
            z = self.mean.contiguous()
            return ops.axpby(z, float(scale), torch.empty_like(z), 0.0) if scale != 1.0 else z.clone()
        return ops.gaussian_posterior(p.detach(), noise=noise.contiguous(), scale=scale, z=True)['z']

    @torch.no_grad()
    def kl(self, other=None):
        if other is not None:
            raise NotImplementedError('DiagonalGaussianDistribution.kl(other=...) is a training-loss term (lossconfig): not implemented')
        if self.deterministic:
            return torch.Tensor([0.0])
        return ops.gaussian_posterior(self.parameters.detach(), kl=True)['kl']

    def nll(self, sample, dims=(1, 2, 3)):
        raise NotImplementedError('DiagonalGaussianDistribution.nll is a training-loss term (lossconfig): not implemented')

    def mode(self):
        return self.mean


# ---- the model --------------------------------------------------------------------------------------------------------
_DEFAULTS = dict(in_channels=3, out_channels=3, down_block_types=('DownEncoderBlock2D',), up_block_types=('UpDecoderBlock2D',),
                 block_out_channels=(64,), layers_per_block=1, act_fn='silu', latent_channels=4, norm_num_groups=32, sample_size=32,
                 scaling_factor=0.18215)


class AutoencoderKL(FirstStage):
    """Construction order follows autoencoder_kl.py:86-111, so `state_dict()` key order matches the reference."""

    def __init__(self, norm_type='group', **kwargs):
        super().__init__()
        cfg = self.config = autoencoder_config('AutoencoderKL', _DEFAULTS, norm_type, kwargs)
        nb = len(cfg['block_out_channels'])
        G, L, boc, Z = cfg['norm_num_groups'], cfg['layers_per_block'], cfg['block_out_channels'], cfg['latent_channels']
        self.encoder = Encoder(cfg['in_channels'], 2 * Z, boc, L, G)                 # double_z
        self.decoder = Decoder(Z, cfg['out_channels'], boc, L, G)
        self.quant_conv = nn.Conv2d(2 * Z, 2 * Z, 1)
        self.post_quant_conv = nn.Conv2d(Z, Z, 1)
        self.use_slicing = False
        self.use_tiling = False
        # only relevant if tiling is enabled (autoencoder_kl.py:116-124)
        ss = cfg['sample_size']
        self.tile_sample_min_size = ss
        ss = ss[0] if isinstance(ss, (list, tuple)) else ss
        self.tile_latent_min_size = int(ss / (2 ** (nb - 1)))
        self.tile_overlap_factor = 0.25
        self._engine = None

    def _new_engine(self):
        return KLEngine(self.config)

    def enable_tiling(self, use_tiling=True):
        self.use_tiling = use_tiling

    def disable_tiling(self):
        self.enable_tiling(False)

    def enable_slicing(self):
        self.use_slicing = True

    def disable_slicing(self):
        self.use_slicing = False

    # ---- encode
    @torch.no_grad()
    def encode(self, x, return_dict=True):
        if self.use_tiling and (x.shape[-1] > self.tile_sample_min_size or x.shape[-2] > self.tile_sample_min_size):
            return self.tiled_encode(x, return_dict=return_dict)
        posterior = DiagonalGaussianDistribution(self.engine().encode(self._input(x)))
        return AutoencoderKLOutput(latent_dist=posterior) if return_dict else (posterior,)

    # ---- decode
    def _decode(self, z):
        if self.use_tiling and (z.shape[-1] > self.tile_latent_min_size or z.shape[-2] > self.tile_latent_min_size):
            return self.tiled_decode(z).sample
        return self.engine().decode(self._input(z))

    @torch.no_grad()
    def decode(self, z, return_dict=True):
        if self.use_slicing and z.shape[0] > 1:                       # one image per call (autoencoder_kl.py:187-189)
            first = self._decode(z[0:1])
            dec = ops.empty_act((z.shape[0],) + tuple(first.shape[1:]), first.device)
            ops.copy_strided(first, dec[0:1])
            for i in range(1, z.shape[0]):
                ops.copy_strided(self._decode(z[i:i + 1]), dec[i:i + 1])
        else:
            dec = self._decode(z)
        return DecoderOutput(sample=dec) if return_dict else (dec,)

    # ---- tiling
    def _tiles(self, x, tile, overlap_size, fn):
        """fn on every tile x[:, :, i : i + tile, j : j + tile] (a contiguous copy: the engine takes contiguous images), through the
        engine's micro-batching.  The results are kept as the blend loop's own buffers."""
        x = self._input(x)
        rows = []
        for i, h in tile_spans(x.shape[2], tile, overlap_size):
            rows.append([fn(x[:, :, i:i + h, j:j + w].contiguous()).contiguous() for j, w in tile_spans(x.shape[3], tile, overlap_size)])
        return rows

    @torch.no_grad()
    def tiled_encode(self, x, return_dict=True):
        """autoencoder_kl.py:210-255: tiles of tile_sample_min_size every overlap_size pixels, encoder + quant_conv on each, then one
        blend launch per tile."""
        overlap_size, blend_extent, row_limit = tile_geometry(self.tile_sample_min_size, self.tile_latent_min_size, self.tile_overlap_factor)
        eng = self.engine()
        with self.pin_weights():
            rows = self._tiles(x, self.tile_sample_min_size, overlap_size, eng.encode)
        posterior = DiagonalGaussianDistribution(blend_tiles(rows, blend_extent, row_limit))
        return AutoencoderKLOutput(latent_dist=posterior) if return_dict else (posterior,)

    @torch.no_grad()
    def tiled_decode(self, z, return_dict=True):
        """autoencoder_kl.py:257-302: latent tiles of tile_latent_min_size every overlap_size, post_quant_conv + decoder on each."""
        overlap_size, blend_extent, row_limit = tile_geometry(self.tile_latent_min_size, self.tile_sample_min_size, self.tile_overlap_factor)
        eng = self.engine()
        with self.pin_weights():
            rows = self._tiles(z, self.tile_latent_min_size, overlap_size, eng.decode)
        dec = blend_tiles(rows, blend_extent, row_limit)
        return DecoderOutput(sample=dec) if return_dict else (dec,)

    @torch.no_grad()
    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None):
        posterior = self.encode(sample).latent_dist
        z = posterior.sample(generator=generator) if sample_posterior else posterior.mode()
        dec = self.decode(z).sample
        return DecoderOutput(sample=dec) if return_dict else (dec,)


class KLEngine(VQEngine):
    """VQEngine without the quantizer: `encode` is the shared encoder pass, whose conv_out and quant_conv carry 2 * latent_channels
    here; `decode` is the shared decoder pass with the quantizer switched off."""

    def micro_batch(self, shape, decode):
        """A single image whose largest tensor (at high resolution the mid block's [T, T] attention scores) passes the reach cannot be
        split by images: refused here, before anything is launched."""
        need = self.per_image_bytes(shape, decode)
        if need > self.MAX_CALL_BYTES:
            raise ValueError('one %d x %d %s needs a tensor of %d bytes >= 2 GiB (32-bit buffer addressing): enable_tiling()'
                             % (shape[2], shape[3], 'latent' if decode else 'image', need))
        return super().micro_batch(shape, decode)

    def decode(self, z):
        """post_quant_conv + Decoder (autoencoder_kl.py:177-178)."""
        return self._batched(z, self._decode, True, quantize=False)
