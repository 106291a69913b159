"""VQModel (the VQ autoencoder of latent diffusion) with the Diffusers interface, executed by the HIP engine.

Mirrors the reference's `diffusers.models.VQModel` (vq_model.py:69-159, vae.py:38-364) for the configuration family it builds:
DownEncoderBlock2D / UpDecoderBlock2D levels, a mid block of two resnets around one single-head attention, GroupNorm eps 1e-6,
Downsample2D(padding=0), nearest x2 Upsample2D, and the legacy VectorQuantizer with beta 0.25 and no remap.  Same constructor
arguments, `.config`, `encode` / `decode` / `forward` / `quantize`, and the exact state-dict keys, every weight held by a real
nn.Conv2d / nn.GroupNorm / nn.Linear / nn.Embedding (parameter holders: all arithmetic runs in the HIP kernels through
`VQEngine`).  Forward only, fp32, no grad; there is no CPU / PyTorch fallback.
"""
import torch
import torch.nn as nn

from . import ops
from .engine import UNetEngine, _SPEC1, _SPEC3
from .model_base import BaseOutput, DiffusersModel, FrozenConfig, _Block
from .unet import Attention, Downsample2D, ResnetBlock2D, Upsample2D

_SPEC_DOWN = ops.ConvSpec(3, 2, 0, 0)        # Downsample2D(padding=0): F.pad(0, 1, 0, 1) + stride-2 valid conv (resnet.py:196-201)
BETA = 0.25                                 # vq_model.py:102
_Output = BaseOutput                        # the name whole-module pickles and earlier callers know


class VQEncoderOutput(BaseOutput):
    """vq_model.py:27-35: `.latents`."""


class DecoderOutput(BaseOutput):
    """vae.py:26-35: `.sample`."""


# ---- parameter holders, named and ordered as in Diffusers -------------------------------------------------------
def _resnet(in_channels, out_channels, groups):
    """unet.ResnetBlock2D without a time embedding, GroupNorm eps 1e-6."""
    return ResnetBlock2D(in_channels, out_channels, None, groups, 1e-6)


def _mid_block(channels, groups):
    """UNetMidBlock2D (unet_2d_blocks.py:392-470) as Encoder / Decoder build it: one head of `channels`, rescale 1."""
    mid = _Block()
    mid.attentions = nn.ModuleList([Attention(channels, 1, channels, groups, 1e-6, 1.0)])
    mid.resnets = nn.ModuleList([_resnet(channels, channels, groups), _resnet(channels, channels, groups)])
    return mid


class Encoder(nn.Module):
    def __init__(self, in_channels, out_channels, block_out_channels, layers_per_block, groups):
        super().__init__()
        boc = block_out_channels
        self.conv_in = nn.Conv2d(in_channels, boc[0], 3, 1, 1)
        self.down_blocks = nn.ModuleList([])
        out_c = boc[0]
        for i in range(len(boc)):
            in_c, out_c = out_c, boc[i]
            blk = _Block()
            blk.resnets = nn.ModuleList([_resnet(in_c if j == 0 else out_c, out_c, groups) for j in range(layers_per_block)])
            blk.downsamplers = nn.ModuleList([Downsample2D(out_c, 0)]) if i != len(boc) - 1 else None
            self.down_blocks.append(blk)
        self.mid_block = _mid_block(boc[-1], groups)
        self.conv_norm_out = nn.GroupNorm(groups, boc[-1], eps=1e-6)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(boc[-1], out_channels, 3, padding=1)


class Decoder(nn.Module):
    def __init__(self, in_channels, out_channels, block_out_channels, layers_per_block, groups):
        super().__init__()
        boc = block_out_channels
        self.conv_in = nn.Conv2d(in_channels, boc[-1], 3, 1, 1)
        self.up_blocks = nn.ModuleList([])            # registered before mid_block, as vae.py:173-177 does
        rev = list(reversed(boc))
        out_c = rev[0]
        for i in range(len(rev)):
            prev, out_c = out_c, rev[i]
            blk = _Block()
            blk.resnets = nn.ModuleList([_resnet(prev if j == 0 else out_c, out_c, groups) for j in range(layers_per_block + 1)])
            blk.upsamplers = nn.ModuleList([Upsample2D(out_c)]) if i != len(rev) - 1 else None
            self.up_blocks.append(blk)
        self.mid_block = _mid_block(boc[-1], groups)
        self.conv_norm_out = nn.GroupNorm(groups, boc[0], eps=1e-6)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(boc[0], out_channels, 3, padding=1)


class VectorQuantizer(nn.Module):
    def __init__(self, n_e, vq_embed_dim, beta=BETA):
        super().__init__()
        self.n_e, self.vq_embed_dim, self.beta, self.legacy, self.remap, self.sane_index_shape = n_e, vq_embed_dim, beta, True, None, False
        self.embedding = nn.Embedding(n_e, vq_embed_dim)
        with torch.no_grad():
            self.embedding.weight.uniform_(-1.0 / n_e, 1.0 / n_e)          # vae.py:289

    @torch.no_grad()
    def forward(self, z):
        """vae.py:332-364 on the HIP quantizer: (z_q, loss, (None, None, indices [N * H * W] int64 in (n, h, w) order))."""
        w = self.embedding.weight
        if w.device.type != 'cuda':
            raise RuntimeError('VectorQuantizer runs on the MI355X HIP kernels only (no CPU / PyTorch fallback)')
        zq, loss, idx = ops.vq_quantize(z.detach().to(torch.float32).contiguous(), w.detach(), beta=self.beta)
        return zq, loss, (None, None, idx)


_DEFAULTS = dict(in_channels=3, out_channels=3, down_block_types=('DownEncoderBlock2D',), up_block_types=('UpDecoderBlock2D',),
                 block_out_channels=(64,), layers_per_block=1, act_fn='silu', latent_channels=3, sample_size=32,
                 num_vq_embeddings=256, norm_num_groups=32, vq_embed_dim=None, scaling_factor=0.18215)


def autoencoder_config(name, defaults, norm_type, kwargs):
    """The constructor checks VQModel and AutoencoderKL share, worded with the class's `name`: the FrozenConfig of `defaults`
    updated by `kwargs`, or the refusal."""
    cfg = dict(defaults)
    unknown = set(kwargs) - set(cfg)
    if unknown:
        raise TypeError('unexpected %s arguments: %s' % (name, sorted(unknown)))
    cfg.update(kwargs)
    for k in ('down_block_types', 'up_block_types', 'block_out_channels'):
        cfg[k] = tuple(cfg[k])
    if norm_type != 'group':
        raise NotImplementedError('%s: norm_type=%r (only the GroupNorm decoder is implemented)' % (name, norm_type))
    if cfg['act_fn'] not in ('silu', 'swish'):
        raise NotImplementedError('%s: act_fn=%r (only silu)' % (name, cfg['act_fn']))
    nb = len(cfg['block_out_channels'])
    if len(cfg['down_block_types']) != nb or len(cfg['up_block_types']) != nb:
        raise ValueError('down_block_types, up_block_types and block_out_channels must have equal lengths')
    if set(cfg['down_block_types']) != {'DownEncoderBlock2D'} or set(cfg['up_block_types']) != {'UpDecoderBlock2D'}:
        raise NotImplementedError('%s: only DownEncoderBlock2D / UpDecoderBlock2D levels are implemented' % name)
    return FrozenConfig(cfg)


class FirstStage(DiffusersModel):
    """What VQModel and AutoencoderKL share besides their holders: fp32 only, `device` / `dtype` read from quant_conv."""

    _fp32_only = True

    def _anchor(self):
        return self.quant_conv.weight

    @staticmethod
    def _input(x):
        return x.detach().to(torch.float32).contiguous()


class VQModel(FirstStage):
    """Construction order follows vq_model.py:86-115, so `state_dict()` key order matches the reference."""

    def __init__(self, norm_type='group', remap=None, **kwargs):
        super().__init__()
        cfg = autoencoder_config('VQModel', _DEFAULTS, norm_type, kwargs)
        if remap is not None:
            raise NotImplementedError('VQModel: a remapped codebook (remap=...) is not implemented')
        D = cfg['vq_embed_dim'] if cfg['vq_embed_dim'] is not None else cfg['latent_channels']
        if D > ops.VQ_MAX_DIM:
            raise NotImplementedError('VQModel: codebook vectors of %d channels (the HIP quantizer takes at most %d)'
                                      % (D, ops.VQ_MAX_DIM))
        self.config = cfg
        G, L, boc = cfg['norm_num_groups'], cfg['layers_per_block'], cfg['block_out_channels']
        self.encoder = Encoder(cfg['in_channels'], cfg['latent_channels'], boc, L, G)
        self.quant_conv = nn.Conv2d(cfg['latent_channels'], D, 1)
        self.quantize = VectorQuantizer(cfg['num_vq_embeddings'], D)
        self.post_quant_conv = nn.Conv2d(D, cfg['latent_channels'], 1)
        self.decoder = Decoder(cfg['latent_channels'], cfg['out_channels'], boc, L, G)
        self._engine = None

    def _new_engine(self):
        return VQEngine(self.config)

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        h = self.engine().encode(self._input(x))
        return VQEncoderOutput(latents=h) if return_dict else (h,)

    @torch.no_grad()
    def decode(self, h, force_not_quantize=False, return_dict=True):
        dec = self.engine().decode(self._input(h), quantize=not force_not_quantize)
        return DecoderOutput(sample=dec) if return_dict else (dec,)

    @torch.no_grad()
    def forward(self, sample, return_dict=True):
        eng = self.engine()
        dec = eng.decode(eng.encode(self._input(sample)), quantize=True)
        return DecoderOutput(sample=dec) if return_dict else (dec,)


class VQEngine(UNetEngine):
    """Forward-only VQModel on the UNet engine's layers: resnets without a time embedding, the single-head mid-block attention,
    stride-2 valid downsampling convolutions, sub-pixel upsample convolutions, and the HIP quantizer (csrc/vq.hip)."""

    # The decoder's mid-block attention at 64 x 64 latents (T = 4096 tokens, d = 512): the one-kernel form (csrc/attention.hip, no
    # [T, T] scores) or the three launches (QK^T, softmax, PV^T; 64 MB of scores per image).  Chosen for this path only by
    # tools/bench_vq.py; the UNets keep ops.FUSED_ATTN's rule.
    FUSED_MID_ATTN = False

    def __init__(self, cfg):
        super().__init__(dict(cfg, norm_eps=1e-6, attention_head_dim=None))
        self.fused_mid_attn = self.FUSED_MID_ATTN

    def _begin(self):
        self._nograd = True                                  # nothing is kept for a backward: F(4, 3) where it qualifies
        self._wino_gen = getattr(self, '_wino_gen', 0) + 1

    def _res(self, pre, x):
        return self.resnet_fwd(pre, x, None, None, 1.0, None)

    def _mid(self, pre, x):
        C = x.shape[1]
        x = self._res(pre + '.resnets.0', x)
        x = self.attn_fwd(pre + '.attentions.0', x, float(C) ** -0.5, 1.0, None, 1, fused_attn=self.fused_mid_attn)
        return self._res(pre + '.resnets.1', x)

    def _head(self, pre, x):
        P = self.P
        n, _ = ops.groupnorm_fwd(x, None, P[pre + '.conv_norm_out.weight'], P[pre + '.conv_norm_out.bias'],
                                 self.cfg['norm_num_groups'], 1e-6, True)
        return self._conv(pre + '.conv_out', n, None, _SPEC3)

    # The engine's kernels address an activation through buffer descriptors with 32-bit offsets: no single call may see 2 GiB
    # (ops._extent_bytes).  VQ-f4's largest tensor is 64 MiB per image (256 channels at 256 x 256 after the decoder's second
    # upsample; the mid-block scores at T = 4096 are as large), so encode / decode run the batch in micro-batches of at most
    # MAX_CALL_BYTES // (largest per-image tensor) images: 31 for the VQ-f4 decode, where a single pass stopped at 32.
    MAX_CALL_BYTES = ops._MAX_BYTES - 1

    def per_image_bytes(self, shape, decode):
        """Largest tensor of one image in an encode (input [N, Cin, H, W]) or decode (latents [N, D, h, w]) pass, in bytes: every
        level's activations at its widest channel count (the first convolution of a level reads the previous level's width), and
        the mid block's [T, T] attention scores."""
        cfg = self.cfg
        boc, nb = list(cfg['block_out_channels']), len(cfg['block_out_channels'])
        H, W = int(shape[2]), int(shape[3])
        if decode:
            rev = boc[::-1]
            sizes = [max(int(shape[1]), rev[0]) * H * W, (H * W) ** 2]
            for i in range(nb):
                hw = (H << i) * (W << i)
                sizes.append(max(rev[i], rev[i - 1] if i else 0, cfg['out_channels'] if i == nb - 1 else 0) * hw)
        else:
            sizes = [max(int(shape[1]), boc[0]) * H * W]
            h, w = H, W
            for i in range(nb):
                sizes.append(max(boc[i], boc[i - 1] if i else 0) * h * w)
                if i != nb - 1:
                    h, w = (h + 1) // 2, (w + 1) // 2
            sizes.append((h * w) ** 2)
        return 4 * max(sizes)

    def micro_batch(self, shape, decode):
        return max(1, self.MAX_CALL_BYTES // self.per_image_bytes(shape, decode))

    def _batched(self, x, fn, decode, **kw):
        m = self.micro_batch(x.shape, decode)
        N = x.shape[0]
        if N <= m:
            return fn(x, **kw)
        out = None
        for i in range(0, N, m):
            y = fn(x[i:i + m], **kw)
            if out is None:
                out = ops.empty_act((N,) + tuple(y.shape[1:]), y.device)
            ops.copy_strided(y, out[i:i + y.shape[0]])
        return out

    def encode(self, x):
        """Encoder + quant_conv (vq_model.py:117-124): x [N, Cin, H, W] -> latents [N, D, H / f, W / f]."""
        return self._batched(x, self._encode, False)

    def decode(self, z, quantize=True):
        """quantize (unless force_not_quantize) + post_quant_conv + Decoder (vq_model.py:126-139)."""
        return self._batched(z, self._decode, True, quantize=quantize)

    def _encode(self, x):
        self._begin()
        nb, L = len(self.cfg['block_out_channels']), self.cfg['layers_per_block']
        h = self._conv('encoder.conv_in', x, None, _SPEC3)
        for i in range(nb):
            for j in range(L):
                h = self._res('encoder.down_blocks.%d.resnets.%d' % (i, j), h)
            if i != nb - 1:
                h = self._conv('encoder.down_blocks.%d.downsamplers.0.conv' % i, h, None, _SPEC_DOWN)
        h = self._mid('encoder.mid_block', h)
        h = self._head('encoder', h)
        return self._conv('quant_conv', h, None, _SPEC1)

    def _decode(self, z, quantize=True):
        self._begin()
        if quantize:
            z, _, _ = ops.vq_quantize(z, self.P['quantize.embedding.weight'], want_indices=False, want_loss=False)
        nb, L = len(self.cfg['block_out_channels']), self.cfg['layers_per_block']
        h = self._conv('post_quant_conv', z, None, _SPEC1)
        h = self._conv('decoder.conv_in', h, None, _SPEC3)
        h = self._mid('decoder.mid_block', h)
        for i in range(nb):
            for j in range(L + 1):
                h = self._res('decoder.up_blocks.%d.resnets.%d' % (i, j), h)
            if i != nb - 1:
                h = self._ups_conv_fwd('decoder.up_blocks.%d.upsamplers.0.conv' % i, h)
        return self._head('decoder', h)
