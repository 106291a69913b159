"""Pruned-model checkpoints (reference: ddpm_prune.py:132-135, ddpm_train.py:289-300,484-498,
ddpm_exp/torch_pruning/dependency.py:278-293).

The reference hands a pruned UNet to the finetune / sampling scripts as a whole-module pickle (`torch.save(model,
'unet_pruned.pth')`): the module *is* the record of the pruned shapes.  Here the same hand-over works three ways:

* `torch.save(model, path)` / `torch.load(path)` -- the whole-module pickle of this package's UNet2DModel / UNetModel
  (the HIP engine, its packed operands and its streams are dropped from the pickle and rebuilt on first use);
* `save_pruned(model, directory)` / `load_pruned(directory)` -- pickle-free: weights as safetensors plus a JSON with the
  constructor config and the replayable `pruning_history` ([root module name, is_out_channel_pruning, indices] per
  group, exactly the reference's DependencyGraph.pruning_history() format); loading builds the un-pruned module, replays
  the history (structure only) and loads the weights strictly;
* `adopt_state_dict(model, state_dict)` -- shape-aware load of a pruned state dict that comes WITHOUT a history (e.g. the
  `state_dict()` of the reference's own `unet_pruned.pth`, whose keys are identical): every Conv2d / Linear / GroupNorm /
  LayerNorm takes the shapes found in the checkpoint, then the coupling graph is checked for consistency.

Host-side only: tensors are plain torch tensors on any device; nothing here touches the HIP kernels."""
import functools
import importlib
import json
import os

import torch
import torch.nn as nn

from . import pruning

FORMAT_VERSION = 1
WEIGHTS, META = 'unet_pruned.safetensors', 'unet_pruned.json'


def _config_dict(model):
    cfg = dict(model.config)
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}


# class name -> (module that defines it, imported on first use; the folder a Diffusers pipeline directory keeps it in; whether an
# LDMPipeline takes it as its first stage).  UNetModel is the CompVis class: it has no Diffusers directory form.
MODELS = {'UNet2DModel': ('unet', 'unet', False), 'VQModel': ('vq', 'vqvae', True), 'AutoencoderKL': ('vae', 'vae', True),
          'UNetModel': ('ldm', None, False)}
_FIRST_STAGES = tuple(n for n, row in MODELS.items() if row[2])


def _build(kind, cfg):
    return getattr(importlib.import_module('.' + MODELS[kind][0], __package__), kind)(**cfg)


def save_pruned(model, directory, pruning_history):
    """Write `unet_pruned.safetensors` + `unet_pruned.json` into `directory`.  `pruning_history`: the list returned by
    `pruner.pruning_history()` (or `pruner.DG.pruning_history()`) after the groups were pruned."""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    sd = {k: v.detach().to('cpu').contiguous() for k, v in model.state_dict().items()}
    save_file(sd, os.path.join(directory, WEIGHTS))
    meta = dict(format_version=FORMAT_VERSION, model_class=type(model).__name__, config=_config_dict(model),
                pruning_history=[[n, bool(o), [int(i) for i in ix]] for n, o, ix in pruning_history],
                shapes={k: list(v.shape) for k, v in sd.items()}, num_parameters=int(sum(v.numel() for v in sd.values())))
    if getattr(model, 'attention_scale_from_width', False):          # an original-DDPM model: its attention rescales with the prune
        meta['attention_scale_from_width'] = True
    with open(os.path.join(directory, META), 'w') as f:
        json.dump(meta, f)
    return meta


def load_pruned(directory, device=None):
    """Rebuild the pruned module from `save_pruned` output: construct, replay the pruning history, load the weights."""
    from safetensors.torch import load_file
    with open(os.path.join(directory, META)) as f:
        meta = json.load(f)
    if meta.get('format_version') != FORMAT_VERSION:
        raise ValueError('unsupported pruned-checkpoint format %r' % (meta.get('format_version'),))
    model = _build(meta['model_class'], meta['config'])
    if meta.get('attention_scale_from_width'):
        model.attention_scale_from_width = True
    pruning.DependencyGraph(model).load_pruning_history(meta['pruning_history'])
    pruning.fix_static_attributes(model)
    sd = load_file(os.path.join(directory, WEIGHTS))
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    if got != meta['shapes']:
        bad = [k for k in meta['shapes'] if got.get(k) != meta['shapes'][k]][:5]
        raise ValueError('replayed pruning history does not reproduce the checkpoint shapes (first mismatches: %s)' % bad)
    model.load_state_dict(sd, strict=True)
    model.eval()
    return model.to(device) if device is not None else model


def adopt_state_dict(model, state_dict):
    """Give every prunable layer of the UN-pruned `model` the shapes found in `state_dict` (same keys), load the weights
    and verify that the result is a consistent pruned network (every coupled member agrees on its channel count)."""
    mods = dict(model.named_modules())
    for key, w in state_dict.items():
        name, _, attr = key.rpartition('.')
        m = mods.get(name)
        if m is None or attr not in ('weight', 'bias'):
            raise KeyError('unexpected key in pruned state dict: %s' % key)
        old = getattr(m, attr)
        if old is None or tuple(old.shape) == tuple(w.shape):
            continue
        setattr(m, attr, nn.Parameter(torch.empty(tuple(w.shape), dtype=old.dtype, device=old.device)))
    for m in mods.values():
        if isinstance(m, nn.Conv2d):
            m.out_channels, m.in_channels = m.weight.shape[0], m.weight.shape[1]
        elif isinstance(m, nn.Linear):
            m.out_features, m.in_features = m.weight.shape
        elif isinstance(m, nn.GroupNorm):
            m.num_channels = m.weight.shape[0]
        elif isinstance(m, nn.LayerNorm):
            m.normalized_shape = (m.weight.shape[0],)
    model.load_state_dict(state_dict, strict=True)
    pruning.fix_static_attributes(model)
    # consistency: walking every coupling group with all of its root's channels must tile each member dimension exactly
    # (a producer narrower or wider than its consumers -- or a concat whose parts do not add up -- leaves holes / overflow)
    dg = pruning.DependencyGraph(model)
    covered = {}
    for group in dg.get_all_groups(ignored_layers=()):
        for dep, idxs in group:
            covered.setdefault((dep.target.name, 'in' if dep.kind == 'in' else 'out'), set()).update(idxs)
    for (name, side), got in covered.items():
        m = dg.name2module[name]
        dim = pruning._in_channels(m) if side == 'in' else pruning._out_channels(m)
        if got != set(range(dim)):
            raise ValueError('inconsistent pruned shapes at %s (%s channels: %d, coupling graph covers %d)'
                             % (name, side, dim, len(got)))
    return model


# --------------------------------------------------------------------------------------------------------
# Original-DDPM ("ddpm_exp") checkpoints <-> Diffusers UNet2DModel keys
# --------------------------------------------------------------------------------------------------------
# The reference's second code path (ddpm_exp/prune.py, finetune_simple.py, runners/diffusion.py) works on the original
# DDPM `Model` class (ddpm_exp/models/diffusion.py:191-341), whose checkpoints (`ckpt.pth`, the `pretrained/` download)
# name the same tensors differently.  The key correspondence below restates the layout that class builds
# (models/diffusion.py:218-305) against unet_2d.py:84-217; the reference's own converter for it is
# tools/convert_ddpm_original_checkpoint_to_diffusers_cifar10.py:100-240.  Differences in content, not only in names:
# attention projections are 1x1 Conv2d there ([C, C, 1, 1]) and Linear here ([C, C]); `up.{i}` is indexed by resolution
# level (0 = full resolution), `up_blocks.{j}` by execution order (0 = lowest resolution).
_RES_O2D = (('norm1', 'norm1'), ('conv1', 'conv1'), ('temb_proj', 'time_emb_proj'), ('norm2', 'norm2'), ('conv2', 'conv2'),
            ('nin_shortcut', 'conv_shortcut'))
_ATT_O2D = (('norm', 'group_norm'), ('q', 'to_q'), ('k', 'to_k'), ('v', 'to_v'), ('proj_out', 'to_out.0'))


def ddpm_original_key_map(keys):
    """{original key: diffusers key} for the parameter names of a ddpm_exp `Model` state dict."""
    keys = list(keys)
    levels = 1 + max(int(k.split('.')[1]) for k in keys if k.startswith('down.'))
    fixed = {'temb.dense.0': 'time_embedding.linear_1', 'temb.dense.1': 'time_embedding.linear_2', 'conv_in': 'conv_in',
             'norm_out': 'conv_norm_out', 'conv_out': 'conv_out', 'mid.block_1': 'mid_block.resnets.0',
             'mid.block_2': 'mid_block.resnets.1', 'mid.attn_1': 'mid_block.attentions.0'}
    out = {}
    for k in keys:
        stem, _, leaf = k.rpartition('.')                      # leaf = weight | bias
        parts = stem.split('.')
        new = None
        if parts[0] in ('down', 'up'):
            i = int(parts[1])
            blk = ('down_blocks.%d' % i) if parts[0] == 'down' else ('up_blocks.%d' % (levels - 1 - i))
            if parts[2] == 'block':
                new = '%s.resnets.%s.%s' % (blk, parts[3], dict(_RES_O2D)[parts[4]])
            elif parts[2] == 'attn':
                new = '%s.attentions.%s.%s' % (blk, parts[3], dict(_ATT_O2D)[parts[4]])
            elif parts[2] == 'downsample':
                new = blk + '.downsamplers.0.conv'
            elif parts[2] == 'upsample':
                new = blk + '.upsamplers.0.conv'
        else:
            for old, rep in fixed.items():
                if stem == old:
                    new = rep
                elif stem.startswith(old + '.'):
                    sub = stem[len(old) + 1:]
                    new = rep + '.' + (dict(_ATT_O2D)[sub] if 'attn' in old else dict(_RES_O2D)[sub])
        if new is None:
            raise KeyError('not a ddpm_exp Model parameter: %s' % k)
        out[k] = new + '.' + leaf
    return out


def convert_ddpm_original(state_dict):
    """Original-DDPM `Model` state dict -> state dict with this package's / Diffusers' UNet2DModel keys."""
    kmap = ddpm_original_key_map(state_dict.keys())
    out = {}
    for k, v in state_dict.items():
        nk = kmap[k]
        if '.attentions.' in nk and not nk.rsplit('.', 2)[-2].startswith('group_norm') and v.dim() == 4:
            v = v.reshape(v.shape[0], v.shape[1])              # 1x1 Conv2d -> Linear
        out[nk] = v
    return out


def convert_to_ddpm_original(state_dict):
    """Inverse of convert_ddpm_original (to hand a pruned / finetuned model back to the ddpm_exp scripts)."""
    levels = 1 + max(int(k.split('.')[1]) for k in state_dict if k.startswith('down_blocks.'))
    res_d2o = {b: a for a, b in _RES_O2D}
    att_d2o = {b: a for a, b in _ATT_O2D}
    fixed = {'time_embedding.linear_1': 'temb.dense.0', 'time_embedding.linear_2': 'temb.dense.1', 'conv_in': 'conv_in',
             'conv_norm_out': 'norm_out', 'conv_out': 'conv_out'}
    out = {}
    for k, v in state_dict.items():
        stem, _, leaf = k.rpartition('.')
        p = stem.split('.')
        if stem in fixed:
            new = fixed[stem]
        elif p[0] == 'mid_block':
            new = ('mid.block_%d.%s' % (int(p[2]) + 1, res_d2o[p[3]])) if p[1] == 'resnets' else \
                  ('mid.attn_1.' + att_d2o['.'.join(p[3:])])
        elif p[0] in ('down_blocks', 'up_blocks'):
            i = int(p[1])
            blk = ('down.%d' % i) if p[0] == 'down_blocks' else ('up.%d' % (levels - 1 - i))
            if p[2] == 'resnets':
                new = '%s.block.%s.%s' % (blk, p[3], res_d2o[p[4]])
            elif p[2] == 'attentions':
                new = '%s.attn.%s.%s' % (blk, p[3], att_d2o['.'.join(p[4:])])
            elif p[2] == 'downsamplers':
                new = blk + '.downsample.conv'
            elif p[2] == 'upsamplers':
                new = blk + '.upsample.conv'
            else:
                raise KeyError(k)
        else:
            raise KeyError(k)
        if ('.attn' in new) and not new.endswith('.norm') and v.dim() == 2:
            v = v.reshape(v.shape[0], v.shape[1], 1, 1)        # Linear -> 1x1 Conv2d
        out[new + '.' + leaf] = v
    return out


def unet2d_config_from_ddpm_original(ch, ch_mult, num_res_blocks, attn_resolutions, image_size, in_channels=3, out_ch=3):
    """UNet2DModel kwargs equivalent to a ddpm_exp `Model` config (ddpm_exp/configs/*.yml: model.ch, ch_mult,
    num_res_blocks, attn_resolutions; data.image_size)."""
    res, down, up = image_size, [], []
    for lvl in range(len(ch_mult)):
        down.append('AttnDownBlock2D' if res in attn_resolutions else 'DownBlock2D')
        up.insert(0, 'AttnUpBlock2D' if res in attn_resolutions else 'UpBlock2D')
        if lvl != len(ch_mult) - 1:
            res //= 2
    return dict(sample_size=image_size, in_channels=in_channels, out_channels=out_ch, layers_per_block=num_res_blocks,
                block_out_channels=tuple(ch * m for m in ch_mult), down_block_types=tuple(down), up_block_types=tuple(up),
                norm_num_groups=32, norm_eps=1e-6, downsample_padding=0, flip_sin_to_cos=False, freq_shift=1,
                attention_head_dim=None, act_fn='silu')


# --------------------------------------------------------------------------------------------------------
# Diffusers pipeline directories (ddpm_prune.py:50 DDPMPipeline.from_pretrained, :131 pipeline.save_pretrained;
# ddpm_train.py:297-306,494-498; ddpm_sample.py:54-62)
#   <dir>/model_index.json                         {"_class_name": ..., "scheduler": ["diffusers", cls], "unet": [...]}
#   <dir>/unet/config.json                         constructor kwargs (+ "_class_name", "_diffusers_version")
#   <dir>/unet/diffusion_pytorch_model.bin|.safetensors
#   <dir>/scheduler/scheduler_config.json
# Layout pinned by tests/golden/pretrained_micro/ (written by the vendored diffusers 0.17.0.dev0).
# --------------------------------------------------------------------------------------------------------
DIFFUSERS_VERSION = '0.17.0.dev0'
_UNET_WEIGHTS = ('diffusion_pytorch_model.safetensors', 'diffusion_pytorch_model.bin')


def _read_json(path):
    with open(path) as f:
        return json.load(f)


def _write_json(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(obj, f, indent=2, sort_keys=True)
        f.write('\n')


_DEPRECATED_ATTN = (('query', 'to_q'), ('key', 'to_k'), ('value', 'to_v'), ('proj_attn', 'to_out.0'))


def convert_deprecated_attention_keys(state_dict):
    """modeling_utils.py:809-851: older checkpoints name the attention projections of `...attentions.<j>` query / key / value /
    proj_attn; they are to_q / to_k / to_v / to_out.0 now.  A state dict without those names is returned as it is."""
    import re
    pat = re.compile(r'^(.*\.attentions\.\d+)\.(query|key|value|proj_attn)\.(weight|bias)$')
    if not any(pat.match(k) for k in state_dict):
        return state_dict
    out = type(state_dict)() if isinstance(state_dict, dict) else {}
    for k, v in state_dict.items():
        m = pat.match(k)
        out[('%s.%s.%s' % (m.group(1), dict(_DEPRECATED_ATTN)[m.group(2)], m.group(3))) if m else k] = v
    return out


def _load_weights(d):
    for name in _UNET_WEIGHTS:
        p = os.path.join(d, name)
        if os.path.exists(p):
            if name.endswith('.safetensors'):
                from safetensors.torch import load_file
                return load_file(p)
            return torch.load(p, map_location='cpu', weights_only=True)
    raise FileNotFoundError('no %s in %s' % (' / '.join(_UNET_WEIGHTS), d))


def _a(name):                               # 'a VQModel', 'an AutoencoderKL'
    return ('an ' if name[0] == 'A' else 'a ') + name


def load_model(class_name, directory, subfolder=None):
    """<Class>.from_pretrained: `directory` (or its `subfolder`, or the class's own pipeline folder in it) holds config.json + the
    weight file; deprecated attention names are converted as modeling_utils.py:809-851 does.  A config.json that names another
    class is refused."""
    d = os.path.join(directory, subfolder) if subfolder else directory
    folder = MODELS[class_name][1]
    if not os.path.exists(os.path.join(d, 'config.json')) and os.path.exists(os.path.join(d, folder, 'config.json')):
        d = os.path.join(d, folder)
    raw = _read_json(os.path.join(d, 'config.json'))
    if raw.get('_class_name', class_name) != class_name:
        raise ValueError('%s holds %s, not %s' % (d, _a(raw['_class_name']), _a(class_name)))
    model = _build(class_name, {k: v for k, v in raw.items() if not k.startswith('_')})
    model.load_state_dict(convert_deprecated_attention_keys(_load_weights(d)), strict=True)
    return model.eval()


def save_model(model, directory, safe_serialization=False):
    """<Class>.save_pretrained layout: config.json + diffusion_pytorch_model.bin (the vendored diffusers writes the .bin pickle of
    the state dict by default), or .safetensors."""
    os.makedirs(directory, exist_ok=True)
    cfg = dict(_config_dict(model), _class_name=type(model).__name__, _diffusers_version=DIFFUSERS_VERSION)
    _write_json(os.path.join(directory, 'config.json'), cfg)
    sd = {k: v.detach().to('cpu').contiguous() for k, v in model.state_dict().items()}
    if safe_serialization:
        from safetensors.torch import save_file
        save_file(sd, os.path.join(directory, _UNET_WEIGHTS[0]))
    else:
        torch.save(sd, os.path.join(directory, _UNET_WEIGHTS[1]))


load_unet = functools.partial(load_model, 'UNet2DModel')
load_vq = functools.partial(load_model, 'VQModel')
load_vae = functools.partial(load_model, 'AutoencoderKL')
save_unet = save_vq = save_vae = save_model


def load_scheduler(cls, directory, subfolder=None):
    d = os.path.join(directory, subfolder) if subfolder else directory
    if not os.path.exists(os.path.join(d, 'scheduler_config.json')) and os.path.exists(os.path.join(d, 'scheduler')):
        d = os.path.join(d, 'scheduler')
    cfg = {k: v for k, v in _read_json(os.path.join(d, 'scheduler_config.json')).items() if not k.startswith('_')}
    if cfg.get('trained_betas') is not None:
        raise NotImplementedError('trained_betas schedulers are not on the hot path')
    # `thresholding` is the class's to take or refuse: DDPMScheduler and DDIMScheduler carry it, the multistep solvers raise
    import inspect
    accepted = set(inspect.signature(cls.__init__).parameters) - {'self'}
    return cls(**{k: v for k, v in cfg.items() if k in accepted})


def save_scheduler(scheduler, directory):
    cfg = {k: v for k, v in vars(scheduler.config).items()}
    cfg.update(_class_name=type(scheduler).__name__, _diffusers_version=DIFFUSERS_VERSION)
    _write_json(os.path.join(directory, 'scheduler_config.json'), cfg)


def load_pipeline(cls, directory):
    from . import diffusion
    index = _read_json(os.path.join(directory, 'model_index.json'))
    sched_name = index.get('scheduler', [None, 'DDPMScheduler'])[1]
    sched_cls = getattr(diffusion, sched_name, None)
    if sched_cls is None:
        raise NotImplementedError('scheduler class %s' % sched_name)
    parts = dict(unet=load_unet(directory, 'unet'), scheduler=load_scheduler(sched_cls, directory, 'scheduler'))
    if 'vqvae' in index:                                 # LDMPipeline (pipeline_latent_diffusion_uncond.py)
        name = index['vqvae'][1]                         # the component's own class: VQModel, or AutoencoderKL
        if name not in _FIRST_STAGES:
            raise NotImplementedError('first-stage class %s' % name)
        parts['vqvae'] = load_model(name, directory, 'vqvae')
    return cls(**parts)


def save_pipeline(pipeline, directory, safe_serialization=False):
    index = dict(_class_name=type(pipeline).__name__, _diffusers_version=DIFFUSERS_VERSION,
                 scheduler=['diffusers', type(pipeline.scheduler).__name__], unet=['diffusers', 'UNet2DModel'])
    if getattr(pipeline, 'vqvae', None) is not None:
        name = type(pipeline.vqvae).__name__
        index['vqvae'] = ['diffusers', name]
        save_model(pipeline.vqvae, os.path.join(directory, 'vqvae'), safe_serialization)
    _write_json(os.path.join(directory, 'model_index.json'), index)
    save_unet(pipeline.unet, os.path.join(directory, 'unet'), safe_serialization)
    save_scheduler(pipeline.scheduler, os.path.join(directory, 'scheduler'))


# --------------------------------------------------------------------------------------------------------
# ldm_exp first stage (ldm/modules/diffusionmodules/model.py Encoder / Decoder, ldm/models/autoencoder.py VQModel) <-> VQModel
# --------------------------------------------------------------------------------------------------------
# `down.{i}` / `up.{i}` are indexed by resolution level in both Encoder and Decoder (0 = full resolution); Diffusers' decoder
# `up_blocks.{j}` by execution order (0 = lowest resolution).  The attention projections are 1x1 Conv2d there, Linear here.
_RES_L2D = (('norm1', 'norm1'), ('conv1', 'conv1'), ('norm2', 'norm2'), ('conv2', 'conv2'), ('nin_shortcut', 'conv_shortcut'))
_ATT_L2D = (('norm', 'group_norm'), ('q', 'to_q'), ('k', 'to_k'), ('v', 'to_v'), ('proj_out', 'to_out.0'))


def ldm_first_stage_key(key, up_levels):
    """Diffusers VQModel key of one ldm_exp first-stage key (without the `first_stage_model.` prefix)."""
    stem, _, leaf = key.rpartition('.')
    p = stem.split('.')
    top = {'quant_conv': 'quant_conv', 'post_quant_conv': 'post_quant_conv', 'quantize.embedding': 'quantize.embedding'}
    new = None
    if stem in top:
        new = top[stem]
    elif p[0] in ('encoder', 'decoder') and len(p) >= 2:
        side = p[0]
        rest = p[1:]
        if rest[0] in ('conv_in', 'conv_out') and len(rest) == 1:
            new = '%s.%s' % (side, rest[0])
        elif rest == ['norm_out']:
            new = side + '.conv_norm_out'
        elif rest[0] == 'mid' and len(rest) >= 3:
            if rest[1] in ('block_1', 'block_2'):
                new = '%s.mid_block.resnets.%d.%s' % (side, int(rest[1][-1]) - 1, dict(_RES_L2D)[rest[2]])
            elif rest[1] == 'attn_1':
                new = '%s.mid_block.attentions.0.%s' % (side, dict(_ATT_L2D)[rest[2]])
        elif rest[0] in ('down', 'up') and len(rest) >= 3:
            i = int(rest[1])
            blk = ('down_blocks.%d' % i) if rest[0] == 'down' else ('up_blocks.%d' % (up_levels - 1 - i))
            if rest[2] == 'block' and len(rest) == 5:
                new = '%s.%s.resnets.%s.%s' % (side, blk, rest[3], dict(_RES_L2D)[rest[4]])
            elif rest[2] == 'downsample' and rest[3:] == ['conv']:
                new = '%s.%s.downsamplers.0.conv' % (side, blk)
            elif rest[2] == 'upsample' and rest[3:] == ['conv']:
                new = '%s.%s.upsamplers.0.conv' % (side, blk)
    if new is None:
        raise KeyError('not an ldm_exp VQ first-stage parameter: %s' % key)
    return new + '.' + leaf


# training-only state of a standalone ldm_exp VQModel checkpoint (autoencoder.py:36-55): the loss module (discriminator, LPIPS),
# the LitEma copy of the weights and the segmentation colouriser -- not part of the encode / quantize / decode network
_LDM_TRAINING_ONLY = ('loss.', 'model_ema.', 'colorize')


def convert_ldm_first_stage(state_dict):
    """ldm_exp first-stage state dict -> state dict with this package's / Diffusers' VQModel keys.  Takes a LatentDiffusion
    checkpoint (its `first_stage_model.*` entries; every other entry is skipped) or a standalone ldm_exp VQModel checkpoint (its
    training-only `loss.*`, `model_ema.*` and `colorize` entries are skipped).  The 1x1-conv attention projections [C, C, 1, 1]
    become Linear weights [C, C]."""
    pre = 'first_stage_model.'
    if any(k.startswith(pre) for k in state_dict):
        state_dict = {k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}
    state_dict = {k: v for k, v in state_dict.items() if not k.startswith(_LDM_TRAINING_ONLY)}
    ups = [int(k.split('.')[2]) for k in state_dict if k.startswith('decoder.up.')]
    levels = 1 + max(ups) if ups else 0
    out = {}
    for k, v in state_dict.items():
        nk = ldm_first_stage_key(k, levels)
        if '.attentions.' in nk and '.group_norm.' not in nk and v.dim() == 4:
            v = v.reshape(v.shape[0], v.shape[1])
        out[nk] = v
    return out


def vq_config_from_ldm(ddconfig, embed_dim, n_embed):
    """VQModel kwargs equivalent to an ldm_exp first stage (first_stage_config.params: ddconfig, embed_dim, n_embed).  The
    ldm_exp Encoder / Decoder normalise with 32 groups and eps 1e-6 (model.py:38-39)."""
    if ddconfig.get('double_z', False):
        raise NotImplementedError('double_z first stages are KL autoencoders, not VQ')
    if list(ddconfig.get('attn_resolutions', [])):
        raise NotImplementedError('attention inside the first stage\'s levels (attn_resolutions) is not a VQModel layout')
    if ddconfig.get('attn_type', 'vanilla') != 'vanilla':
        raise NotImplementedError('attn_type %r' % ddconfig.get('attn_type'))
    mult = list(ddconfig['ch_mult'])
    return dict(in_channels=ddconfig.get('in_channels', 3), out_channels=ddconfig.get('out_ch', 3),
                down_block_types=['DownEncoderBlock2D'] * len(mult), up_block_types=['UpDecoderBlock2D'] * len(mult),
                block_out_channels=[ddconfig['ch'] * m for m in mult], layers_per_block=ddconfig['num_res_blocks'], act_fn='silu',
                latent_channels=ddconfig['z_channels'], sample_size=ddconfig.get('resolution', 256), num_vq_embeddings=n_embed,
                norm_num_groups=32, vq_embed_dim=embed_dim, scaling_factor=0.18215)


def kl_config_from_ldm(ddconfig, embed_dim):
    """AutoencoderKL kwargs equivalent to an ldm_exp KL first stage (first_stage_config.params: ddconfig, embed_dim;
    ldm/models/autoencoder.py:285-310).  `double_z` is required; ldm_exp's quant_conv maps 2 z_channels -> 2 embed_dim and its
    post_quant_conv embed_dim -> z_channels, which is the Diffusers layout only when embed_dim == z_channels (every shipped config)."""
    if not ddconfig.get('double_z', False):
        raise NotImplementedError('a first stage without double_z is a VQ autoencoder, not KL (vq_config_from_ldm)')
    if embed_dim != ddconfig['z_channels']:
        raise NotImplementedError('embed_dim %r != z_channels %r is not an AutoencoderKL layout' % (embed_dim, ddconfig['z_channels']))
    cfg = vq_config_from_ldm(dict(ddconfig, double_z=False), embed_dim, 0)       # the same refusals, in the same words
    for k in ('num_vq_embeddings', 'vq_embed_dim'):
        del cfg[k]
    return cfg


# --------------------------------------------------------------------------------------------------------
# finetuned LDM weights in the reference's LatentDiffusion key layout (ldm_exp/main.py checkpoints, read back by
# sample_for_FID.py:44-48 with `load_state_dict(sd, strict=False)` into the pruned pickle)
# --------------------------------------------------------------------------------------------------------
LDM_UNET_PREFIX, LDM_EMBEDDER_PREFIX, LDM_EMA_PREFIX = 'model.diffusion_model.', 'cond_stage_model.', 'model_ema.'


def lit_ema_key(name):
    """LitEma's buffer name of UNet parameter `name` (ldm/modules/ema.py:16-21: the DiffusionWrapper's parameter name
    'diffusion_model.<name>' with every dot removed, since buffer names may not contain dots)."""
    return LDM_EMA_PREFIX + ('diffusion_model.' + name).replace('.', '')


def _ema_parts(ema):
    if ema is None:
        return None
    if isinstance(ema, dict):
        return float(ema['decay']), int(ema['num_updates']), ema['shadow']
    return float(ema.ema_decay), int(ema.num_updates), ema.ema_state()       # an ldm_train.LdmFinetuneEngine


def ldm_finetuned_state_dict(model, embedder, ema=None):
    """{'model.diffusion_model.<name>', 'cond_stage_model.embedding.weight', and with `ema` 'model_ema.decay',
    'model_ema.num_updates', 'model_ema.diffusion_model<name without dots>'} -> CPU tensors.
    ema: None, an ldm_train.LdmFinetuneEngine built with use_ema=True, or dict(decay, num_updates, shadow={name: tensor})."""
    sd = {LDM_UNET_PREFIX + n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    sd.update({LDM_EMBEDDER_PREFIX + n: p.detach().cpu().clone() for n, p in embedder.named_parameters()})
    parts = _ema_parts(ema)
    if parts is not None:
        decay, num_updates, shadow = parts
        sd[LDM_EMA_PREFIX + 'decay'] = torch.tensor(decay, dtype=torch.float32)
        sd[LDM_EMA_PREFIX + 'num_updates'] = torch.tensor(num_updates, dtype=torch.int)
        for n, _ in model.named_parameters():
            sd[lit_ema_key(n)] = shadow[n].detach().cpu().clone()
    return sd


def save_ldm_finetuned(path, model, embedder, ema=None, training_state=None, epoch=0):
    """A file holding {'state_dict': ldm_finetuned_state_dict(...)}, the layout of the reference's Lightning checkpoints.
    training_state: an ldm_train.LdmFinetuneEngine -- adds what Lightning's `last.ckpt` carries to continue a run:
    `optimizer_states` = [engine.optimizer_state_dict()] (torch.optim.AdamW's layout, UNet then embedder, ddpm.py:1372-1381),
    `global_step` (optimizer steps) and `epoch`.  Lightning is not available to this project's tests, so these three container key
    names are UNPINNED; the payload (AdamW's state layout) is pinned against torch itself."""
    blob = {'state_dict': ldm_finetuned_state_dict(model, embedder, ema)}
    if training_state is not None:
        blob.update(optimizer_states=[training_state.optimizer_state_dict()], global_step=int(training_state.step_count),
                    epoch=int(epoch))
    torch.save(blob, path)


def load_ldm_finetuned(path, model, embedder, engine=None):
    """Load a save_ldm_finetuned file (or a reference checkpoint of the same, possibly pruned, shapes) into `model` and
    `embedder` in place (parameters that live in a finetune engine's flat buffer stay there).  Keys this package does not know
    (`first_stage_model.*`, `betas`, ...) are ignored, as under strict=False; a key it knows with another shape is an error.
    engine: the ldm_train.LdmFinetuneEngine of `model` and `embedder` -- also restores Adam's moments and step from
    `optimizer_states[0]` and, when the engine keeps one, the LitEma shadow and `num_updates` (ValueError when the file has
    none, raised before anything is written; an engine built with use_ema=False ignores a file's shadow); the hyper-parameters
    stay the engine's.  The result then carries `global_step` and `epoch`.
    Returns dict(missing=[keys of ours absent from the file], ema=None | dict(decay, num_updates, shadow={name: tensor}))."""
    blob = torch.load(os.fspath(path), map_location='cpu', weights_only=True) if isinstance(path, (str, os.PathLike)) else path
    sd = blob['state_dict'] if 'state_dict' in blob else blob
    if engine is not None:                                  # what can be refused is refused before the first write
        if engine.model is not model or engine.embedder is not embedder:
            raise ValueError('load_ldm_finetuned: `engine` does not train this model and embedder')
        if 'optimizer_states' not in blob:
            raise ValueError('load_ldm_finetuned(engine=...): the file holds no optimizer_states (written without training_state=)')
        if engine.ema is not None and LDM_EMA_PREFIX + 'decay' not in sd:
            raise ValueError('the engine keeps a LitEma shadow, the file has none (model_ema.*): a resumed run would go on '
                             'with a stale shadow')
    missing = []
    with torch.no_grad():
        for prefix, mod in ((LDM_UNET_PREFIX, model), (LDM_EMBEDDER_PREFIX, embedder)):
            for n, p in list(mod.named_parameters()) + list(mod.named_buffers()):
                t = sd.get(prefix + n)
                if t is None:
                    missing.append(prefix + n)
                    continue
                if tuple(t.shape) != tuple(p.shape):
                    raise ValueError('%s: checkpoint shape %s, model shape %s' % (prefix + n, tuple(t.shape), tuple(p.shape)))
                p.data.copy_(t)
    eng = getattr(model, '_engine', None)
    if eng is not None:
        eng.packs.clear()                                   # in-place weight writes are invisible to the pack cache
    ema = None
    if LDM_EMA_PREFIX + 'decay' in sd:
        shadow = {}
        for n, p in model.named_parameters():
            t = sd.get(lit_ema_key(n))
            if t is None:
                missing.append(lit_ema_key(n))
            elif tuple(t.shape) != tuple(p.shape):
                raise ValueError('%s: checkpoint shape %s, model shape %s' % (lit_ema_key(n), tuple(t.shape), tuple(p.shape)))
            else:
                shadow[n] = t
        ema = dict(decay=float(sd[LDM_EMA_PREFIX + 'decay']), num_updates=int(sd[LDM_EMA_PREFIX + 'num_updates']), shadow=shadow)
    out = dict(missing=missing, ema=ema)
    if engine is not None:
        own = None
        if engine.ema is not None:
            own = engine.ema_state()
            absent = [n for n in own if n not in ema['shadow']]
            if absent:
                raise ValueError('the file\'s LitEma shadow lacks %s' % absent[:5])
        engine.load_optimizer_state_dict(blob['optimizer_states'][0])
        if own is not None:
            for n, t in own.items():
                t.copy_(ema['shadow'][n])
            engine.num_updates = ema['num_updates']
        engine._weights_changed()
        out.update(global_step=int(blob.get('global_step', engine.step_count)), epoch=int(blob.get('epoch', 0)))
    return out


# --------------------------------------------------------------------------------------------------------
# training state: the native one-file form, and the DDIM code base's `ckpt.pth` list
# --------------------------------------------------------------------------------------------------------
TRAINING_STATE_VERSION = 1


def _engine_modules(engine):
    """[(key in the file, module)] whose weights a training-state file holds."""
    mods = [('weights', engine.model)]
    if getattr(engine, 'embedder', None) is not None:
        mods.append(('embedder', engine.embedder))
    return mods


def _is_writer(engine):
    import torch.distributed as dist
    from .sweep import dist_active
    active = dist_active(engine.group)
    return active, (not active or dist.get_rank(engine.group) == 0)


def save_training_state(path, engine):
    """One file to stop a finetune and go on later, bit for bit: the weights by parameter name (for the LDM engine the embedder's
    too) and engine.state_dict() (train_state.py: moments, EMA shadow, counters, LR schedule, layout, hyper-parameters).  Plain
    tensors, numbers, strings and lists: it loads under weights_only=True.  The model is NOT described: rebuild it first as today
    (load_pruned, the whole-module pickle, or the config).  The teacher of a distillation engine, the data-loader position and
    host generators stay with the caller.  Under a process group the state is the same on every rank: rank 0 writes, every
    rank returns once the file is there.  Raises ValueError in the middle of an accumulation window."""
    active, writer = _is_writer(engine)
    state = engine.state_dict(device='cpu') if writer else engine.state_dict()      # (every rank checks the window)
    if writer:
        blob = dict(format_version=TRAINING_STATE_VERSION, engine=type(engine).__name__, training_state=state)
        for key, mod in _engine_modules(engine):
            blob[key] = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
        tmp = os.fspath(path) + '.tmp'
        torch.save(blob, tmp)
        os.replace(tmp, os.fspath(path))
    if active:
        import torch.distributed as dist
        dist.barrier(group=engine.group)


def load_training_state(path, engine, strict=True):
    """Load a save_training_state file into `engine` and its (already rebuilt) model in place: weights into the parameters (views
    of the engine's flat buffer), the state through engine.load_state_dict(strict=strict).  Every rank loads.  A file taken at
    another parameter layout (an un-pruned state for a pruned model), or whose state fails any other check of
    engine.check_state_dict, raises ValueError before anything is written."""
    from . import train_state
    blob = torch.load(os.fspath(path), map_location='cpu', weights_only=True)
    if blob.get('format_version') != TRAINING_STATE_VERSION:
        raise ValueError('unsupported training-state file format %r' % (blob.get('format_version'),))
    if blob.get('engine') != type(engine).__name__:
        raise ValueError('the file holds a %s state, the engine is a %s' % (blob.get('engine'), type(engine).__name__))
    state = blob['training_state']
    train_state.check_layout(train_state.param_layout(engine._state_named()), state['layout'])
    todo = []
    for key, mod in _engine_modules(engine):
        own, got = mod.state_dict(), blob[key]
        if list(own) != list(got):
            raise ValueError('%s: the file\'s tensor names differ from the model\'s (%s)' % (key, sorted(set(own) ^ set(got))[:5]))
        for k, t in own.items():
            if tuple(t.shape) != tuple(got[k].shape):
                raise ValueError('%s.%s: file shape %s, model shape %s' % (key, k, tuple(got[k].shape), tuple(t.shape)))
            todo.append((t, got[k]))
    engine.check_state_dict(state, strict=strict)            # every check before the first write
    with torch.no_grad():
        for t, src in todo:
            t.copy_(src)                                     # state_dict() tensors share the parameters' storage
    engine.load_state_dict(state, strict=strict)
    engine._weights_changed()


def ddpm_original_parameter_order(keys):
    """`keys` (parameter names of a ddpm_exp `Model`) in the order of that model's `parameters()`, which is the order its
    constructor registers modules in (models/diffusion.py:215-299): temb.dense, conv_in, down.<level> (its blocks, then its
    attentions, then downsample), mid (block_1, attn_1, block_2), up.<level> ascending (blocks, attentions, upsample), norm_out,
    conv_out; inside a block norm1, conv1, temb_proj, norm2, conv2, nin_shortcut; inside an attention norm, q, k, v, proj_out;
    weight before bias.  Adam's state indices and EMAHelper's shadow LIST are positional in this order -- not UNet2DModel's."""
    top = {'temb': 0, 'conv_in': 1, 'down': 2, 'mid': 3, 'up': 4, 'norm_out': 5, 'conv_out': 6}
    res = {a: i for i, (a, _) in enumerate(_RES_O2D)}
    att = {a: i for i, (a, _) in enumerate(_ATT_O2D)}
    leaf = {'weight': 0, 'bias': 1}

    def key(k):
        p = k.split('.')
        if p[0] not in top or p[-1] not in leaf:
            raise KeyError('not a ddpm_exp Model parameter: %s' % k)
        if p[0] == 'temb':
            mid = (int(p[2]),)
        elif p[0] in ('down', 'up'):
            kind = {'block': 0, 'attn': 1, 'downsample': 2, 'upsample': 2}[p[2]]
            mid = (int(p[1]), kind) + ((int(p[3]), (res if kind == 0 else att)[p[4]]) if kind < 2 else (0, 0))
        elif p[0] == 'mid':
            mid = ({'block_1': 0, 'attn_1': 1, 'block_2': 2}[p[1]], (att if p[1] == 'attn_1' else res)[p[2]])
        else:
            mid = ()
        return (top[p[0]],) + mid + (leaf[p[-1]],)
    return sorted(keys, key=key)


def _ddpm_exp_names(engine):
    """(our parameter names, the same tensors' ddpm_exp names in that model's parameters() order, {ddpm_exp name: ours})."""
    ours = [n for n, _ in engine.model.named_parameters()]
    o2d = {o: d for d, o in zip(ours, convert_to_ddpm_original({n: torch.empty(0) for n in ours}))}
    return ours, ddpm_original_parameter_order(o2d), o2d


def save_ddpm_exp_states(path, engine, epoch):
    """The `ckpt.pth` list of the DDIM code base (runners/diffusion.py:331-344) from a train.FinetuneEngine:
    [state dict in that code base's key names, optimizer.state_dict(), epoch, step, EMAHelper's shadow list (with EMA)] --
    what its `--resume_training` reads (:236-248; element 0 as a state dict is its `else` branch).  Adam's indices and the shadow
    list are positional in the order of THAT model's parameters() (ddpm_original_parameter_order); the attention projections
    are 1x1 convolutions there, so their weights, moments and shadow are written as [C, C, 1, 1].  Under a process group rank 0
    writes and every rank returns once the file is there, as save_training_state."""
    engine._check_window('save_ddpm_exp_states()')
    ours, order, o2d = _ddpm_exp_names(engine)
    named = dict(engine.model.named_parameters())
    opt = engine.optimizer_state_dict()

    def to_orig(by_ours):
        conv = convert_to_ddpm_original(by_ours)
        return [conv[o] for o in order]
    weights = to_orig({n: named[n].detach().cpu().clone() for n in ours})
    m = to_orig({n: opt['state'][i]['exp_avg'] for i, n in enumerate(ours)})
    v = to_orig({n: opt['state'][i]['exp_avg_sq'] for i, n in enumerate(ours)})
    state = {i: dict(step=opt['state'][0]['step'].clone(), exp_avg=m[i], exp_avg_sq=v[i]) for i in range(len(order))}
    states = [dict(zip(order, weights)), dict(state=state, param_groups=opt['param_groups']), int(epoch), int(engine.step_count)]
    if engine.ema is not None:
        states.append(to_orig({n: t.detach().cpu().clone() for n, t in engine.ema_state().items()}))
    active, writer = _is_writer(engine)
    if writer:
        tmp = os.fspath(path) + '.tmp'
        torch.save(states, tmp)
        os.replace(tmp, os.fspath(path))
    if active:
        import torch.distributed as dist
        dist.barrier(group=engine.group)


def load_ddpm_exp_states(path, engine):
    """Read a `ckpt.pth` list (a path or the list itself) into a train.FinetuneEngine and its model in place; returns (epoch, step).
    The hyper-parameters come from the ENGINE, not from the file's param_groups (the reference overrides eps the same way,
    runners/diffusion.py:243).  A list whose element 0 is a pickled module (what the reference's own loop writes) is refused: save
    that module's state_dict() instead, or rebuild the model from it first."""
    import pickle
    if isinstance(path, (str, os.PathLike)):
        try:
            states = torch.load(os.fspath(path), map_location='cpu', weights_only=True)
        except pickle.UnpicklingError as e:
            raise ValueError('%s does not load as plain tensors: element 0 of a ckpt.pth written by the reference\'s training loop is '
                             'a pickled module; store its state_dict() there instead (%s)' % (path, str(e).splitlines()[0])) from None
    else:
        states = path
    if not isinstance(states, (list, tuple)) or len(states) < 4:
        raise ValueError('a ckpt.pth holds [state dict, optimizer state, epoch, step(, ema list)]')
    if isinstance(states[0], torch.nn.Module) or not isinstance(states[0], dict):
        raise ValueError('element 0 of the ckpt.pth list is a %s, not a state dict: a pickled module is not read here'
                         % type(states[0]).__name__)
    engine._check_window('load_ddpm_exp_states()')
    ours, order, o2d = _ddpm_exp_names(engine)
    named = dict(engine.model.named_parameters())
    if sorted(states[0]) != sorted(order):
        raise ValueError('the checkpoint\'s parameter names differ from the model\'s (%s)' % sorted(set(states[0]) ^ set(order))[:5])
    w = convert_ddpm_original(dict(states[0]))
    for n in ours:
        if tuple(w[n].shape) != tuple(named[n].shape):
            raise ValueError('%s: checkpoint shape %s, model shape %s' % (n, tuple(w[n].shape), tuple(named[n].shape)))
    opt = states[1]
    ids = [i for g in opt['param_groups'] for i in g['params']]
    if len(ids) != len(order):
        raise ValueError('the optimizer state covers %d parameters, the model has %d' % (len(ids), len(order)))
    pos = {n: i for i, n in enumerate(ours)}

    def to_ours(tensors):                                    # positional in `order` -> indexed by our parameter order
        conv = convert_ddpm_original(dict(zip(order, tensors)))
        return [conv[n] for n in ours]
    state = {}
    if opt['state']:
        m = to_ours([opt['state'][i]['exp_avg'] for i in ids])
        v = to_ours([opt['state'][i]['exp_avg_sq'] for i in ids])
        state = {pos[n]: dict(step=opt['state'][ids[0]]['step'], exp_avg=m[pos[n]], exp_avg_sq=v[pos[n]]) for n in ours}
        steps = {float(opt['state'][i]['step']) for i in ids}
        if len(steps) != 1:
            raise ValueError('the parameters are at different optimizer steps: %s' % sorted(steps))
    shadow = None
    if engine.ema is not None:
        if len(states) < 5:
            raise ValueError('the engine keeps an EMA shadow, the ckpt.pth list has none (element 4)')
        shadow = to_ours(list(states[4]) if isinstance(states[4], (list, tuple)) else list(states[4].values()))
        for n, t in zip(ours, shadow):
            if tuple(t.shape) != tuple(named[n].shape):
                raise ValueError('EMA shadow of %s: shape %s, model shape %s' % (n, tuple(t.shape), tuple(named[n].shape)))
    engine.load_optimizer_state_dict(dict(state=state, param_groups=[dict(params=list(range(len(ours))))]))
    with torch.no_grad():
        for n in ours:
            named[n].data.copy_(w[n])
        if shadow is not None:
            for (n, dst), t in zip(engine.ema_state().items(), shadow):
                dst.copy_(t)
    engine._weights_changed()
    return int(states[2]), int(states[3])
