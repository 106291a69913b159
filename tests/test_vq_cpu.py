"""VQ first stage and LDMPipeline, CPU part: the fp64 restatement (tests/vq_ref.py) against the reference-written fixtures
(tests/golden/make_golden_vq.py), the ldm_exp key map, the pipeline directory layout, deprecated attention names and the
configurations that are refused."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import pkg
import vq_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MICRO = os.path.join(GOLD, 'ldm_pipeline_micro')


def _fx():
    return dict(np.load(os.path.join(GOLD, 'vq_tiny.npz')))


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


def test_vq_ref_matches_reference_fixture():
    syn = pkg('synthetic')
    cfg, fx = syn.VQ_TINY_CFG, _fx()
    P = vq_ref.params(cfg, int(fx['seed']))
    x = torch.from_numpy(fx['x']).double()
    lat = vq_ref.encode(P, cfg, x)
    assert _rel(lat, fx['latents64']) < 1e-10
    zq, loss, idx, margin = vq_ref.quantize(lat, P['quantize.embedding.weight'])
    assert float(margin.min()) >= 1e-5 and float(fx['margin']) >= 1e-5
    assert torch.equal(idx, torch.from_numpy(fx['idx64']))
    assert torch.equal(idx, torch.from_numpy(fx['idx_cdist64'])) and torch.equal(idx, torch.from_numpy(fx['idx_cdist32']))
    assert _rel(zq, fx['zq64']) < 1e-12 and abs(float(loss) / float(fx['loss64']) - 1) < 1e-12
    assert _rel(vq_ref.decode(P, cfg, lat), fx['decode64']) < 1e-10
    assert _rel(vq_ref.decode(P, cfg, lat, force_not_quantize=True), fx['decode_nq64']) < 1e-10
    assert _rel(vq_ref.decode(P, cfg, vq_ref.encode(P, cfg, x)), fx['forward64']) < 1e-10
    # the fp32 restatement stays as close to fp64 as the reference's own fp32 run
    P32 = {k: v.float() for k, v in P.items()}
    lat32 = vq_ref.encode(P32, cfg, x.float())
    assert _rel(lat32, fx['latents64']) < 4 * max(_rel(fx['latents32'], fx['latents64']), 1e-7)
    # rows in identical pairs: the lowest index of a tie, as the reference's fp32 argmin chose it
    E = P32['quantize.embedding.weight']
    Edup = E[torch.arange(E.shape[0]) // 2]
    zq_dup, _, idx_dup, _ = vq_ref.quantize(torch.from_numpy(fx['latents32']), Edup)
    assert torch.equal(idx_dup, torch.from_numpy(fx['idx_dup32'])) and bool((idx_dup % 2 == 0).all())
    assert torch.equal(zq_dup, torch.from_numpy(fx['zq_dup32']))


def _ldm_keys():
    with open(os.path.join(GOLD, 'vq_ldm_keys.json')) as f:
        return json.load(f)


def _ldm_state_dict(cfg, seed):
    """The fixture's weights under ldm_exp keys (the mapping the generator checked with ldm_exp's own Encoder / Decoder)."""
    P = vq_ref.params(cfg, seed, torch.float32)
    return {lk: P[dk].reshape(shape) for lk, (dk, shape) in _ldm_keys()['keys'].items()}, P


def test_ldm_first_stage_key_map_reproduces_the_ldm_exp_leg():
    ckpt, syn = pkg('checkpoint'), pkg('synthetic')
    cfg = syn.VQ_TINY_CFG
    sd, P = _ldm_state_dict(cfg, int(_fx()['seed']))
    assert len(sd) == len(P) == 125
    for prefix in ('', 'first_stage_model.'):
        extra = {'model.diffusion_model.out.2.weight': torch.zeros(1)} if prefix else {}
        out = ckpt.convert_ldm_first_stage(dict({prefix + k: v for k, v in sd.items()}, **extra))
        assert set(out) == set(P)
        for k, v in out.items():
            assert v.shape == P[k].shape and torch.equal(v, P[k]), k
    levels = _ldm_keys()['levels']
    for lk, (dk, _) in _ldm_keys()['keys'].items():
        assert ckpt.ldm_first_stage_key(lk, levels) == dk
    model = pkg('vq').VQModel(**cfg)
    model.load_state_dict(ckpt.convert_ldm_first_stage(sd), strict=True)
    # a standalone ldm_exp VQModel checkpoint also holds its training-only state (loss module, LitEma copy, colouriser)
    standalone = dict(sd, **{'loss.discriminator.main.0.weight': torch.zeros(2), 'loss.logvar': torch.zeros(()),
                             'model_ema.decay': torch.zeros(()), 'model_ema.encoderconv_inweight': torch.zeros(1),
                             'colorize': torch.zeros(3, 4, 1, 1)})
    out = ckpt.convert_ldm_first_stage(standalone)
    assert set(out) == set(P) and all(torch.equal(out[k], P[k]) for k in P)
    with pytest.raises(KeyError):
        ckpt.convert_ldm_first_stage({'encoder.down.0.block.0.temb_proj.weight': torch.zeros(1)})


def test_vq_config_from_ldm_is_vq_f4():
    ckpt, syn, vq = pkg('checkpoint'), pkg('synthetic'), pkg('vq')
    dd = dict(double_z=False, z_channels=3, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4], num_res_blocks=2,
              attn_resolutions=[], dropout=0.0)                 # cin256-v2.yaml:41-59
    cfg = ckpt.vq_config_from_ldm(dd, 3, 8192)
    assert cfg == syn.VQ_F4_CFG
    model = vq.VQModel(**cfg)
    n_all = sum(p.numel() for p in model.parameters())
    n_dec = sum(p.numel() for n, p in model.named_parameters() if n.startswith('decoder.'))
    assert round(n_all / 1e6, 1) == 55.3 and round(n_dec / 1e6, 1) == 33.0
    with pytest.raises(NotImplementedError):
        ckpt.vq_config_from_ldm(dict(dd, double_z=True), 3, 8192)


def test_vq_model_keys_config_and_refusals():
    vq, syn = pkg('vq'), pkg('synthetic')
    model = vq.VQModel(**syn.VQ_TINY_CFG)
    assert list(model.state_dict()) == list(vq_ref.param_shapes(syn.VQ_TINY_CFG))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == vq_ref.param_shapes(syn.VQ_TINY_CFG)
    assert model.config.num_vq_embeddings == 64 and model.dtype == torch.float32 and model.device.type == 'cpu'
    with pytest.raises(RuntimeError, match='HIP'):
        model.decode(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match='HIP'):
        model.quantize(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match='17 channels'):
        vq.VQModel(**dict(syn.VQ_TINY_CFG, vq_embed_dim=17))
    with pytest.raises(NotImplementedError, match='remap'):
        vq.VQModel(remap='used_codes.npy', **syn.VQ_TINY_CFG)
    with pytest.raises(NotImplementedError, match='spatial'):
        vq.VQModel(norm_type='spatial', **syn.VQ_TINY_CFG)
    with pytest.raises(NotImplementedError):
        pkg('ops').vq_quantize(torch.zeros(1, 17, 2, 2), torch.zeros(4, 17))


def _micro_parts():
    vq, unet, diffusion = pkg('vq'), pkg('unet'), pkg('diffusion')
    syn = pkg('synthetic')

    def cfg(rel):
        with open(os.path.join(MICRO, rel)) as f:
            return {k: v for k, v in json.load(f).items() if not k.startswith('_')}
    vqm = vq.VQModel(**cfg('vqvae/config.json'))
    for n, p in vqm.named_parameters():
        p.data.copy_(torch.from_numpy(syn.det_param(n, p.shape, int(_fx()['seed']))))
    u = unet.UNet2DModel(**cfg('unet/config.json'))
    syn.det_init_(u, 81)
    sched = diffusion.DDIMScheduler(**{k: v for k, v in cfg('scheduler/scheduler_config.json').items()
                                      if k in ('beta_schedule', 'beta_start', 'beta_end', 'clip_sample')})
    return diffusion.LDMPipeline(vqvae=vqm, unet=u, scheduler=sched)


def test_ldm_pipeline_save_pretrained_matches_reference_layout(tmp_path):
    diffusion = pkg('diffusion')
    pipe = _micro_parts()
    out = str(tmp_path / 'ldm')
    pipe.save_pretrained(out)
    for rel in ('model_index.json', 'unet/config.json', 'vqvae/config.json'):
        with open(os.path.join(out, rel)) as f, open(os.path.join(MICRO, rel)) as g:
            assert json.load(f) == json.load(g), rel
    with open(os.path.join(out, 'scheduler/scheduler_config.json')) as f, \
            open(os.path.join(MICRO, 'scheduler/scheduler_config.json')) as g:
        ours, ref = json.load(f), json.load(g)
    assert all(ref[k] == v for k, v in ours.items())
    back = diffusion.LDMPipeline.from_pretrained(out)
    assert dict(back.vqvae.config) == dict(pipe.vqvae.config) and dict(back.unet.config) == dict(pipe.unet.config)
    assert type(back.scheduler) is diffusion.DDIMScheduler and back.scheduler.config.beta_schedule == 'scaled_linear'
    for a, b in ((back.vqvae, pipe.vqvae), (back.unet, pipe.unet)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    # a DDIM directory still loads as a DDIMPipeline without a vqvae
    ddim = diffusion.DDIMPipeline(unet=pipe.unet, scheduler=pipe.scheduler)
    ddim.save_pretrained(str(tmp_path / 'ddim'))
    with open(str(tmp_path / 'ddim' / 'model_index.json')) as f:
        assert 'vqvae' not in json.load(f)
    assert not hasattr(diffusion.DDIMPipeline.from_pretrained(str(tmp_path / 'ddim')), 'vqvae')


_DEPRECATED = (('to_q', 'query'), ('to_k', 'key'), ('to_v', 'value'), ('to_out.0', 'proj_attn'))


def _deprecate(sd):
    out = {}
    for k, v in sd.items():
        for new, old in _DEPRECATED:
            k = k.replace('.attentions.0.%s.' % new, '.attentions.0.%s.' % old) if '.attentions.' in k else k
        out[k] = v
    return out


def test_deprecated_attention_names_load(tmp_path):
    ckpt = pkg('checkpoint')
    pipe = _micro_parts()
    for model, load in ((pipe.vqvae, ckpt.load_vq), (pipe.unet, ckpt.load_unet)):
        d = str(tmp_path / type(model).__name__)
        model.save_pretrained(d)
        path = os.path.join(d, 'diffusion_pytorch_model.bin')
        sd = torch.load(path, weights_only=True)
        old = _deprecate(sd)
        assert any('.query.' in k for k in old) and any('.proj_attn.' in k for k in old)
        torch.save(old, path)
        back = load(d)
        sb = back.state_dict()
        assert list(sb) == list(sd) and all(torch.equal(sb[k], sd[k]) for k in sd)
    assert ckpt.convert_deprecated_attention_keys(sd) is sd           # no deprecated names: the same object, untouched


def test_vq_micro_batch_is_sized_from_the_largest_per_image_tensor(monkeypatch):
    """Every engine call must stay below 2 GiB (32-bit buffer offsets): encode / decode split the batch by the largest tensor of
    one image.  The rule's sizes equal the largest convolution input / output and attention-score tensor of the restatement."""
    vq, syn = pkg('vq'), pkg('synthetic')
    F = vq_ref.F
    seen = []
    conv, softmax = F.conv2d, torch.softmax

    def rec_conv(x, w, b=None, stride=1, padding=0):
        y = conv(x, w, b, stride=stride, padding=padding)
        # the stride-2 input is F.pad'ed by one row / column here; the engine reads the unpadded tensor
        seen.extend([x[0].numel() if stride == 1 else x.shape[1] * (x.shape[2] - 1) * (x.shape[3] - 1), y[0].numel()])
        return y

    def rec_softmax(x, dim):
        seen.append(x[0].numel())
        return softmax(x, dim=dim)
    monkeypatch.setattr(F, 'conv2d', rec_conv)
    monkeypatch.setattr(vq_ref.torch, 'softmax', rec_softmax)
    for cfg, lat_hw in ((syn.VQ_F4_CFG, 64), (syn.VQ_TINY_CFG, 8), (dict(syn.VQ_TINY_CFG, block_out_channels=[32, 64, 48]), 5)):
        eng = vq.VQEngine(cfg)
        P = {k: torch.empty(sh, device='meta') for k, sh in vq_ref.param_shapes(cfg).items()}
        f = 2 ** (len(cfg['block_out_channels']) - 1)
        for decode, shape in ((True, (1, 3, lat_hw, lat_hw)), (False, (1, 3, lat_hw * f, lat_hw * f))):
            seen.clear()
            x = torch.empty(shape, device='meta')
            if decode:
                vq_ref.decode(P, cfg, x, force_not_quantize=True)
            else:
                vq_ref.encode(P, cfg, x)
            assert eng.per_image_bytes(shape, decode) == 4 * max(seen), (cfg['block_out_channels'], decode)
    eng = vq.VQEngine(syn.VQ_F4_CFG)
    assert eng.per_image_bytes((1, 3, 64, 64), True) == 64 << 20                  # 256 channels at 256 x 256
    assert eng.micro_batch((1, 3, 64, 64), True) == 31 and eng.micro_batch((1, 3, 256, 256), False) == 31
