"""AutoencoderKL, CPU part: the parameter holders and config against the reference's key list, the directory round-trip, the ldm_exp
binding, the tile geometry, and the torch stand-ins of the two kernels of csrc/vae.hip (tests/kl_ref.py) against the reference's own
fp32 results, bit for bit (tests/golden/make_golden_kl.py wrote them)."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import kl_ref as R
from helpers import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    vae, syn = pkg('vae'), pkg('synthetic')
    model = vae.AutoencoderKL(**syn.KL_TINY_CFG)
    model.load_state_dict(R.params([(k, s) for k, s in R.keys()['state_dict']]), strict=True)
    return model.eval()


def test_state_dict_keys_order_shapes_and_config_equal_the_reference():
    vae, syn = pkg('vae'), pkg('synthetic')
    fx = R.keys()
    model = vae.AutoencoderKL(**syn.KL_TINY_CFG)
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == fx['state_dict']
    want = {k: v for k, v in fx['config'].items() if not k.startswith('_')}
    assert {k: (list(v) if isinstance(v, tuple) else v) for k, v in model.config.items()} == want
    assert sd['encoder.conv_out.weight'].shape[0] == 8 and sd['quant_conv.weight'].shape == (8, 8, 1, 1)
    assert sd['post_quant_conv.weight'].shape == (4, 4, 1, 1)
    d = vae.AutoencoderKL()                                                           # the reference's defaults
    assert d.config.latent_channels == 4 and d.config.scaling_factor == 0.18215 and d.config.sample_size == 32
    assert d.config.block_out_channels == (64,) and d.config.norm_num_groups == 32
    assert (model.tile_sample_min_size, model.tile_latent_min_size, model.tile_overlap_factor) == (16, 8, 0.25)
    assert model.use_tiling is False and model.use_slicing is False
    model.enable_tiling()
    model.enable_slicing()
    assert model.use_tiling and model.use_slicing
    model.disable_tiling()
    model.disable_slicing()
    assert not model.use_tiling and not model.use_slicing
    model.enable_tiling(False)
    assert not model.use_tiling


def test_refusals_are_worded_as_vq_models():
    vae, vq, syn = pkg('vae'), pkg('vq'), pkg('synthetic')
    cfg = syn.KL_TINY_CFG
    for kw in (dict(norm_type='spatial'), dict(act_fn='relu'), dict(down_block_types=['AttnDownEncoderBlock2D'] * 2)):
        with pytest.raises(NotImplementedError) as a:
            vae.AutoencoderKL(**dict(cfg, **kw))
        with pytest.raises(NotImplementedError) as b:
            vq.VQModel(**dict(syn.VQ_TINY_CFG, **kw))
        assert str(a.value) == str(b.value).replace('VQModel', 'AutoencoderKL')
    with pytest.raises(TypeError, match='num_vq_embeddings'):
        vae.AutoencoderKL(**dict(cfg, num_vq_embeddings=4))
    with pytest.raises(ValueError):
        vae.AutoencoderKL(**dict(cfg, block_out_channels=[16]))
    model = _model()
    assert model.dtype == torch.float32 and model.device.type == 'cpu'
    for call in (lambda: model.encode(torch.zeros(1, 3, 16, 16)), lambda: model.decode(torch.zeros(1, 4, 8, 8)),
                 lambda: model(torch.zeros(1, 3, 16, 16)), lambda: vae.DiagonalGaussianDistribution(torch.zeros(1, 8, 2, 2))):
        with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
            call()


def test_config_and_directory_round_trip(tmp_path):
    vae, ckpt = pkg('vae'), pkg('checkpoint')
    model = _model()
    again = vae.AutoencoderKL.from_config(dict(model.config, _class_name='AutoencoderKL'))
    assert dict(again.config) == dict(model.config)
    for safe in (False, True):
        d = str(tmp_path / ('safe' if safe else 'bin'))
        model.save_pretrained(d, safe_serialization=safe)
        with open(os.path.join(d, 'config.json')) as f:
            cfg = json.load(f)
        assert cfg['_class_name'] == 'AutoencoderKL' and cfg['latent_channels'] == 4 and cfg['block_out_channels'] == [16, 32]
        back = vae.AutoencoderKL.from_pretrained(d)
        sa, sb = model.state_dict(), back.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa) and dict(back.config) == dict(model.config)
    # under a `vae/` folder, as the Diffusers latent pipelines keep it: found with and without the subfolder's name
    model.save_pretrained(str(tmp_path / 'pipe' / 'vae'))
    for back in (vae.AutoencoderKL.from_pretrained(str(tmp_path / 'pipe')),
                 vae.AutoencoderKL.from_pretrained(str(tmp_path / 'pipe'), subfolder='vae')):
        assert all(torch.equal(v, back.state_dict()[k]) for k, v in model.state_dict().items())
    vqm = pkg('vq').VQModel(**pkg('synthetic').VQ_TINY_CFG)
    vqm.save_pretrained(str(tmp_path / 'vq'))
    with pytest.raises(ValueError, match='VQModel'):
        ckpt.load_vae(str(tmp_path / 'vq'))


def test_pipeline_directories_name_the_first_stage_class(tmp_path):
    diffusion, unet, syn = pkg('diffusion'), pkg('unet'), pkg('synthetic')
    micro = os.path.join(R.GOLD, 'ldm_pipeline_micro')
    with open(os.path.join(micro, 'unet', 'config.json')) as f:
        u = unet.UNet2DModel(**{k: v for k, v in json.load(f).items() if not k.startswith('_')})
    syn.det_init_(u, 81)
    pipe = diffusion.LDMPipeline(vqvae=_model(), unet=u, scheduler=diffusion.DDIMScheduler())
    pipe.save_pretrained(str(tmp_path / 'kl'))
    with open(str(tmp_path / 'kl' / 'model_index.json')) as f:
        assert json.load(f)['vqvae'] == ['diffusers', 'AutoencoderKL']
    back = diffusion.LDMPipeline.from_pretrained(str(tmp_path / 'kl'))
    assert type(back.vqvae).__name__ == 'AutoencoderKL'
    assert all(torch.equal(v, back.vqvae.state_dict()[k]) for k, v in pipe.vqvae.state_dict().items())
    with open(os.path.join(micro, 'model_index.json')) as f:                     # the reference-written VQ directory names VQModel
        assert json.load(f)['vqvae'] == ['diffusers', 'VQModel']


def test_kl_config_from_ldm_and_the_key_map():
    ckpt, vae, syn = pkg('checkpoint'), pkg('vae'), pkg('synthetic')
    f8 = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
              attn_resolutions=[], dropout=0.0)                         # models/first_stage_models/kl-f8/config.yaml
    assert ckpt.kl_config_from_ldm(f8, 4) == syn.KL_F8_CFG
    f4 = dict(f8, z_channels=3, ch_mult=[1, 2, 4])                      # kl-f4
    cfg = ckpt.kl_config_from_ldm(f4, 3)
    assert cfg['block_out_channels'] == [128, 256, 512] and cfg['latent_channels'] == 3 and 'num_vq_embeddings' not in cfg
    vae.AutoencoderKL(**dict(cfg, block_out_channels=[32, 64, 128]))
    f16 = dict(f8, z_channels=16, ch_mult=[1, 1, 2, 2, 4], attn_resolutions=[16])
    with pytest.raises(NotImplementedError) as a:
        ckpt.kl_config_from_ldm(f16, 16)
    with pytest.raises(NotImplementedError) as b:
        ckpt.vq_config_from_ldm(dict(f16, double_z=False), 16, 8)
    assert str(a.value) == str(b.value) and 'attn_resolutions' in str(a.value)
    with pytest.raises(NotImplementedError, match='embed_dim'):
        ckpt.kl_config_from_ldm(f8, 8)
    with pytest.raises(NotImplementedError, match='double_z'):
        ckpt.kl_config_from_ldm(dict(f8, double_z=False), 4)
    with pytest.raises(NotImplementedError, match='double_z'):
        ckpt.vq_config_from_ldm(f8, 4, 8)
    # the key map the generator checked with ldm_exp's own Encoder(double_z=True) / Decoder
    with open(os.path.join(R.GOLD, 'kl_ldm_keys.json')) as f:
        km = json.load(f)
    P = R.params([(k, s) for k, s in R.keys()['state_dict']])
    sd = {lk: P[dk].reshape(shape) for lk, (dk, shape) in km['keys'].items()}
    assert len(sd) == len(P)
    for lk, (dk, _) in km['keys'].items():
        assert ckpt.ldm_first_stage_key(lk, km['levels']) == dk
    for prefix, extra in (('', {'loss.logvar': torch.zeros(()), 'loss.discriminator.main.0.weight': torch.zeros(2)}),
                          ('first_stage_model.', {'model.diffusion_model.out.2.weight': torch.zeros(1)})):
        out = ckpt.convert_ldm_first_stage(dict({prefix + k: v for k, v in sd.items()}, **extra))
        assert set(out) == set(P) and all(out[k].shape == P[k].shape and torch.equal(out[k], P[k]) for k in P)
    tiny = dict(f8, z_channels=4, ch=16, ch_mult=[1, 2], num_res_blocks=1, resolution=16)
    model = vae.AutoencoderKL(**dict(ckpt.kl_config_from_ldm(tiny, 4), norm_num_groups=8))
    model.load_state_dict(ckpt.convert_ldm_first_stage(sd), strict=True)


def test_tile_geometry():
    vae = pkg('vae')
    # tiles of 16 every 12 over 40 x 28 pixels: 4 x 3 tiles, 4-pixel edge tiles (the fixture's grid)
    assert vae.tile_geometry(16, 8, 0.25) == (12, 2, 6) and vae.tile_geometry(8, 16, 0.25) == (6, 4, 12)
    assert vae.tile_spans(40, 16, 12) == [(0, 16), (12, 16), (24, 16), (36, 4)]
    assert vae.tile_spans(28, 16, 12) == [(0, 16), (12, 16), (24, 4)]
    assert vae.tile_spans(20, 8, 6) == [(0, 8), (6, 8), (12, 8), (18, 2)] and vae.tile_spans(14, 8, 6) == [(0, 8), (6, 8), (12, 2)]
    # below, at and above the tile size
    assert vae.tile_spans(10, 16, 12) == [(0, 10)] and vae.tile_spans(12, 16, 12) == [(0, 12)]
    assert vae.tile_spans(16, 16, 12) == [(0, 16), (12, 4)] and vae.tile_spans(17, 16, 12) == [(0, 16), (12, 5)]
    assert vae.tile_spans(13, 16, 12) == [(0, 13), (12, 1)]               # an edge tile below the blend extent
    # the canvas: each tile gives min(length, row_limit); the fixture's tiles add up to the image
    assert vae.canvas_layout([8, 8, 8, 2], 6) == ([0, 6, 12, 18], 20) and vae.canvas_layout([16, 16, 4], 12) == ([0, 12, 24], 28)
    assert vae.canvas_layout([16, 1], 12) == ([0, 12], 13) and vae.canvas_layout([10], 12) == ([0], 10)
    # KL-f8 at sample_size 512: 64-latent tiles every 48, 128-pixel blends, 384-pixel crops
    assert vae.tile_geometry(64, 512, 0.25) == (48, 128, 384) and vae.tile_geometry(512, 64, 0.25) == (384, 16, 48)
    assert [s for s, _ in vae.tile_spans(256, 64, 48)] == [0, 48, 96, 144, 192, 240]
    model = _model()
    model.tile_sample_min_size, model.tile_latent_min_size, model.tile_overlap_factor = 32, 4, 0.5       # settable
    assert vae.tile_geometry(model.tile_sample_min_size, model.tile_latent_min_size, model.tile_overlap_factor) == (16, 2, 2)


@pytest.mark.parametrize('side', ['enc', 'dec'])
def test_tiling_loop_over_the_stand_in_reproduces_the_reference_tiles_and_canvas(side):
    """From the fixture's tiles as the reference's encoder / decoder left them: the loop of vae.blend_tiles over the torch stand-in of
    dp_tile_blend gives the reference's blended tiles and its concatenated canvas, bit for bit."""
    vae = pkg('vae')
    fx = R.load('kl_tiled.npz')
    nr, nc = (int(v) for v in fx['grid'])
    rows = [[torch.from_numpy(fx['%s_pre_%d_%d' % (side, i, j)]).clone() for j in range(nc)] for i in range(nr)]
    _, blend_extent, row_limit = vae.tile_geometry(16, 8, 0.25) if side == 'enc' else vae.tile_geometry(8, 16, 0.25)
    canvas = vae.blend_tiles(rows, blend_extent, row_limit, blend=R.tile_blend)
    changed = 0
    for i in range(nr):
        for j in range(nc):
            want = fx['%s_post_%d_%d' % (side, i, j)]
            assert np.array_equal(rows[i][j].numpy(), want), (side, i, j)
            changed += not np.array_equal(want, fx['%s_pre_%d_%d' % (side, i, j)])
    assert changed == nr * nc - 1                                          # every tile but the first is blended
    assert np.array_equal(canvas.numpy(), fx['moments32' if side == 'enc' else 'decode32'])
    assert tuple(rows[3][2].shape[2:]) == ((2, 2) if side == 'enc' else (4, 4))       # the corner tile: the blend extent itself


def test_posterior_stand_in_reproduces_the_reference_bit_for_bit():
    fx = R.load('kl_tiny.npz')
    m = torch.from_numpy(fx['moments32'])
    got = R.posterior(R.restride(m, fx['moments_strides32']), torch.from_numpy(fx['noise']))
    for name, key in (('logvar', 'logvar32'), ('std', 'std32'), ('var', 'var32'), ('z', 'sample32'), ('kl', 'kl32')):
        assert np.array_equal(got[name].numpy(), fx[key]), name
    assert np.array_equal(m[:, :4].numpy(), fx['mode32'])
    scaled = R.posterior(m, torch.from_numpy(fx['noise']), scale=0.18215)['z']
    assert torch.equal(scaled, 0.18215 * torch.from_numpy(fx['sample32']))
    # the noise the fixture stores is what the package's randn_tensor draws from the same generators
    diffusion = pkg('diffusion')
    for seed, key in ((R.NOISE_SEED, 'noise'), (R.FORWARD_SEED, 'forward_noise')):
        drawn = diffusion.randn_tensor(fx[key].shape, generator=torch.Generator().manual_seed(seed), device='cpu', dtype=torch.float32)
        assert np.array_equal(drawn.numpy(), fx[key])


def test_every_launch_site_of_vae_hip_is_in_its_branch_table():
    """csrc/vae.hip launches through VAE_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites are
    tabled in tests/test_vae_gpu.py.  The file is in both build lists, and its entry points are declared and bound."""
    import test_vae_gpu as T
    L, ops = pkg('_lib'), pkg('ops')
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['vae.hip']
    src = open(os.path.join(csrc, 'vae.hip')).read()
    body = src.replace('#define VAE_LAUNCH(', '')
    sites = re.findall(r'\bVAE_LAUNCH\((\(\w+<\w+>\)|\w+),', body)
    assert len(sites) == T.LAUNCH_SITES['vae.hip'] == body.count('VAE_LAUNCH(') == 4, sites
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define VAE_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert sorted(sites) == sorted(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    assert {f for f in os.listdir(csrc) if 'VAE_LAUNCH(' in open(os.path.join(csrc, f)).read()} == {'vae.hip'}
    assert 'csrc/vae.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/vae.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert 'asm' not in src and 'fp contract(off)' in src
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    assert len(L.SIGNATURES['dp_gaussian_posterior']) == 13 and len(L.SIGNATURES['dp_tile_blend']) == 17
    assert hdr.count('int dp_tile_blend(') == 1 and hdr.count('int dp_gaussian_posterior(') == 1
    m = re.search(r'#define DP_VAE_MAX_BLOCKS (\d+)', hdr)
    assert int(m.group(1)) == ops.VAE_MAX_BLOCKS == T.MAX_BLOCKS
    lib = L.load()
    assert lib.dp_gaussian_posterior_ws.restype is ctypes.c_longlong
    assert lib.dp_gaussian_posterior_ws(2, 1000) == 2 * 4 and lib.dp_gaussian_posterior_ws(1, 1 << 26) == 4096
    assert lib.dp_gaussian_posterior_ws(8192, 300) == 8192 and lib.dp_gaussian_posterior_ws(0, 5) == 0


def test_training_loss_terms_are_refused_and_ldm_sweep_takes_the_class():
    vae, ldm_sweep = pkg('vae'), pkg('ldm_sweep')
    assert list(inspect.signature(ldm_sweep.encode_first_stage).parameters) == ['vq', 'images', 'scale_factor', 'generator']
    assert ldm_sweep.AutoencoderKL is vae.AutoencoderKL
    d = object.__new__(vae.DiagonalGaussianDistribution)
    d.deterministic = False
    with pytest.raises(NotImplementedError, match='training-loss'):
        d.kl(other=d)
    with pytest.raises(NotImplementedError, match='training-loss'):
        d.nll(torch.zeros(1))


def test_an_image_past_the_reach_is_refused_before_any_launch():
    """KL-f8: the decoder's mid-block scores are 4 (h w)^2 bytes -- 1 GiB at 128 x 128 latents (a 1024 x 1024 image), 16 GiB at 256 x 256:
    the latter cannot be split by images and raises on the host; with tiling the largest tensor is a tile's."""
    vae, syn = pkg('vae'), pkg('synthetic')
    eng = vae.KLEngine(syn.KL_F8_CFG)
    assert eng.per_image_bytes((1, 4, 128, 128), True) == 1 << 30 and eng.micro_batch((1, 4, 128, 128), True) == 1
    assert eng.per_image_bytes((1, 4, 256, 256), True) == 1 << 34
    for shape, decode in (((1, 4, 256, 256), True), ((1, 3, 2048, 2048), False)):
        with pytest.raises(ValueError, match='enable_tiling'):
            eng.micro_batch(shape, decode)
    assert eng.micro_batch((64, 4, 64, 64), True) == 7           # a 512-pixel tile: 256 MiB per image (the last level reads 256 channels at 512 x 512)
