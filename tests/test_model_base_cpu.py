"""The surface the four nn.Module front ends share (model_base.py) and the one save / load pair behind the three Diffusers classes
(checkpoint.load_model / save_model), table-driven over the classes at the suite's tiny configurations.  CPU only."""
import itertools
import json
import os
import pickle
import shutil

import pytest
import torch

import golden_common as gc
from helpers import pkg

# class name -> (module, tiny configuration, the folder a pipeline directory keeps it in | None: no Diffusers directory form)
CASES = {'UNet2DModel': ('unet', lambda: gc.TINY_CFG, 'unet'),
         'VQModel': ('vq', lambda: pkg('synthetic').VQ_TINY_CFG, 'vqvae'),
         'AutoencoderKL': ('vae', lambda: pkg('synthetic').KL_TINY_CFG, 'vae'),
         'UNetModel': ('ldm', lambda: gc.LDM_TINY_CFG, None)}
DIFFUSERS = [n for n, c in CASES.items() if c[2] is not None]
TRANSIENT = ('_leaf_cache', '_structure_tracing', '_hook_warned')


def _cls(name):
    return getattr(pkg(CASES[name][0]), name)


def _new(name, seed=3):
    with torch.no_grad():
        return gc.det_init_(_cls(name)(**dict(CASES[name][1]())), seed).eval()


def _same_weights(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return list(sa) == list(sb) and all(sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]) for k in sa)


@pytest.fixture(scope='module')
def saved(tmp_path_factory):
    """{class name: (model, its save_pretrained directory)}, written once."""
    out = {}
    for name in DIFFUSERS:
        model = _new(name)
        d = str(tmp_path_factory.mktemp(name))
        model.save_pretrained(d)
        out[name] = (model, d)
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_device_dtype_and_the_cpu_refusal(name):
    model = _new(name)
    first = next(model.parameters())
    assert model.device == first.device and model.dtype == first.dtype == torch.float32
    assert model.double().dtype == torch.float64 == next(model.parameters()).dtype
    with pytest.raises(RuntimeError) as e:
        model.engine()
    assert name in str(e.value) and 'HIP' in str(e.value) and 'no CPU / PyTorch fallback' in str(e.value)
    assert model._engine is None                                   # refused before an engine is built


@pytest.mark.parametrize('name', list(CASES))
def test_pickle_drops_the_engine_and_the_transient_attributes(name):
    model = _new(name)
    model._engine = lambda: None                                   # stands for the engine: would not pickle
    if name == 'UNet2DModel':
        model.__dict__.update(_leaf_cache=[{}], _structure_tracing=True, _hook_warned={'tracer'})
    back = pickle.loads(pickle.dumps(model))
    assert type(back) is type(model) and back._engine is None and model._engine is not None
    assert not any(k in back.__dict__ for k in TRANSIENT)
    if name == 'UNet2DModel':
        assert all(k in model.__dict__ for k in TRANSIENT)         # the pickle left the live module alone
    assert dict(back.config) == dict(model.config) and _same_weights(back, model)


@pytest.mark.parametrize('name', DIFFUSERS)
def test_from_config_and_directory_round_trip(name, saved, tmp_path):
    ckpt = pkg('checkpoint')
    model, plain = saved[name]
    again = _cls(name).from_config(dict(model.config, _class_name=name, _diffusers_version=ckpt.DIFFUSERS_VERSION))
    assert type(again) is type(model) and dict(again.config) == dict(model.config)
    for safe in (False, True):
        d = str(tmp_path / ('safe' if safe else 'bin'))
        model.save_pretrained(d, safe_serialization=safe)
        assert sorted(os.listdir(d)) == ['config.json', 'diffusion_pytorch_model.' + ('safetensors' if safe else 'bin')]
        back = _cls(name).from_pretrained(d)
        assert type(back) is type(model) and not back.training
        assert dict(back.config) == dict(model.config) and _same_weights(back, model)
    # under the folder a pipeline directory keeps it in: found from the directory alone, and by the folder's name
    folder = CASES[name][2]
    model.save_pretrained(str(tmp_path / 'pipe' / folder))
    for back in (_cls(name).from_pretrained(str(tmp_path / 'pipe')), _cls(name).from_pretrained(str(tmp_path / 'pipe'), subfolder=folder)):
        assert _same_weights(back, model)
    # a config.json that does not name its class loads as before
    with open(os.path.join(plain, 'config.json')) as f:
        cfg = json.load(f)
    assert cfg.pop('_class_name') == name and cfg['_diffusers_version'] == ckpt.DIFFUSERS_VERSION
    os.makedirs(str(tmp_path / 'anon'))
    with open(str(tmp_path / 'anon' / 'config.json'), 'w') as f:
        json.dump(cfg, f)
    shutil.copyfile(os.path.join(plain, 'diffusion_pytorch_model.bin'), str(tmp_path / 'anon' / 'diffusion_pytorch_model.bin'))
    assert _same_weights(ckpt.load_model(name, str(tmp_path / 'anon')), model)


@pytest.mark.parametrize('held,asked', list(itertools.permutations(DIFFUSERS, 2)))
def test_a_directory_of_another_class_is_refused(held, asked, saved):
    ckpt = pkg('checkpoint')
    loaders = dict(UNet2DModel=ckpt.load_unet, VQModel=ckpt.load_vq, AutoencoderKL=ckpt.load_vae)
    for load in (loaders[asked], _cls(asked).from_pretrained):
        with pytest.raises(ValueError) as e:
            load(saved[held][1])
        assert held in str(e.value) and asked in str(e.value) and 'holds' in str(e.value)


@pytest.mark.parametrize('name', list(CASES))
def test_build_knows_every_class(name):
    ckpt = pkg('checkpoint')
    model = _new(name)
    built = ckpt._build(type(model).__name__, ckpt._config_dict(model))
    assert type(built) is type(model) and dict(built.config) == dict(model.config)
    assert [(k, tuple(v.shape)) for k, v in built.state_dict().items()] == [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
