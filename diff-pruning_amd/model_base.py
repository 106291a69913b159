"""What the nn.Module front ends (unet.UNet2DModel, vq.VQModel, vae.AutoencoderKL, ldm.UNetModel) share: they hold parameters
and hand all arithmetic to a HIP engine, so the engine's life-cycle, the Diffusers directory plumbing and the small holders are
written once here.  There is no CPU / PyTorch fallback."""
from collections import OrderedDict

import torch
import torch.nn as nn

from .engine import _PinnedWeights


class BaseOutput(OrderedDict):
    """diffusers.utils.BaseOutput behaviour: attribute, key and index access, `.to_tuple()`."""

    def __init__(self, **fields):
        super().__init__()
        for k, v in fields.items():
            self[k] = v

    def __getattr__(self, name):
        try:
            return OrderedDict.__getitem__(self, name)
        except KeyError:
            raise AttributeError(name) from None

    def __getitem__(self, k):
        return OrderedDict.__getitem__(self, k) if isinstance(k, str) else self.to_tuple()[k]

    def to_tuple(self):
        return tuple(self.values())


class FrozenConfig(dict):
    """dict with attribute access (Diffusers' FrozenDict behaviour: `unet.config.sample_size`)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None          # keeps copy / pickle protocol probes working


class _Block(nn.Module):
    pass


class EngineModel(nn.Module):
    """A parameter holder run by a HIP engine.  A subclass gives its engine (`_new_engine`, called once, lazily), the parameter
    that `device` / `dtype` are read from (`_anchor`), whether it refuses anything but fp32 (`_fp32_only`) and the attributes
    besides the engine that a pickle leaves out (`_transient`)."""

    _fp32_only = False
    _transient = ()

    def __getstate__(self):
        """Whole-module pickles (`torch.save(model, 'unet_pruned.pth')`, ddpm_prune.py:135) carry parameters and shapes
        only: the HIP engine (packed operands, streams) is rebuilt on first use after loading."""
        state = dict(self.__dict__)
        state['_engine'] = None
        for k in self._transient:
            state.pop(k, None)
        return state

    def _new_engine(self):
        raise NotImplementedError

    def _anchor(self):
        raise NotImplementedError

    @property
    def dtype(self):
        return self._anchor().dtype

    @property
    def device(self):
        return self._anchor().device

    def engine(self):
        """The HIP execution engine bound to the *current* parameter tensors (re-bound after pruning).  In-place weight writes
        (EMAModel.copy_to / restore) are invisible to the packed-operand cache, so it is dropped on every call outside
        `pin_weights()` (the weights are packed again)."""
        w = self._anchor()
        if w.device.type != 'cuda':
            raise RuntimeError('%s runs on the MI355X HIP kernels only: move the model to a cuda device '
                               '(there is no CPU / PyTorch fallback)' % type(self).__name__)
        if self._fp32_only and w.dtype != torch.float32:
            raise NotImplementedError('%s runs in fp32 only' % type(self).__name__)
        if self._engine is None:
            self._engine = self._new_engine()
        self._engine.packs.rebind()
        self._engine.bind({n: p.detach() for n, p in self.named_parameters()}, None)
        return self._engine

    def pin_weights(self):
        """Context manager: the weights are not written inside the block (sweep, sampling loop, importance pass) -> the packed
        operands are kept across calls."""
        return _PinnedWeights(self)


class DiffusersModel(EngineModel):
    """EngineModel with the Diffusers directory surface; checkpoint.MODELS lists the classes and their pipeline sub-folders."""

    @classmethod
    def from_config(cls, config):
        return cls(**{k: v for k, v in dict(config).items() if not k.startswith('_')})

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, **kwargs):
        """config.json + diffusion_pytorch_model.{safetensors,bin} in a local directory (modeling_utils.py layout), in its
        `subfolder`, or in the class's own pipeline sub-folder."""
        from . import checkpoint
        return checkpoint.load_model(cls.__name__, pretrained_model_name_or_path, subfolder)

    def save_pretrained(self, save_directory, safe_serialization=False):
        from . import checkpoint
        checkpoint.save_model(self, save_directory, safe_serialization)
