"""Importance criteria, group pruner and channel-slicing functions with the `torch_pruning` call surface.

Mirrors the part of (vendored) torch_pruning the reference's prune scripts use:
  importance.TaylorImportance / MagnitudeImportance / RandomImportance   importance.py:11-16,18-126,221-225,332-434
  importance.LAMPImportance                                              importance.py:154-219
  pruner.MagnitudePruner (= MetaPruner).step(interactive) / prune_local  pruner/algorithms/metapruner.py:11-254
  MetaPruner(global_pruning=True) / prune_global                         pruner/algorithms/metapruner.py:126-133,256-297
  Group.prune()                                                          dependency.py:157-185
  function.prune_{conv,linear}_{out,in}_channels, prune_groupnorm_out_channels   pruner/function.py:85-146,168-207,274-302

Slicing: ONE table (`_SLICING`: per layer kind the count attribute, the weight dimension, what else is cut) read by one slicer
(`_slice_channels`); the `prune_*_channels` names are that slicer bound to a table row, and the batched group slice
(`_prune_group_batched`, ops.slice_batch) takes its rules from the same rows.

Scoring: ONE core (`_Criterion`).  A criterion is data -- the dp_wg_reduce modes of its conv / linear and GroupNorm members, whether
the finish takes |.|, whether it averages and normalises -- and the core selects the members that carry a term (`_terms`), describes
each as the reduction kernels see it (`_desc`) and scores them on the device (csrc/importance.hip) by one of three routes that give
the same bits: member by member (ops.wg_reduce, then ops.axpby / ops.gather_add), one group in one launch pair (ops.group_score),
every group in one launch pair (ops.score_groups, csrc/prune_global.hip).  The two batched routes lay their member table out with
the same function (`_MemberTable.add`); every route ends in the same `_finish`.  The argsort over the <= 1024 scores of a group and
the bookkeeping of the slicing are host work; global pruning selects on the device (ops.select_smallest).
The data-free criteria beyond the default configuration (MagnitudeImportance with another p, reduction or normaliser, LAMPImportance)
keep one row per member instead of a member sum and score through csrc/magnitude.hip (ops.magnitude_rows, ops.magnitude_finish).

`TaylorImportance.__call__(group, ch_groups=1)` accepts both this module's groups and groups produced by a real
`torch_pruning.DependencyGraph` (items `(dep, idxs)` with `dep.target.module` / `dep.handler`), so it can be handed
to `tp.pruner.MagnitudePruner(importance=...)` unchanged (drop-in boundary B1 of SURVEY.md §8b).
"""
import abc
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .graph import UNetGraph, LdmGraph, ChannelView, coupled_members, all_groups


# --------------------------------------------------------------------------------------------------------
# pruning functions (function.py:85-146, 168-207, 274-302): slice weights AND their accumulated grads
# --------------------------------------------------------------------------------------------------------
_index_cache = {}


def _index_tensor(key, build, device):
    """Small host->device index vectors recur across the members of one group (same channel count, same dropped
    set): build and upload each once.  The cache is bounded and only ever holds immutable index tensors."""
    k = (key, str(device))
    t = _index_cache.get(k)
    if t is None:
        if len(_index_cache) > 256:
            _index_cache.clear()
        t = torch.tensor(build(), dtype=torch.long, device=device)
        _index_cache[k] = t
    return t


def _keep(n, idxs, device):
    drop = frozenset(int(i) for i in idxs)
    return _index_tensor(('keep', n, drop), lambda: [i for i in range(n) if i not in drop], device)


def _slice_tensor(layer, attr, dim, keep):
    """A parameter keeps its accumulated gradient; running statistics are plain buffers.  What the layer does not have (no bias, a
    non-affine norm, untracked statistics) is None and stays so."""
    p = getattr(layer, attr, None)
    if p is None:
        return
    if not isinstance(p, nn.Parameter):
        setattr(layer, attr, p.data.index_select(dim, keep))
        return
    g = p.grad.data.index_select(dim, keep) if p.grad is not None else None
    newp = nn.Parameter(p.data.index_select(dim, keep))
    newp.grad = g
    setattr(layer, attr, newp)


# layer kind -> direction -> (attributes that hold the channel count, weight dimension that is cut, what follows on dimension 0).
# A kind without an 'in' row is cut the same way from either side (function.py gives those one function under two names).
_ALSO_BIAS, _ALSO_STATS = ('bias',), ('bias', 'running_mean', 'running_var')
_SLICING = {
    'conv':           {'out': (('out_channels',), 0, _ALSO_BIAS), 'in': (('in_channels',), 1, ())},
    'linear':         {'out': (('out_features',), 0, _ALSO_BIAS), 'in': (('in_features',), 1, ())},
    'conv_transpose': {'out': (('out_channels',), 1, _ALSO_BIAS), 'in': (('in_channels',), 0, ())},        # weight [Cin, Cout, k, k]
    # one filter per channel: in_channels, out_channels and groups shrink together
    'depthwise_conv': {'out': (('out_channels', 'in_channels', 'groups'), 0, _ALSO_BIAS)},
    'groupnorm':      {'out': (('num_channels',), 0, _ALSO_BIAS)},
    'layernorm':      {'out': (('normalized_shape',), 0, _ALSO_BIAS)},        # the normalised (last) dimension
    'batchnorm':      {'out': (('num_features',), 0, _ALSO_STATS)},
    'instancenorm':   {'out': (('num_features',), 0, _ALSO_STATS)},           # statistics, when tracked, so that the module stays usable
    'prelu':          {'out': (('num_parameters',), 0, ())},
    'embedding':      {'out': (('embedding_dim',), 1, ())},                   # the columns of the table
}
_LAYER_KINDS = ((nn.Linear, 'linear'), (nn.GroupNorm, 'groupnorm'), (nn.LayerNorm, 'layernorm'),
                (nn.modules.batchnorm._BatchNorm, 'batchnorm'), (nn.modules.instancenorm._InstanceNorm, 'instancenorm'),
                (nn.PReLU, 'prelu'), (nn.Embedding, 'embedding'))
_MEMBER_KINDS = {'ln': 'layernorm', 'gn': 'groupnorm', 'bn': 'batchnorm', 'inorm': 'instancenorm', 'prelu': 'prelu',
                 'embed': 'embedding'}


def _count(layer, attr):
    """The channel count behind a count attribute.  Hooks: LayerNorm keeps a shape tuple; a PReLU with one shared slope has none."""
    n = getattr(layer, attr)
    if attr == 'normalized_shape':
        return n[-1]
    if attr == 'num_parameters' and n == 1:
        return None
    return n


def _set_count(layer, attr, n):
    setattr(layer, attr, tuple(layer.normalized_shape[:-1]) + (n,) if attr == 'normalized_shape' else n)


def _slice_channels(layer, idxs, rule):
    """The one slicer: drop the channels `idxs` of `layer` as the table row `rule` says."""
    attrs, dim, also = rule
    n = _count(layer, attrs[0])
    if n is None:
        return layer
    # a non-affine norm has no weight to ask for the device, one without tracked statistics no running_mean; with neither only the count changes
    held = [t for t in (getattr(layer, 'weight', None), getattr(layer, 'running_mean', None)) if t is not None]
    keep = _keep(n, idxs, held[0].device if held else 'cpu')
    for attr in attrs:
        _set_count(layer, attr, n - len(set(idxs)))
    _slice_tensor(layer, 'weight', dim, keep)
    for attr in also:
        _slice_tensor(layer, attr, 0, keep)
    return layer


_FUNCTIONS = {}          # (layer kind, direction) -> its pruning function


def _pruning_function(kind, direction):
    """The slicer bound to one table row, under torch_pruning's name for it (`_member_kind` and the tests read handler names)."""
    def prune(layer, idxs):
        return _slice_channels(layer, idxs, prune.rule)
    prune.kind, prune.rule = kind, _SLICING[kind][direction]
    prune.__name__ = prune.__qualname__ = 'prune_%s_%s_channels' % (kind, direction)
    prune.__doc__ = 'function.py %s: cut %s, dimension %d of the weight%s.' % (
        prune.__name__, ' / '.join(prune.rule[0]), prune.rule[1], ''.join(', ' + a for a in prune.rule[2]))
    _FUNCTIONS[kind, direction] = prune
    return prune


prune_conv_out_channels = _pruning_function('conv', 'out')
prune_conv_in_channels = _pruning_function('conv', 'in')
prune_linear_out_channels = _pruning_function('linear', 'out')
prune_linear_in_channels = _pruning_function('linear', 'in')
prune_conv_transpose_out_channels = _pruning_function('conv_transpose', 'out')
prune_conv_transpose_in_channels = _pruning_function('conv_transpose', 'in')
prune_depthwise_conv_out_channels = _pruning_function('depthwise_conv', 'out')
prune_groupnorm_out_channels = _pruning_function('groupnorm', 'out')
prune_groupnorm_in_channels = prune_groupnorm_out_channels
prune_layernorm_out_channels = _pruning_function('layernorm', 'out')
prune_batchnorm_out_channels = _pruning_function('batchnorm', 'out')
prune_instancenorm_out_channels = _pruning_function('instancenorm', 'out')
prune_prelu_out_channels = _pruning_function('prelu', 'out')
prune_embedding_out_channels = _pruning_function('embedding', 'out')


function = SimpleNamespace(
    prune_batchnorm_out_channels=prune_batchnorm_out_channels, prune_batchnorm_in_channels=prune_batchnorm_out_channels,
    prune_depthwise_conv_out_channels=prune_depthwise_conv_out_channels,
    prune_depthwise_conv_in_channels=prune_depthwise_conv_out_channels,
    prune_instancenorm_out_channels=prune_instancenorm_out_channels, prune_instancenorm_in_channels=prune_instancenorm_out_channels,
    prune_prelu_out_channels=prune_prelu_out_channels, prune_prelu_in_channels=prune_prelu_out_channels,
    prune_embedding_out_channels=prune_embedding_out_channels, prune_embedding_in_channels=prune_embedding_out_channels,
    prune_conv_out_channels=prune_conv_out_channels, prune_conv_in_channels=prune_conv_in_channels,
    prune_linear_out_channels=prune_linear_out_channels, prune_linear_in_channels=prune_linear_in_channels,
    prune_groupnorm_out_channels=prune_groupnorm_out_channels, prune_groupnorm_in_channels=prune_groupnorm_in_channels,
    prune_layernorm_out_channels=prune_layernorm_out_channels)


for _kind, _rows in _SLICING.items():          # a kind without an 'in' row: the same cut by the same function from either side
    if 'in' not in _rows:
        _rows['in'], _FUNCTIONS[_kind, 'in'] = _rows['out'], _FUNCTIONS[_kind, 'out']
_kind_of_type = {}


def _layer_kind(layer):
    kind = _kind_of_type.get(type(layer))
    if kind is None:
        kind = _kind_of_type[type(layer)] = next((k for cls, k in _LAYER_KINDS if isinstance(layer, cls)), 'conv')
    return kind


def _handler_for(layer, kind):
    """The pruning function of a member: by the member kind for the pass-through layers, else by what the layer is."""
    lk = _MEMBER_KINDS.get(kind)
    if lk is None:
        lk = _layer_kind(layer)
        if lk == 'conv' and isinstance(layer, nn.modules.conv._ConvNd) and (layer.transposed or layer.groups > 1):
            lk = 'conv_transpose' if layer.transposed else 'depthwise_conv'
    return _FUNCTIONS[lk, 'in' if kind == 'in' else 'out']


def _out_channels(layer):
    return _count(layer, _SLICING[_layer_kind(layer)]['out'][0][0])


def _in_channels(layer):
    return _count(layer, _SLICING[_layer_kind(layer)]['in'][0][0])


# --------------------------------------------------------------------------------------------------------
# groups
# --------------------------------------------------------------------------------------------------------
class Dependency:
    """One member of a group: `handler(target.module, idxs)` prunes it (dependency.py:91-140 surface)."""
    __slots__ = ('target', 'handler', 'kind')

    def __init__(self, module, name, kind):
        self.target = SimpleNamespace(module=module, name=name)
        self.handler = _handler_for(module, kind)
        self.kind = kind

    def __call__(self, idxs):
        return self.handler(self.target.module, idxs)


class Group:
    """Iterates as (dep, idxs), root first (dependency.py:143-191)."""

    def __init__(self, items, dg=None, aux=()):
        self._items = items
        self._DG = dg
        self._aux = list(aux)       # traced graphs: (slice node, channels of it in this group), see graph.coupled_members

    def __iter__(self):
        return iter(self._items)

    def __len__(self):
        return len(self._items)

    def __getitem__(self, k):
        return self._items[k]

    def prune(self, idxs=None, record_history=True):
        """dependency.py:160-188: prune every member; the root goes into the graph's replayable pruning history as
        [root module name, is_out_channel_pruning, root indices]."""
        if idxs is not None:
            raise NotImplementedError('re-indexing an enumerated group: ask the graph for get_pruning_group(module, fn, idxs)')
        if not _prune_group_batched(self._items):
            for dep, ix in self._items:
                dep(ix)
        for node, n in self._aux:                  # the outputs of a torch.split shrink with the tensor that is split
            j, info = node.part
            info.sizes[j] -= n
        self._aux = []
        if record_history and self._DG is not None and self._items:
            root, ridx = self._items[0]
            self._DG._pruning_history.append([root.target.name, root.kind != 'in', [int(i) for i in ridx]])

    def details(self):
        return ['%s:%s(%d)' % (dep.kind, dep.target.name, len(idxs)) for dep, idxs in self._items]
PRUNE_BATCH = not os.environ.get('DP_NO_PRUNE_BATCH')
_BATCHED_KINDS = ('conv', 'linear', 'groupnorm')


def _prune_group_batched(items):
    """function.py:85-146,168-207,274-302 for ALL members of a group in one kernel launch (ops.slice_batch): every weight, bias
    and accumulated gradient keeps its un-pruned channels; the layers' channel attributes are updated as the per-member
    functions do.  Returns False (nothing touched) when a member is not a plain Conv2d / Linear / affine GroupNorm on the device
    (`_BATCHED_KINDS` rows of `_SLICING`), or when one tensor would be sliced twice in the group -- the caller then prunes member
    by member."""
    if not PRUNE_BATCH or not hasattr(ops, 'slice_batch') or not items:
        return False
    plan, seen = [], set()
    for dep, idxs in items:
        layer = dep.target.module
        if getattr(dep.handler, 'kind', None) not in _BATCHED_KINDS or getattr(layer, 'transposed', False) \
                or getattr(layer, 'groups', 1) != 1 or layer.weight is None:
            return False
        (attr,), dim, also = dep.handler.rule
        names = ['weight'] + [nm for nm in also if getattr(layer, nm, None) is not None]
        for nm in names:
            if (id(layer), nm) in seen or (getattr(layer, nm).device.type != 'cuda' and not getattr(ops, 'IS_MOCK', False)):
                return False          # host-side structure edits (history replay on a CPU model) slice member by member
            seen.add((id(layer), nm))
        plan.append((layer, dim, names, attr, idxs))
    keep_host, slices, assign, off_next = [], [], [], 0
    for layer, dim, names, attr, idxs in plan:
        n = getattr(layer, attr)
        mask = np.ones(n, dtype=bool)
        mask[np.asarray(idxs, dtype=np.int64)] = False
        keep = np.nonzero(mask)[0]
        if not len(keep):
            return False
        off = off_next
        off_next += len(keep)
        keep_host.append(keep)
        for nm in names:
            p = getattr(layer, nm)
            d = dim if nm == 'weight' else 0
            shp = list(p.shape)
            R = shp[0]
            Cc = shp[1] if len(shp) > 1 else 1
            T = 1
            for v in shp[2:]:
                T *= v
            new_shape = list(shp)
            new_shape[d] = len(keep)
            outs = []
            for src in (p.data, p.grad.data if p.grad is not None else None):
                if src is None:
                    outs.append(None)
                    continue
                dst = torch.empty(new_shape, dtype=src.dtype, device=src.device)
                slices.append((src.contiguous(), dst, R, Cc, T, d, len(keep), off))
                outs.append(dst)
            assign.append((layer, nm, outs[0], outs[1]))
    dev = plan[0][0].weight.device
    keep_dev = torch.from_numpy(np.concatenate(keep_host)).to(dev)
    ops.slice_batch(slices, keep_dev)
    for layer, nm, w, g in assign:
        newp = nn.Parameter(w)
        newp.grad = g
        layer._parameters[nm] = newp            # what Module.__setattr__ does for an existing parameter, minus its checks
    for layer, dim, names, attr, idxs in plan:
        object.__setattr__(layer, attr, getattr(layer, attr) - len(set(idxs)))
    return True


def _member_kind(dep):
    """Resolve 'out' / 'in' / 'gn' for this module's Dependency objects and for real torch_pruning ones."""
    k = getattr(dep, 'kind', None)
    if k is not None:
        return k
    fn = dep.handler
    owner = type(getattr(fn, '__self__', None)).__name__
    name = getattr(fn, '__name__', '')
    if 'LayerNorm' in owner or 'layernorm' in name:
        return 'ln'
    if 'GroupNorm' in owner or 'groupnorm' in name:
        return 'gn'
    if owner in ('ConvPruner', 'LinearPruner') or 'conv' in name or 'linear' in name:
        if 'out_channels' in name:
            return 'out'
        if 'in_channels' in name:
            return 'in'
    return None


# --------------------------------------------------------------------------------------------------------
# importance criteria
# --------------------------------------------------------------------------------------------------------
class Importance(abc.ABC):
    @abc.abstractmethod
    def __call__(self, group, ch_groups=1):
        raise NotImplementedError

    def score_all(self, groups, ch_groups=None):
        """Global pruning (metapruner.py:259-267): the score of EVERY group on the weights as they are now, one entry per group
        (None where the criterion has no term).  This form calls the criterion group by group."""
        chg = ch_groups if ch_groups is not None else [1] * len(groups)
        return [self(g, ch_groups=c) for g, c in zip(groups, chg)]


_MODES = {'sum_sq': 0, 'sum_abs': 1, 'abs_sum': 2}
_NO_TERM = ('ln', 'bn', 'inorm', 'prelu', 'embed')                     # member kinds the vendored criteria have no branch for
_OUT_KINDS = ('out', 'gn', 'ln', 'bn', 'inorm', 'prelu', 'embed')      # members pruned through an out-channel pruning function
_F_SQ, _F_ABS, _F_SIGNED, _F_GN_ABS, _F_GRAD_SQ, _F_SUM = 0, 1, 2, 3, 4, 5      # dp_wg_reduce modes (include/dp_hip.h)


class _MemberTable:
    """The member table of ops.group_score (one group) / ops.score_groups (every group): each member's reduction lands in a
    scratch vector shared by the table, an index-mapped member reads its channels through a shared index list."""

    def __init__(self):
        self.need, self.idx, self.dev = 0, [], None           # scratch floats, index entries, the device of the first member

    def add(self, members, n0):
        """Lay out one group of n0 channels.  members: (w, g, R, C, T, dim, (mode,), idxs) each -- a [R, C, T] view of w and g reduced
        in dp_wg_reduce `mode` to R values (dim 0, and mode 3) or C values (dim 1, through C * T column sums), of which `idxs`
        (ascending) are this group's; all of them in order when idxs is 0 .. n0 - 1 of an n0-channel layer.  Returns the kernels'
        member dicts, or None for a tensor the kernels cannot take (not contiguous, another device); an index outside the layer
        is refused."""
        out = []
        for w, g, R, Cc, T, dim, (mode,), idxs in members:
            self.dev = w.device if self.dev is None else self.dev
            if not (w.is_contiguous() and g.is_contiguous()) or w.device != self.dev or g.device != self.dev:
                return None
            cols = mode != _F_GN_ABS and dim == 1
            n_full = Cc if cols else R
            m = dict(w=w, g=g, R=R, C=Cc, T=T, dim=dim, mode=mode, full_off=0, col_off=0, idx_off=-1)
            m['col_off' if cols else 'full_off'] = self.need
            self.need += Cc * T if cols else n_full
            if not (n_full == n0 and idxs[0] == 0 and idxs[-1] == n0 - 1):
                if idxs[0] < 0 or idxs[-1] >= n_full:
                    raise IndexError('group member index outside its layer (%d channels)' % n_full)
                m['idx_off'] = len(self.idx)
                self.idx.extend(idxs)
            out.append(m)
        return out

    def index_tensor(self):
        return torch.from_numpy(np.asarray(self.idx, dtype=np.int64)).to(self.dev) if self.idx else None


class _Criterion(Importance):
    """The scoring core.  Every member that carries a term contributes the sum over its other dims of f(w, g) -- one dp_wg_reduce
    pass per mode of `conv_modes` (conv / linear members) or `gn_modes` (GroupNorm members; empty: they carry no term) -- members
    whose length differs from the root's are dropped (importance.py:422-426), the rest are summed at their channel positions, and
    `_finish` ends it: |.| when `final_abs`; the mean over the members and the division by the mean when `mean_finish`.
    `group_batched`: `__call__` scores a group through ops.group_score (else member by member)."""
    conv_modes = (_F_SQ,)
    gn_modes = (_F_ABS,)
    final_abs = False
    mean_finish = False
    group_batched = False

    def __init__(self, group_reduction='mean', normalizer='mean'):      # read only where mean_finish, as in the reference
        self.group_reduction, self.normalizer = group_reduction, normalizer
        self._scratch = None

    def _grown_scratch(self, need, dev):
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != dev:
            self._scratch = torch.empty(max(need, 1 << 16), dtype=torch.float32, device=dev)
        return self._scratch

    def _grad(self, layer):
        g = layer.weight.grad
        if g is None:
            raise RuntimeError('%s needs accumulated gradients (run the sweep before pruner.step())' % type(self).__name__)
        return g.data

    def _terms(self, group):
        """The members that carry a term: [(layer, kind, idxs)] in group order (each index list sorted in place)."""
        terms = []
        for dep, idxs in group:
            idxs.sort()
            kind = _member_kind(dep)
            if kind is None or kind in _NO_TERM:      # LayerNorm / BatchNorm / ... members carry no term (importance.py:383-418)
                continue
            layer = dep.target.module
            if kind == 'gn' and (not layer.affine or not self.gn_modes):
                continue
            terms.append((layer, kind, idxs))
        return terms

    def _desc(self, layer, kind):
        """-> (w, g, R, C, T, dim, modes): the member as dp_wg_reduce sees it."""
        w, g = layer.weight.data, self._grad(layer)
        if kind == 'gn':
            return w, g, w.shape[0], 1, 1, 0, self.gn_modes
        dim = 0 if kind == 'out' else 1
        if getattr(layer, 'transposed', False):        # ConvTranspose: weight [Cin, Cout, k, k] (importance.py:390-392,404-406)
            dim = 1 - dim
        T = 1
        for v in w.shape[2:]:
            T *= v
        return w, g, w.shape[0], w.shape[1] if w.dim() > 1 else 1, T, dim, self.conv_modes

    def _members(self, terms, n0):
        for layer, kind, idxs in terms:
            if len(idxs) == n0:
                yield self._desc(layer, kind) + (idxs,)

    @property
    def _batchable(self):
        """One reduction per member: a member that accumulates two modes (FullTaylorImportance(order=2)) adds them BEFORE the
        member sum, which the one-pass member table cannot express bit for bit -> scored member by member."""
        return len(self.conv_modes) == 1 and len(self.gn_modes) <= 1

    def _score_members(self, terms, n0, dev):
        """Member by member: ops.wg_reduce per mode, then ops.axpby (all channels in order) or ops.gather_add."""
        score, used = torch.zeros(n0, dtype=torch.float32, device=dev), 0
        for w, g, R, Cc, T, dim, modes, idxs in self._members(terms, n0):
            n_full = Cc if dim == 1 else R
            full = torch.empty(n_full, dtype=torch.float32, device=w.device)
            scratch = self._grown_scratch(Cc * T, w.device) if dim == 1 else None
            w, g = w.contiguous(), g.contiguous()
            if modes != (_F_GN_ABS,):                   # mode 3 takes the 1-D GroupNorm weight as it is
                w, g = w.view(R, Cc, T), g.view(R, Cc, T)
            for i, mode in enumerate(modes):
                ops.wg_reduce(w, g, dim, mode, full, i > 0, scratch)
            if n_full == n0 and idxs[0] == 0 and idxs[-1] == n0 - 1:
                ops.axpby(full, 1.0, score, 1.0)
            else:
                ops.gather_add(full, _index_tensor(('idx', tuple(idxs)), lambda: idxs, dev), score)
            used += 1
        return score, used

    def _score_group(self, terms, n0):
        """All members of the group through ops.group_score (two launches): the same per-member reductions in the same member
        order as `_score_members`, hence the same bits.  Returns (score, members used) or None (not applicable)."""
        table = _MemberTable()
        members = table.add(self._members(terms, n0), n0)
        if not members:
            return None
        score = torch.empty(n0, dtype=torch.float32, device=table.dev)
        ops.group_score(members, n0, table.index_tensor(), self._grown_scratch(table.need, table.dev), score)
        return score, len(members)

    def _finish(self, score, used):
        if self.final_abs:           # |score|: signed row "sum" over one column with the abs-after-sum mode
            out = torch.empty_like(score)
            ops.wg_reduce(score.view(-1, 1), torch.ones_like(score).view(-1, 1), 0, _F_SIGNED, out, False)
            score = out
        if self.mean_finish:
            if self.group_reduction == 'mean':
                ops.axpby(score, 0.0, score, 1.0 / used)
            if self.normalizer == 'mean':
                mean = float(score.mean())
                ops.axpby(score, 0.0, score, 1.0 / mean)
        return score

    @torch.no_grad()
    def __call__(self, group, ch_groups=1):
        terms = self._terms(group)
        if not terms:
            return None
        n0 = len(terms[0][2])
        batched = self.group_batched and self._batchable and PRUNE_BATCH and hasattr(ops, 'group_score')
        got = self._score_group(terms, n0) if batched else None            # None: member by member
        return self._finish(*(got or self._score_members(terms, n0, terms[0][0].weight.device)))

    @torch.no_grad()
    def score_all(self, groups, ch_groups=None):
        """Every group's member reductions and member sums in ONE launch pair (ops.score_groups, csrc/prune_global.hip): the member
        table of `_score_group` with ONE scratch / index / score vector shared by all groups -- the same per-member reductions in
        the same member order as `__call__`, hence the same bits -- then the same per-group finish.  Where that is not applicable
        (no batched kernels, two reductions per member, a tensor the kernels cannot take) the criterion is called group by group."""
        if not PRUNE_BATCH or not hasattr(ops, 'score_groups') or not self._batchable:
            return super().score_all(groups, ch_groups)
        table, per_group = _MemberTable(), []
        for group in groups:
            terms = self._terms(group)
            n0 = len(terms[0][2]) if terms else 0
            members = table.add(self._members(terms, n0), n0)
            if members is None:
                return super().score_all(groups, ch_groups)
            per_group.append((members, n0) if terms else None)
        live = [pg for pg in per_group if pg is not None]
        if not live:
            return [None] * len(groups)
        scores = torch.empty(sum(n0 for _, n0 in live), dtype=torch.float32, device=table.dev)
        ops.score_groups(live, table.index_tensor(), self._grown_scratch(table.need, table.dev), scores)
        out, off = [], 0
        for pg in per_group:
            if pg is None:
                out.append(None)
                continue
            members, n0 = pg
            part = scores[off:off + n0]
            out.append(self._finish(part.clone() if self.mean_finish else part, len(members)))      # normalised in place: a tensor of its own
            off += n0
        return out


class TaylorImportance(_Criterion):
    """First-order Taylor importance on the device.

    multivariable=None  -> the reference's vendored criterion (importance.py:375-434): conv/linear members
                           contribute sum((w*g)^2) over the other dims, GroupNorm members |w*g|, members whose length
                           differs from the root's are dropped, plain sum over members, no normalisation ('sum_sq').
    multivariable=True / False -> the pip torch_pruning criterion named by ddpm_prune.py:60,66: |sum w*g| / sum |w*g|
                           per member, mean over members, mean-normalised (that package is absent from the reference
                           tree and unpinned in requirements.txt:7: PARITY UNPINNED for these two modes).
    groupnorm_term      -> whether GroupNorm members add |w*g|.  The vendored criterion has that branch
                           (importance.py:412-418) -> default True for multivariable=None.  The pip criterion of that
                           era only had a BatchNorm branch (prune_batchnorm_out_channels), GroupNorm members matched no
                           branch and added nothing -> default False for the multivariable modes (recalled, unpinned).
    `sweep.prune_model` defaults to the vendored ('sum_sq') criterion: the only one pinned by reference outputs.
    Of `group_reduction` and `normalizer` this class honours only 'mean' (any other value leaves the member sum as it is)."""
    group_batched = True

    def __init__(self, group_reduction='mean', normalizer='mean', multivariable=None, groupnorm_term=None):
        super().__init__(group_reduction, normalizer)
        self.multivariable = multivariable
        self.mode = 'sum_sq' if multivariable is None else ('abs_sum' if multivariable else 'sum_abs')
        self.groupnorm_term = (multivariable is None) if groupnorm_term is None else bool(groupnorm_term)
        self.conv_modes = (_MODES[self.mode],)
        self.gn_modes = (_F_GN_ABS,) if self.groupnorm_term else ()
        self.mean_finish = multivariable is not None


class FullTaylorImportance(_Criterion):
    """importance.py:482-548: order 1: sum w*g; order 2: sum w*g + sum (w*g)^2; |.| after the members are summed."""
    final_abs = True

    def __init__(self, order=1, group_reduction='mean', normalizer='mean'):
        super().__init__(group_reduction, normalizer)
        if order not in (1, 2):
            raise ValueError('order must be 1 or 2')
        self.order = order
        self.conv_modes = (_F_SUM,) if order == 1 else (_F_SUM, _F_SQ)
        self.gn_modes = self.conv_modes


class AbsTaylorImportance(_Criterion):
    """importance.py:611-670: sum |w*g| per member, plain sum over members."""
    conv_modes = (_F_ABS,)
    gn_modes = (_F_ABS,)

    def __init__(self, order=1, group_reduction='mean', normalizer='mean'):
        super().__init__(group_reduction, normalizer)


class FisherImportance(_Criterion):
    """importance.py:715-781: conv / linear members sum g^2, GroupNorm members (w*g)^2."""
    conv_modes = (_F_GRAD_SQ,)
    gn_modes = (_F_SQ,)


_REDUCTIONS = ('sum', 'mean', 'max', 'prod', 'first')
_NORMALIZERS = (None, 'sum', 'standarization', 'mean', 'max', 'gaussian')        # the reference's spellings


class MagnitudeImportance(_Criterion):
    """importance.py:18-126: sum |w|^p per conv / linear member (GroupNorm members carry no term: the vendored class only
    matches BatchNorm; members whose length differs from the first term's are dropped), `group_reduction` over the members
    ('sum' | 'mean' | 'max' | 'prod' | 'first'), then `normalizer` (None | 'sum' | 'standarization' | 'mean' | 'max' | 'gaussian' |
    a callable applied to each group's device tensor).  Any p > 0.  Divisions are the IEEE ones: an all-zero group under 'mean'
    scores NaN, as it does there.

    The configuration (2, 'mean', 'mean') runs where it always ran: the fused reduction with g := w (|w*w| = |w|^2) and the
    core's mean finish.  Every other one runs on csrc/magnitude.hip: one member launch (ops.magnitude_rows) and one finish launch
    (ops.magnitude_finish) for ALL groups handed to `score_all` (for the one group of `__call__`), no device-to-host read.
    DP_NO_PRUNE_BATCH, host tensors, a callable normaliser or a group wider than ops.MAGNITUDE_MAX_WIDTH take the reference's
    expressions in torch on the device the weights are on, group by group."""
    conv_modes = (_F_ABS,)
    gn_modes = ()
    mean_finish = True
    root = False              # members are (sum |w|^p)^(1/p)
    lamp = None               # None | 'vendored' | 'paper'
    sort_indices = True       # importance.py:65 sorts every index list of the group in place
    length_filter = True      # importance.py:118-122

    def __init__(self, p=2, group_reduction='mean', normalizer='mean'):
        super().__init__(group_reduction, normalizer)
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not p > 0:
            raise ValueError('%s: p must be a number > 0, got %r' % (type(self).__name__, p))
        if group_reduction is None:
            raise ValueError('group_reduction=None leaves one row per member: no pruner can rank that')
        if group_reduction not in _REDUCTIONS:
            raise NotImplementedError('group_reduction %r (known: %s)' % (group_reduction, ', '.join(_REDUCTIONS)))
        if not callable(normalizer) and normalizer not in _NORMALIZERS:
            raise NotImplementedError('normalizer %r (known: %s, or a callable)' % (normalizer, ', '.join(map(str, _NORMALIZERS))))
        self.p = p
        self._held = None

    def _grad(self, layer):
        return layer.weight.data

    @property
    def _present_path(self):
        return type(self) is MagnitudeImportance and self.p == 2 and self.group_reduction == 'mean' and self.normalizer == 'mean'

    @property
    def scores_stay_on_device(self):
        """prune_global keeps this criterion's scores where they are (its records hold device slices)."""
        return not self._present_path

    def _mag_members(self, group):
        """-> (n0, [(w, R, C, T, dim, idxs)]) of the members that carry a term, or None.  len(idxs) is n0, or for an in-channel
        member of LAMPImportance a multiple of it (`_kernel_scores` / `_torch_score` fold it)."""
        members, kinds = [], []
        for dep, idxs in group:
            if self.sort_indices:
                idxs.sort()
            kind = _member_kind(dep)
            if kind not in ('out', 'in'):
                continue
            layer = dep.target.module
            w = layer.weight.data
            dim = 0 if kind == 'out' else 1
            if getattr(layer, 'transposed', False):        # ConvTranspose: weight [Cin, Cout, k, k]
                dim = 1 - dim
            T = 1
            for v in w.shape[2:]:
                T *= v
            R, Cc = w.shape[0], w.shape[1] if w.dim() > 1 else 1
            if len(idxs) and (min(idxs) < 0 or max(idxs) >= (Cc if dim else R)):
                raise IndexError('group member index outside its layer (%d channels)' % (Cc if dim else R))
            members.append((w, R, Cc, T, dim, idxs))
            kinds.append(kind)
        if not members:
            return None
        n0 = len(members[0][5])
        if self.length_filter:
            members = [m for m in members if len(m[5]) == n0]
        elif any(len(m[5]) != n0 and (k != 'in' or n0 == 0 or len(m[5]) % n0 or not m[5]) for m, k in zip(members, kinds)):
            # importance.py:188-195 views an in-channel member of k * n0 channels as [n0, k, .]; anything else fails in view / torch.stack
            raise RuntimeError('%s: the members of the group rooted at %s differ in length (%s)' % (
                type(self).__name__, getattr(group[0][0].target, 'name', '?'), sorted({len(m[5]) for m in members})))
        return n0, members

    def _on_kernels(self, live):
        """Per group of `live`: whether the kernels take it (a group above the cap goes to torch on its own, the rest stay batched)."""
        if not PRUNE_BATCH or not hasattr(ops, 'magnitude_rows') or callable(self.normalizer):
            return [False] * len(live)
        dev = live[0][1][0][0].device
        if dev.type != 'cuda' and not getattr(ops, 'IS_MOCK', False):
            return [False] * len(live)
        return [n0 <= ops.MAGNITUDE_MAX_WIDTH and all(m[0].device == dev and m[0].dtype == torch.float32 and m[0].is_contiguous() for m in ms)
                for n0, ms in live]

    def _kernel_scores(self, live):
        """The member table and the group table of every group in `live`; two launches; -> one score view per group."""
        members, groups, idx, row = [], [], [], 0
        dev = live[0][1][0][0].device
        for n0, ms in live:
            groups.append((row, n0, len(ms)))
            for w, R, Cc, T, dim, idxs in ms:
                idx_off = -1
                if not ((Cc if dim else R) == n0 == len(idxs) and all(i == j for j, i in enumerate(idxs))):
                    idx_off = len(idx)
                    idx.extend(idxs)
                members.append(dict(w=w, R=R, C=Cc, T=T, dim=dim, n0=n0, idx_off=idx_off, row_off=row, fold=len(idxs) // n0))
                row += n0
        rows = torch.empty(row, dtype=torch.float32, device=dev)
        scores = torch.empty(sum(n0 for n0, _ in live), dtype=torch.float32, device=dev)
        idx_dev = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev) if idx else None
        ops.magnitude_rows(members, idx_dev, self.p, self.root, rows)
        ops.magnitude_finish(groups, rows, self.group_reduction, self.normalizer, self.lamp, scores)
        self._held = (rows, scores, idx_dev)          # the launchers' tables live on these until the next call
        out, off = [], 0
        for n0, _ in live:
            out.append(scores[off:off + n0])
            off += n0
        return out

    def _torch_score(self, n0, ms):
        """importance.py:59-126 / :161-219 in torch, in the dtype and on the device of the weights."""
        rows = []
        for w, R, Cc, T, dim, idxs in ms:
            m = w.reshape(R, Cc * T) if dim == 0 else w.reshape(R, Cc, T).transpose(0, 1).reshape(Cc, R * T)
            m = m[torch.as_tensor(idxs, dtype=torch.long, device=w.device)]
            if len(idxs) != n0:                            # importance.py:188-195: k consecutive channels of the list make one
                m = m.reshape(n0, -1)
            rows.append(torch.norm(m, dim=1, p=self.p) if self.root else m.abs().pow(self.p).sum(1))
        imp, red, norm = torch.stack(rows, dim=0), self.group_reduction, self.normalizer
        imp = {'sum': lambda: imp.sum(dim=0), 'mean': lambda: imp.mean(dim=0), 'max': lambda: imp.max(dim=0)[0],
               'prod': lambda: torch.prod(imp, dim=0), 'first': lambda: imp[0]}[red]()
        if callable(norm):
            imp = norm(imp)
        elif norm is not None:
            imp = {'sum': lambda: imp / imp.sum(), 'standarization': lambda: (imp - imp.min()) / (imp.max() - imp.min() + 1e-8),
                   'mean': lambda: imp / imp.mean(), 'max': lambda: imp / imp.max(),
                   'gaussian': lambda: (imp - imp.mean()) / (imp.std() + 1e-8)}[norm]()
        if self.lamp is None:
            return imp
        a = torch.argsort(imp, dim=0, descending=True, stable=True)
        q = imp[a]
        q = q / torch.cumsum(q, dim=0)
        if self.lamp == 'vendored':
            return q[a]
        out = torch.empty_like(q)
        out[a] = q
        return out

    def _score(self, groups):
        per = [self._mag_members(g) for g in groups]
        live = [x for x in per if x is not None]
        if not live:
            return [None] * len(groups)
        taken = self._on_kernels(live)
        batched = iter(self._kernel_scores([x for x, t in zip(live, taken) if t]) if any(taken) else ())
        got = iter([next(batched) if t else self._torch_score(n0, ms) for (n0, ms), t in zip(live, taken)])
        return [None if x is None else next(got) for x in per]

    @torch.no_grad()
    def __call__(self, group, ch_groups=1):
        if self._present_path:
            return super().__call__(group, ch_groups)
        return self._score([group])[0]

    @torch.no_grad()
    def score_all(self, groups, ch_groups=None):
        if self._present_path:
            return super().score_all(groups, ch_groups)
        return self._score(groups)


class LAMPImportance(MagnitudeImportance):
    """importance.py:154-219: members are torch.norm(., p) per channel = (sum |w|^p)^(1/p), the same reduction and normaliser,
    then `lamp`: with a = the descending argsort of the scores and q = sorted / cumsum(sorted), the vendored code returns q[a]
    (`torch.arange(n)[a]` is a itself, not its inverse) -- the default, because masks are pinned to the reference; paper_order=True
    scatters with the true inverse (out[a[k]] = q[k]), the score of arXiv 2010.07611.  Ties sort by ascending channel.  As there, the
    index lists are not sorted and no member is dropped.  An in-channel member that holds the group's channels k times over (both
    halves of a concatenation come from the group) is viewed as [n0, k, .], k consecutive entries of its list to a channel, as
    importance.py:188-195 does; any other difference in length raises RuntimeError naming the root layer (there: torch.stack / view)."""
    root = True
    sort_indices = False
    length_filter = False

    def __init__(self, p=2, group_reduction='mean', normalizer='mean', paper_order=False):
        super().__init__(p, group_reduction, normalizer)
        self.paper_order = bool(paper_order)
        self.lamp = 'paper' if paper_order else 'vendored'


class RandomImportance(Importance):
    @torch.no_grad()
    def __call__(self, group, ch_groups=1):
        return torch.rand(len(group[0][1]))


importance = SimpleNamespace(Importance=Importance, TaylorImportance=TaylorImportance,
                             FullTaylorImportance=FullTaylorImportance, AbsTaylorImportance=AbsTaylorImportance,
                             FisherImportance=FisherImportance,
                             MagnitudeImportance=MagnitudeImportance, LAMPImportance=LAMPImportance,
                             RandomImportance=RandomImportance)


# --------------------------------------------------------------------------------------------------------
# pruner
# --------------------------------------------------------------------------------------------------------
def linear_scheduler(ch_sparsity, steps):
    return [((i) / float(steps)) * ch_sparsity for i in range(steps + 1)]


class DependencyGraph:
    """Group enumeration (dependency.py:259-527).  For the two model families of this package the op graph is written
    down from the model configuration (graph.py); any other module is traced through autograd with `example_inputs`
    (trace.py), as `tp.DependencyGraph().build_dependency(model, example_inputs=...)` does."""

    def __init__(self, model=None, example_inputs=None, forward_fn=None, output_transform=None):
        self._pruning_history = []
        if model is not None:
            self.build_dependency(model, example_inputs, forward_fn, output_transform)

    def build_dependency(self, model, example_inputs=None, forward_fn=None, output_transform=None):
        """dependency.py:295-383.  Returns self."""
        self.model = model
        cfg = getattr(model, 'config', None)
        cfg = dict(cfg) if cfg is not None and hasattr(cfg, 'keys') else {}
        # The written-down graphs are for exactly two architectures (this package's classes or the reference's own of the same
        # name); anything else -- including other Diffusers models that share config keys -- is traced.
        cls = type(model).__name__
        if cls == 'UNetModel' and 'model_channels' in cfg:
            self.graph = LdmGraph(cfg)
        elif cls == 'UNet2DModel' and 'block_out_channels' in cfg and 'down_block_types' in cfg:
            self.graph = UNetGraph(cfg)
        else:
            if example_inputs is None:
                raise ValueError('example_inputs are needed to trace %s' % type(model).__name__)
            from .trace import TracedGraph
            self.graph = TracedGraph(model, example_inputs, forward_fn, output_transform)
        self.name2module = dict(model.named_modules())
        self.module2name = {m: n for n, m in self.name2module.items()}
        return self

    def pruning_history(self):
        """dependency.py:278-279: [[root module name, is_out_channel_pruning, idxs], ...] in application order."""
        return self._pruning_history

    def load_pruning_history(self, pruning_history):
        """dependency.py:281-293: replay a recorded history on this (un-pruned) model -- structure only, no gradients
        needed; afterwards the parameter shapes match the pruned checkpoint."""
        self._pruning_history = [[n, bool(o), [int(i) for i in ix]] for n, o, ix in pruning_history]
        for name, is_out, idxs in self._pruning_history:
            if not is_out:
                raise NotImplementedError('in-channel roots do not occur in histories written by the prune scripts')
            module = self.name2module[name]
            self.get_pruning_group(module, _handler_for(module, 'out'), idxs).prune(record_history=False)

    def _chan(self):
        n2m = self.name2module
        return ChannelView(lambda name: _out_channels(n2m[name]))

    def _group(self, members, aux=()):
        return Group([(Dependency(self.name2module[m.name], m.name, m.kind), list(m.idxs)) for m in members], self, aux)

    def get_pruning_group(self, module, pruning_fn, idxs):
        name = self.module2name[module]
        aux = []
        return self._group(coupled_members(self.graph, self._chan(), name, list(idxs), aux), aux)

    def get_all_groups(self, ignored_layers=(), root_module_types=(nn.Conv2d, nn.Linear)):
        ignored = tuple(self.module2name[m] for m in ignored_layers if m in self.module2name)
        for _, members in all_groups(self.graph, self._chan, ignored):
            yield self._group(members)

    def check_pruning_group(self, group):
        for dep, idxs in group:
            n = _out_channels(dep.target.module) if dep.kind in _OUT_KINDS else _in_channels(dep.target.module)
            if n is None:                        # a PReLU with one shared slope has no channel count
                continue
            if n <= len(idxs):
                return False
        return True

    get_out_channels = staticmethod(_out_channels)
    get_in_channels = staticmethod(_in_channels)


class MetaPruner:
    """metapruner.py:11-297: the local pruning path the reference's scripts use (`prune_local`) and, with
    `global_pruning=True`, one ranking across every group of the network (`prune_global`)."""

    def __init__(self, model, example_inputs=None, importance=None, global_pruning=False, ch_sparsity=0.5,
                 ch_sparsity_dict=None, max_ch_sparsity=1.0, iterative_steps=1,
                 iterative_sparsity_scheduler=linear_scheduler, ignored_layers=None, channel_groups=None, round_to=None,
                 root_module_types=(nn.Conv2d, nn.Linear)):
        self.model, self.importance, self.global_pruning = model, importance, bool(global_pruning)
        self.ch_sparsity, self.max_ch_sparsity = ch_sparsity, max_ch_sparsity
        self.round_to, self.root_module_types = round_to, root_module_types
        self.channel_groups = dict(channel_groups) if channel_groups else {}
        self.DG = DependencyGraph(model, example_inputs)
        self.ignored_layers = []
        for layer in (ignored_layers or []):
            self.ignored_layers.extend(list(layer.modules()))
        self.iterative_steps, self.current_step = iterative_steps, 0
        self.layer_init_out_ch, self.layer_init_in_ch = {}, {}
        for m in model.modules():
            if isinstance(m, (nn.modules.conv._ConvNd, nn.Linear, nn.GroupNorm, nn.LayerNorm, nn.modules.batchnorm._BatchNorm,
                              nn.modules.instancenorm._InstanceNorm, nn.PReLU, nn.Embedding)) and _out_channels(m) is not None:
                self.layer_init_out_ch[m] = _out_channels(m)
                self.layer_init_in_ch[m] = _in_channels(m)
        self.per_step_ch_sparsity = iterative_sparsity_scheduler(ch_sparsity, iterative_steps)
        self.ch_sparsity_dict = {}
        for module, sp in (ch_sparsity_dict or {}).items():
            for sub in module.modules():
                if isinstance(sub, (nn.Conv2d, nn.Linear, nn.GroupNorm)):
                    self.ch_sparsity_dict[sub] = iterative_sparsity_scheduler(sp, iterative_steps)
        for m in model.modules():                       # metapruner.py:118-124
            if isinstance(m, nn.GroupNorm):
                self.channel_groups[m] = m.num_groups
        self.records = []          # per pruned group: (root name, ch_groups, score tensor, pruned idxs) for reporting
        self.global_threshold = None
        if self.global_pruning:                         # metapruner.py:126-133
            self.initial_total_channels = 0
            for group in self.DG.get_all_groups(self.ignored_layers, self.root_module_types):
                self.initial_total_channels += _out_channels(group[0][0].target.module) // self.get_channel_groups(group)

    def get_target_sparsity(self, layer):
        return self.ch_sparsity_dict.get(layer, self.per_step_ch_sparsity)[self.current_step]

    def reset(self):
        self.current_step = 0

    def step(self, interactive=False):
        self.current_step += 1
        if self.global_pruning:
            if interactive:
                return self.prune_global()
            for group in self.prune_global():
                group.prune()
            return
        if interactive:
            return self.prune_local()
        for group in self.prune_local():
            group.prune()

    def pruning_history(self):
        return self.DG.pruning_history()

    def load_pruning_history(self, pruning_history):
        self.DG.load_pruning_history(pruning_history)

    def estimate_importance(self, group, ch_groups=1):
        return self.importance(group, ch_groups=ch_groups)

    def _check_sparsity(self, group):
        for dep, _ in group:
            m = dep.target.module
            if m not in self.layer_init_out_ch:
                continue                             # e.g. a PReLU with one shared slope
            if dep.kind in _OUT_KINDS:
                n = _out_channels(m)
                if n < self.layer_init_out_ch[m] * (1 - self.max_ch_sparsity) or n == 1:
                    return False
            else:
                n = _in_channels(m)
                if n < self.layer_init_in_ch[m] * (1 - self.max_ch_sparsity) or n == 1:
                    return False
        return True

    def get_channel_groups(self, group):
        if isinstance(self.channel_groups, int):
            return self.channel_groups
        for dep, _ in group:
            if dep.target.module in self.channel_groups:
                return self.channel_groups[dep.target.module]
        return 1

    def prune_local(self):
        if self.current_step > self.iterative_steps:
            return
        for group in self.DG.get_all_groups(self.ignored_layers, self.root_module_types):
            if not self._check_sparsity(group):
                continue
            module = group[0][0].target.module
            fn = group[0][0].handler
            ch_groups = self.get_channel_groups(group)
            imp = self.estimate_importance(group, ch_groups=ch_groups)
            if imp is None:
                continue
            cur = _out_channels(module)
            n_pruned = cur - int(self.layer_init_out_ch[module] * (1 - self.get_target_sparsity(module)))
            if self.round_to:
                n_pruned = n_pruned - (n_pruned % self.round_to)
            if n_pruned <= 0:
                continue
            imp_host = imp.detach().float().cpu()          # <= 1024 scores: argsort on the host (metapruner.py:237-249)
            if ch_groups > 1:
                gs = cur // ch_groups
                per = n_pruned // ch_groups
                order = torch.argsort(imp_host[:gs * ch_groups].view(ch_groups, gs), dim=1)[:, :per]
                idxs = (order + torch.arange(ch_groups).view(-1, 1) * gs).reshape(-1)
            else:
                idxs = torch.argsort(imp_host)[:(n_pruned // ch_groups)]
            idxs = idxs.tolist()
            pg = self.DG.get_pruning_group(module, fn, idxs)
            if self.DG.check_pruning_group(pg):
                self.records.append((group[0][0].target.name, ch_groups, imp_host, sorted(idxs)))
                yield pg

    def prune_global(self):
        """metapruner.py:256-297, quirks included: every group is scored on the UNPRUNED weights (of a head / GroupNorm-grouped
        root only the first sub-group's scores are ranked), the kept scores are concatenated in group order, the threshold is the
        n_pruned-th smallest of them, and each group loses the channels whose score is <= the threshold (ties at the threshold all
        go; a group may lose none, and is still yielded).  Scores: one launch pair for all groups (`importance.score_all`); the
        selection and the per-group index lists: `ops.select_smallest`, one device-to-host copy.  Without the batched kernels
        (DP_NO_PRUNE_BATCH, a criterion that cannot batch, host tensors) the same arithmetic runs group by group / through
        torch.topk.  `records` rows hold the RANKED scores (the first sub-group's for a grouped root)."""
        if self.current_step > self.iterative_steps:
            return
        groups, chg = [], []
        for group in self.DG.get_all_groups(self.ignored_layers, self.root_module_types):
            if self._check_sparsity(group):
                groups.append(group)
                chg.append(self.get_channel_groups(group))
        if PRUNE_BATCH and hasattr(self.importance, 'score_all'):
            imps = self.importance.score_all(groups, chg)
        else:
            imps = [self.estimate_importance(g, ch_groups=c) for g, c in zip(groups, chg)]
        ranked = []
        for group, ch_groups, imp in zip(groups, chg, imps):
            if imp is None:
                continue
            if ch_groups > 1:
                imp = imp[:len(imp) // ch_groups]
            ranked.append((group, ch_groups, imp))
        if not ranked:
            return
        imp = torch.cat([r[-1] for r in ranked], dim=0)
        n_pruned = len(imp) - int(self.initial_total_channels * (1 - self.per_step_ch_sparsity[self.current_step]))
        if n_pruned <= 0:
            return
        offsets = [0]
        for r in ranked:
            offsets.append(offsets[-1] + len(r[-1]))
        on_device = imp.is_cuda or getattr(ops, 'IS_MOCK', False)
        select = PRUNE_BATCH and hasattr(ops, 'select_smallest') and on_device and all(a < b for a, b in zip(offsets, offsets[1:]))
        # a criterion that scores on the device without a read (csrc/magnitude.hip) keeps its scores there: the selection's one copy is the only one
        stay = select and getattr(self.importance, 'scores_stay_on_device', False)
        imp_host = imp.detach() if stay else imp.detach().float().cpu()
        if select:
            thres, picked = ops.select_smallest(imp.detach().float().contiguous(), offsets, n_pruned)
        else:
            topk_imp, _ = torch.topk(imp_host, k=n_pruned, largest=False)
            thres = float(topk_imp[-1])
            picked = [(imp_host[a:b] <= topk_imp[-1]).nonzero().view(-1).numpy() for a, b in zip(offsets, offsets[1:])]
        self.global_threshold = thres
        for (group, ch_groups, _), idxs, a, b in zip(ranked, picked, offsets, offsets[1:]):
            module = group[0][0].target.module
            fn = group[0][0].handler
            idxs = [int(i) for i in idxs]
            if ch_groups > 1:
                gs = _out_channels(module) // ch_groups
                idxs = [i + gs * c for c in range(ch_groups) for i in idxs]
            if self.round_to:
                idxs = idxs[:len(idxs) - (len(idxs) % self.round_to)]
            pg = self.DG.get_pruning_group(module, fn, idxs)
            if self.DG.check_pruning_group(pg):
                self.records.append((group[0][0].target.name, ch_groups, imp_host[a:b], sorted(idxs)))
                yield pg


MagnitudePruner = MetaPruner
pruner = SimpleNamespace(MetaPruner=MetaPruner, MagnitudePruner=MagnitudePruner)
utils = None        # filled below (count_ops_and_params is defined after the pruner classes)


def fix_static_attributes(model):
    """ddpm_prune.py:111-116: Up/Downsample2D keep a `channels` attribute their forward asserts on."""
    for m in model.modules():
        if hasattr(m, 'channels') and hasattr(m, 'conv') and isinstance(m.conv, nn.Conv2d):
            m.channels = m.conv.in_channels


def prune_every_step(model, importance=None, iterative_steps=1, **pruner_args):
    """What the prune scripts do after the importance pass (ddpm_prune.py:79-116, prune_ldm.py:70-100): build the pruner (the
    vendored Taylor criterion unless one is given), prune every group each `step()` yields, then fix the static `channels`
    attributes and drop the engine's weight packs, which describe the old shapes.  Returns the pruner."""
    pr = MagnitudePruner(model, None, importance=importance if importance is not None else TaylorImportance(),
                         iterative_steps=iterative_steps, **pruner_args)
    for _ in range(iterative_steps):
        for g in pr.step(interactive=True):
            g.prune()
    fix_static_attributes(model)
    if getattr(model, '_engine', None) is not None:
        model._engine.packs.clear()
    return pr


def count_ops_and_params(model, example_inputs=None):
    """`tp.utils.count_ops_and_params(model, example_inputs)` (ddpm_prune.py:89,118, ddpm_sample.py:51) for UNet2DModel:
    returns (MACs-style count per image, parameter count) with the vendored counter's conventions
    (utils/op_counter.py:53-101,248-298): Conv2d = k*k*Cin*Cout*positions + Cout*positions (bias), Linear =
    numel(input)*out + out (bias, once), GroupNorm = 2*numel(input); activations, interpolation and the attention
    matmuls are not counted.  The reference obtains the shapes with forward hooks; here they follow from the block
    structure (this model has no PyTorch forward to hook).  `example_inputs` only supplies the spatial size."""
    cfg = getattr(model, 'config', None)
    if cfg is None or 'block_out_channels' not in cfg:
        raise NotImplementedError('count_ops_and_params is implemented for UNet2DModel')
    H = W = cfg['sample_size'] if isinstance(cfg['sample_size'], int) else None
    if H is None:
        H, W = cfg['sample_size']
    if example_inputs is not None:
        x = example_inputs['sample'] if isinstance(example_inputs, dict) else example_inputs[0]
        H, W = int(x.shape[-2]), int(x.shape[-1])
    levels = len(cfg['block_out_channels'])

    def hw(level):
        return (H >> level) * (W >> level)

    def positions(name, module):
        p = name.split('.')
        if p[0] == 'down_blocks':
            lvl = int(p[1])
            return hw(lvl + 1) if p[2] == 'downsamplers' else hw(lvl)
        if p[0] == 'up_blocks':
            lvl = levels - 1 - int(p[1])
            return hw(lvl - 1) if p[2] == 'upsamplers' else hw(lvl)
        if p[0] == 'mid_block':
            return hw(levels - 1)
        return H * W                                            # conv_in, conv_norm_out, conv_out

    total = 0
    for name, m in model.named_modules():
        if isinstance(m, nn.Conv2d):
            pos = positions(name, m)
            total += m.kernel_size[0] * m.kernel_size[1] * m.in_channels * m.out_channels * pos
            if m.bias is not None:
                total += m.out_channels * pos
        elif isinstance(m, nn.Linear):
            tokens = positions(name, m) if '.attentions.' in name else 1      # q/k/v/out see [1, T, C]; the rest [1, C]
            total += tokens * m.in_features * m.out_features + (m.out_features if m.bias is not None else 0)
        elif isinstance(m, nn.GroupNorm):
            total += 2 * m.num_channels * positions(name, m)
    return float(total), count_params(model)


def count_params(model):
    return sum(p.numel() for p in model.parameters())


utils = SimpleNamespace(count_ops_and_params=count_ops_and_params, count_params=count_params)
