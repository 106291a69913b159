"""The ops-level calls pruning makes, pinned (`-m "not gpu"`): on the CPU stand-ins of tests/mock_ops_prune_global.py every call of
wg_reduce / axpby / gather_add / group_score / score_groups / select_smallest / slice_batch is recorded in order with its scalar
arguments (R, C, T, dim, mode, accumulate, offsets, n0, index lists, k) and a hash of the bytes it produced, for every criterion, local
and global pruning, PRUNE_BATCH on and off, on the tiny UNet and on two traced toy networks (`generator`: ConvTranspose, InstanceNorm,
PReLU, Embedding and the index-mapped Linear -> view members; `plain_cnn`: BatchNorm and the flatten index map -- no single toy network
has a ConvTranspose AND a BatchNorm), and on a hand-made group with a member index outside its layer.  The kept-channel lists of
slice_batch are held by length and hash (written out they alone would pass the size limit of a committed file); each run ends in a
`pruned` record (roots, index lists, hash of the scores) or a `raised` one.  tests/golden/prune_score_calls.json holds, per case,
the number of records, the number of each call and a running hash over the records read out every 16 of them (`summarise`: the
17 000 records written out are three quarters of a megabyte); tests/golden/make_prune_score_calls.py writes it, and with `--full`
writes every record, to compare two commits record by record.  A refactor of pruning.py leaves the fixture as it is.

Recorded on the commit before pruning.py was folded onto one scoring core, then changed in exactly five cases: the four
`generator/magnitude/*` runs raised IndexError there (MagnitudeImportance ignored `layer.transposed`, so the ConvTranspose member was
reduced along the wrong dimension) and now score and prune; `out_of_range/call/batch` reached group_score with the bad index there and
is now refused before the call.

The hashes are of fp32 bytes computed by host arithmetic on a few hundred numbers per tensor; the gradients behind them are taken on one
thread so that no reduction depends on how many cores the host has."""
import contextlib
import copy
import hashlib
import json
import os
import types

import pytest
import torch

import toy_nets
from helpers import GOLD, pkg

FIXTURE = os.path.join(GOLD, 'prune_score_calls.json')
RECORDED = ('wg_reduce', 'axpby', 'gather_add', 'group_score', 'score_groups', 'select_smallest', 'slice_batch')
CRITERIA = ('taylor', 'taylor_mv_true', 'taylor_mv_false', 'full1', 'full2', 'abs', 'fisher', 'magnitude')
MODELS = ('tiny', 'generator', 'plain_cnn')


def criterion(name):
    p = pkg('pruning')
    return dict(taylor=p.TaylorImportance, taylor_mv_true=lambda: p.TaylorImportance(multivariable=True),
                taylor_mv_false=lambda: p.TaylorImportance(multivariable=False), full1=lambda: p.FullTaylorImportance(order=1),
                full2=lambda: p.FullTaylorImportance(order=2), abs=p.AbsTaylorImportance, fisher=p.FisherImportance,
                magnitude=p.MagnitudeImportance)[name]()


def digest(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:10]


def ranges(idxs):
    """[0, 1, 2, 7, 8] -> [[0, 3], [7, 9]] (any list round-trips; ascending ones come out short)."""
    out = []
    for i in (int(v) for v in idxs):
        if out and out[-1][1] == i:
            out[-1][1] = i + 1
        else:
            out.append([i, i + 1])
    return out


def _member(m):
    return [m[k] for k in ('R', 'C', 'T', 'dim', 'mode', 'full_off', 'col_off', 'idx_off')]


def recorder(log):
    """A stand-in module that is mock_ops_prune_global with the seven calls wrapped: each appends [arguments, None] to `log` before it
    runs and puts the hash of what it produced in place of the None after (a call that raises keeps its None)."""
    import mock_ops_prune_global as mock
    rec = types.ModuleType('recording_ops')
    rec.__dict__.update({k: v for k, v in vars(mock).items() if not k.startswith('__')})

    def wrap(name, describe, result):
        real = getattr(mock, name)

        def call(*a, **kw):
            entry = [[name] + describe(*a, **kw), None]
            log.append(entry)
            r = real(*a, **kw)
            entry[1] = result(r, *a)
            return r
        setattr(rec, name, call)

    def wg(w, g, dim, mode, out, accumulate, scratch=None):           # R, C, T as ops.wg_reduce derives them
        R, Cc = w.shape[0], (w.shape[1] if w.dim() > 1 else 1)
        return [R, Cc, w.numel() // (R * Cc), dim, mode, int(bool(accumulate))]
    wrap('wg_reduce', wg, lambda r, w, g, dim, mode, out, *_: digest(out))
    wrap('axpby', lambda x, a, y, b: [x.numel(), a, b, int(x is y)], lambda r, x, a, y, b: digest(y))
    wrap('gather_add', lambda src, idx, dst: [src.numel(), dst.numel(), ranges(idx.tolist())], lambda r, src, idx, dst: digest(dst))
    wrap('group_score', lambda members, n0, idx_dev, scratch, score:
         [n0, [_member(m) for m in members], None if idx_dev is None else ranges(idx_dev.tolist())],
         lambda r, members, n0, idx_dev, scratch, score: digest(score))
    wrap('score_groups', lambda groups, idx_dev, scratch, scores:
         [[[n0, [_member(m) for m in members]] for members, n0 in groups], None if idx_dev is None else ranges(idx_dev.tolist())],
         lambda r, groups, idx_dev, scratch, scores: digest(scores))
    wrap('select_smallest', lambda scores, offsets, k: [[int(o) for o in offsets], int(k), digest(scores)],
         lambda r, *_: [repr(float(r[0])), [ranges(ix.tolist()) for ix in r[1]]])
    wrap('slice_batch', lambda items, keep_dev: [[[R, Cc, T, dim, nk, off] for _, _, R, Cc, T, dim, nk, off in items],
                                                 keep_dev.numel(), digest(keep_dev)],      # the kept lists: by their hash
         lambda r, items, keep_dev: digest(*[it[1] for it in items]))
    return rec


@contextlib.contextmanager
def recording(log, batch):
    pruning = pkg('pruning')
    saved = pruning.ops, pruning.PRUNE_BATCH
    pruning.ops, pruning.PRUNE_BATCH = recorder(log), bool(batch)
    try:
        yield
    finally:
        pruning.ops, pruning.PRUNE_BATCH = saved


@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


_models = {}


def fresh_model(name):
    """A copy (weights and gradients) of the case's model; the original is built once.  -> (model, example inputs, ignored layers)"""
    if name not in _models:
        with one_thread():
            if name == 'tiny':
                from test_prune_global_cpu import tiny_model_with_oracle_grads
                _models[name] = (tiny_model_with_oracle_grads('tiny_taylor_0.3'), None, None)
            else:
                model, inputs, _ = toy_nets.build(name)
                out = model(*inputs)
                sum((o * o).sum() for o in (out if isinstance(out, tuple) else (out,))).backward()
                _models[name] = (model, inputs, toy_nets.NETS[name][2])
    base, inputs, ignored = _models[name]
    model = copy.deepcopy(base)
    for p, q in zip(model.parameters(), base.parameters()):
        p.grad = None if q.grad is None else q.grad.clone()
    mods = dict(model.named_modules())
    return model, inputs, None if ignored is None else [mods[n] for n in ignored]


def run_case(model_name, crit, global_pruning, batch):
    """-> the ordered records of one pruning run; an exception ends the list as ['raised', its type]."""
    pruning = pkg('pruning')
    model, inputs, ignored = fresh_model(model_name)
    log = []
    with recording(log, batch):
        try:
            if model_name == 'tiny':
                pr = pkg('sweep').prune_model(model, 0.3, importance=criterion(crit), global_pruning=global_pruning)
            else:
                pr = pruning.MetaPruner(model, inputs, importance=criterion(crit), global_pruning=global_pruning, ch_sparsity=0.5,
                                        ignored_layers=ignored)
                for g in pr.step(interactive=True):
                    g.prune()
            log.append([['pruned'] + [[r[0], ranges(r[3])] for r in pr.records], digest(*[r[2] for r in pr.records])])
        except Exception as e:                  # noqa: BLE001 -- what a case raises is part of what is pinned
            log.append([['raised', type(e).__name__], None])
    return log


def out_of_range_group():
    """A hand-made group whose second member's index list reaches past its layer (6 input channels, index 6)."""
    pruning = pkg('pruning')
    g = torch.Generator().manual_seed(3)
    a, b = torch.nn.Conv2d(4, 3, 3), torch.nn.Conv2d(6, 5, 1)
    for m in (a, b):
        m.weight.grad = torch.randn(m.weight.shape, generator=g)
    return pruning.Group([(pruning.Dependency(a, 'a', 'out'), [0, 1, 2]), (pruning.Dependency(b, 'b', 'in'), [2, 4, 6])])


def run_out_of_range(path, batch):
    pruning = pkg('pruning')
    log = []
    with recording(log, batch):
        try:
            imp = pruning.TaylorImportance()
            imp(out_of_range_group()) if path == 'call' else imp.score_all([out_of_range_group()])
        except Exception as e:                  # noqa: BLE001
            log.append([['raised', type(e).__name__], None])
    return log


def case_names():
    names = ['%s/%s/%s/%s' % (m, c, 'global' if gl else 'local', 'batch' if b else 'member')
             for m in MODELS for c in CRITERIA for gl in (False, True) for b in (True, False)]
    return names + ['out_of_range/call/batch', 'out_of_range/score_all/batch']


def run_named(name):
    p = name.split('/')
    if p[0] == 'out_of_range':
        return run_out_of_range(p[1], p[2] == 'batch')
    return run_case(p[0], p[1], p[2] == 'global', p[3] == 'batch')


CHUNK = 16


def summarise(log):
    """The records of one run as the fixture holds them: how many there are, how many of each call, and a running sha1 over the
    records (arguments and result hash, in order) read out after every CHUNK of them and at the end -- so a difference is pinned to
    the first chunk that holds it -- and how the run ended."""
    h, chain, calls = hashlib.sha1(), [], {}
    for i, rec in enumerate(log):
        h.update(json.dumps(rec, separators=(',', ':')).encode())
        calls[rec[0][0]] = calls.get(rec[0][0], 0) + 1
        if (i + 1) % CHUNK == 0 or i + 1 == len(log):
            chain.append(h.hexdigest()[:10])
    return dict(n=len(log), calls=dict(sorted(calls.items())), end=log[-1][0][:2] if log[-1][0][0] == 'raised' else 'pruned',
                chain=chain)


def record_all(full=False):
    """{case: its summary} -- the fixture -- or, full=True, {case: every record}, for comparing two commits record by record."""
    return {name: (run_named(name) if full else summarise(run_named(name))) for name in case_names()}


@pytest.fixture(scope='module')
def pinned():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(pinned):
    assert sorted(pinned) == sorted(case_names())
    assert {c for case in pinned.values() for c in case['calls']} == set(RECORDED) | {'pruned', 'raised'}
    assert all(len(case['chain']) == -(-case['n'] // CHUNK) and sum(case['calls'].values()) == case['n'] for case in pinned.values())


@pytest.mark.parametrize('model', MODELS + ('out_of_range',))
def test_pruning_makes_the_pinned_calls(pinned, model):
    """Every case of one model: the same calls in the same order with the same arguments, and the same bytes out of each.  A
    difference shows the records of the first chunk that holds it."""
    for name in (n for n in case_names() if n.startswith(model + '/')):
        log = run_named(name)
        got, want = summarise(log), pinned[name]
        if got != want:
            k = next((i for i, (g, w) in enumerate(zip(got['chain'], want['chain'])) if g != w), min(len(got['chain']), len(want['chain'])))
            assert got == want, (name, 'first difference in records %d..%d' % (k * CHUNK, (k + 1) * CHUNK - 1),
                                 {x: (got[x], want[x]) for x in ('n', 'calls', 'end')}, log[k * CHUNK:(k + 1) * CHUNK])


def test_a_member_index_outside_its_layer_is_refused_on_both_batched_paths():
    """The bounds check of the member table guards ops.group_score (`__call__`) as it guards ops.score_groups (`score_all`): the
    refusal is pruning's own, before any call reaches a kernel."""
    imp, log = pkg('pruning').TaylorImportance(), []
    with recording(log, True):
        with pytest.raises(IndexError, match='outside its layer'):
            imp(out_of_range_group())
        with pytest.raises(IndexError, match='outside its layer'):
            imp.score_all([out_of_range_group()])
    assert not log


def test_magnitude_honours_transposed_convolutions():
    """MagnitudeImportance on a group with a ConvTranspose2d(3, 5, 3) out-channel member (weight [Cin, Cout, k, k]: the out channels
    are dimension 1), a ConvTranspose2d in-channel member (dimension 0) and a plain in-channel member, against the formula of the
    reference's MagnitudeImportance.__call__ (importance.py:60-126, the `transposed` branches at lines 73 and 89) recomputed in fp64
    torch -- member by member (`__call__`) and through the one-pass table (`score_all`)."""
    from helpers import relerr
    from test_prune_global_cpu import SCORE_BOUND
    pruning = pkg('pruning')
    torch.manual_seed(7)
    up, nxt, conv = torch.nn.ConvTranspose2d(3, 5, 3), torch.nn.ConvTranspose2d(5, 4, 3), torch.nn.Conv2d(5, 2, 3)
    idxs = list(range(5))

    def group():
        return pruning.Group([(pruning.Dependency(up, 'up', 'out'), list(idxs)), (pruning.Dependency(nxt, 'nxt', 'in'), list(idxs)),
                              (pruning.Dependency(conv, 'conv', 'in'), list(idxs))])
    assert [d.handler.__name__ for d, _ in group()] == ['prune_conv_transpose_out_channels', 'prune_conv_transpose_in_channels',
                                                        'prune_conv_in_channels']
    w_up, w_nxt, w_conv = (m.weight.data.double() for m in (up, nxt, conv))
    imp64 = torch.stack([w_up.transpose(1, 0)[idxs].flatten(1).abs().pow(2).sum(1),             # importance.py:73-77
                         w_nxt.flatten(1).abs().pow(2).sum(1)[idxs],                            # importance.py:89-90, 98, 103
                         w_conv.transpose(0, 1).flatten(1).abs().pow(2).sum(1)[idxs]]).mean(0)  # importance.py:92
    want = imp64 / imp64.mean()
    imp, log = pruning.MagnitudeImportance(), []
    with recording(log, True):
        one = imp(group())
        (every,) = imp.score_all([group()])
    assert [r[0][0] for r in log if r[0][0] in ('group_score', 'score_groups')] == ['score_groups']
    for got in (one, every):
        err = relerr(got, want)
        print('magnitude, transposed members: relative error %.3e (bound %.1e)' % (err, SCORE_BOUND))
        assert got.dtype == torch.float32 and tuple(got.shape) == (5,) and err < SCORE_BOUND, err
