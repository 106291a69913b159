"""csrc/magnitude.hip on the device (`-m gpu`): dp_magnitude_rows and dp_magnitude_finish against the fp64 restatement of
tests/magnitude_ref.py at the smallest shapes that can go wrong, and the fixture masks of tests/golden/magnitude_family.json (the
reference's own MagnitudePruner) reproduced from device weights.

Bound of every comparison: max(4 e_ref32, 1e-5) on helpers.relerr (max-abs error over the reference's max-abs) -- e_ref32 = the same
expression in torch fp32 on the host (tests/mock_ops_magnitude.py) against fp64, 1e-5 = the floor tests/test_prune_global_gpu.py holds
scores to.  The finish is judged on the rows the device produced (read back and restated in fp64), and the LAMP stage on the
normalised fp32 vector the device produced: LAMP as vendored gathers through the sort order, so it is discontinuous where two scores
swap, and a comparison across precisions of anything before the sort would test the data's near-ties, not the kernel.

Launch-site tables of csrc/magnitude.hip (the discipline of tests/test_prune_global_gpu.py, for the file's own MG_LAUNCH macro):
  BRANCHES every kernel expression the file's launch sites can record; LAUNCH_SITES MG_LAUNCH( sites per file
  (tests/test_magnitude_family_cpu.py counts them); CASES entry -> the cases that reach it and assert the ring names.
Every measured value is printed beside its bound (pytest -s); profiles/magnitude_family_gpu_tests.txt holds them."""
import ctypes

import numpy as np
import pytest
import torch

import golden_common as gc
import magnitude_ref as MR
from helpers import load_json, pkg, relerr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FLOOR = 1e-5

LAUNCH_SITES = {'magnitude.hip': 4}
BRANCHES = ['mg_rows_kernel<1>', 'mg_rows_kernel<2>', 'mg_rows_kernel<0>', 'mg_finish_kernel']
ROWS_OF_P = {1: BRANCHES[0], 2: BRANCHES[1], 3: BRANCHES[2], 0.5: BRANCHES[2]}
CASES = {}


def case(*entries):
    def deco(fn):
        for e in entries:
            assert e in BRANCHES, e
            CASES.setdefault(e, []).append(fn)
        return fn
    return deco


@pytest.fixture(scope='module')
def ops():
    o = pkg('ops')
    o.L.load()
    return o


def launched(ops, fn):
    """(fn(), the kernel expressions of the launches fn issued, oldest first, outer parentheses stripped)."""
    lib = ops.L.load()
    c0 = lib.dp_launch_count()
    r = fn()
    n = min(lib.dp_launch_count() - c0, 256)          # the ring keeps the last 256
    assert n >= 0
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    assert k >= n
    return r, [arr[i].decode().strip('()') for i in range(k - n, k)]


def _line(report, key, **kw):
    report['magnitude/' + key] = kw
    print('magnitude/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ====================================================================================================================== the kernels
def cap(ops):
    return ops.MAGNITUDE_MAX_WIDTH


def build_groups(widths, descending=False):
    """Per width one group of 1 to 5 members (cycling), host tensors: (w, R, C, T, dim, idxs) each.  The member kinds, in the order a
    group takes them: out-channel conv with T = 9; in-channel conv with T = 9; in-channel linear (T = 1) read through an index list
    into a wider layer; out-channel member whose row length is a multiple of 4 (the 16-byte loads); out-channel member through an index
    list.  Every third member's tensor starts at element offset 1 of its buffer (no 16-byte alignment).  descending: every member is
    read through the list n0 - 1 .. 0."""
    groups, seed = [], 7
    for gi, n0 in enumerate(widths):
        other = (3, 5, 2, 7, 1)[gi % 5]
        kinds = [(n0, other, 9, 0, False), (other + 1, n0, 9, 1, False), (other + 2, n0 + 5, 1, 1, True), (n0, 4, 3, 0, False),
                 (n0 + 3, other, 1, 0, True)]
        members = []
        for j in range(1 + gi % 5):
            R, Cc, T, dim, mapped = kinds[(gi + j) % 5]
            seed += 1
            buf = rnd(R * Cc * T + 1, seed=seed)
            w = buf[1:] if (gi + j) % 3 == 2 else buf[:-1]
            n_full = Cc if dim else R
            if descending:
                idxs = list(range(n0 - 1, -1, -1))
            elif mapped:
                idxs = sorted(torch.randperm(n_full, generator=torch.Generator().manual_seed(seed))[:n0].tolist())
            else:
                idxs = list(range(n0))
            members.append((w, R, Cc, T, dim, idxs))
        groups.append((n0, members))
    return groups


def lay_out(groups):
    """The member table and the group table as pruning.MagnitudeImportance._kernel_scores lays them out, tensors on the device
    (an offset-1 view keeps its misalignment: the whole buffer is moved, then sliced)."""
    members, gtab, idx, row, keep = [], [], [], 0, []
    for n0, ms in groups:
        gtab.append((row, n0, len(ms)))
        for w, R, Cc, T, dim, idxs in ms:
            base = w._base if w._base is not None else w
            dbase = base.reshape(-1).to(DEV)
            keep.append(dbase)
            dw = dbase[w.storage_offset():w.storage_offset() + w.numel()]
            assert dw.is_contiguous() and (dw.data_ptr() - dbase.data_ptr()) == 4 * w.storage_offset()
            idx_off = -1
            if not ((Cc if dim else R) == n0 and idxs == list(range(n0))):
                idx_off = len(idx)
                idx.extend(idxs)
            members.append(dict(w=dw, R=R, C=Cc, T=T, dim=dim, n0=n0, idx_off=idx_off, row_off=row, fold=len(idxs) // n0))
            row += n0
    idx_dev = torch.tensor(idx, dtype=torch.int64, device=DEV) if idx else None
    return members, gtab, idx_dev, row, keep


def host_rows32(groups, p, root):
    import mock_ops_magnitude as mock
    members, gtab, idx, row = [], [], [], 0
    for n0, ms in groups:
        for w, R, Cc, T, dim, idxs in ms:
            members.append(dict(w=w.contiguous(), R=R, C=Cc, T=T, dim=dim, n0=n0, idx_off=len(idx), row_off=row, fold=len(idxs) // n0))
            idx.extend(idxs)
            row += n0
    return mock.magnitude_rows(members, torch.tensor(idx, dtype=torch.int64), p, root, torch.empty(row))


def rows_case(ops, report, p, root, widths, tag, descending=False):
    groups = build_groups(widths, descending)
    members, gtab, idx_dev, total, keep = lay_out(groups)
    assert any(m['w'].data_ptr() % 16 for m in members) and any(m['w'].data_ptr() % 16 == 0 and (m['C'] * m['T']) % 4 == 0 and m['dim'] == 0
                                                                for m in members)
    rows = torch.full((total,), float('nan'), device=DEV)
    _, names = launched(ops, lambda: ops.magnitude_rows(members, idx_dev, p, root, rows))
    assert names == [ROWS_OF_P[p]], names
    again = torch.full((total,), float('nan'), device=DEV)
    ops.magnitude_rows(members, idx_dev, p, root, again)
    assert torch.equal(rows, again), 'two calls differ'
    r32, off = host_rows32(groups, p, root), 0
    for n0, ms in groups:
        want = MR.member_rows(ms, p, root).reshape(-1)
        got = rows[off:off + len(ms) * n0]
        err, e32 = relerr(got, want), relerr(r32[off:off + len(ms) * n0], want)
        bound = max(4 * e32, FLOOR)
        _line(report, 'rows/%s/p%s%s/n0_%d' % (tag, p, '_root' if root else '', n0), members=len(ms), err=err, bound=bound, e_ref32=e32)
        assert err <= bound, (p, root, n0, err, bound)
        off += len(ms) * n0
    return rows, gtab, groups, names


def widths_of(ops):
    return [1, 2, 63, 64, 65, 257, 1024, cap(ops)]


@case('mg_rows_kernel<1>')
def rows_p1(ops, report):
    return rows_case(ops, report, 1, False, widths_of(ops), 'plain')[3]


@case('mg_rows_kernel<2>')
def rows_p2(ops, report):
    return rows_case(ops, report, 2, True, widths_of(ops), 'plain')[3]


@case('mg_rows_kernel<0>')
def rows_p3(ops, report):
    return rows_case(ops, report, 3, False, widths_of(ops), 'plain')[3]


@pytest.mark.parametrize('p,root', [(1, False), (2, False), (3, False), (0.5, False), (1, True), (2, True), (3, True)])
def test_rows_against_fp64(ops, report, p, root):
    """Widths 1, 2, 63, 64, 65, 257, 1024 and the cap; 1 to 5 members; T of 1 and 9; dim 0 and 1; identity and index-mapped members; base
    pointers at element offset 1 and 16-byte aligned rows; two calls bit-equal."""
    rows_case(ops, report, p, root, widths_of(ops), 'plain')


def test_rows_through_a_descending_index_list(ops, report):
    rows_case(ops, report, 2, True, [2, 65, 257], 'descending', descending=True)


def test_rows_fold_a_member_that_holds_the_channels_twice(ops, report):
    """fold = 2 and 3: value j sums the channels at entries j * fold .. of an unsorted list (importance.py:188-195), dim 1 and dim 0."""
    g = torch.Generator().manual_seed(21)
    groups = []
    for n0, k in ((65, 2), (5, 3), (1, 2)):
        first = (rnd(n0 * 2 * 9, seed=n0), n0, 2, 9, 0, list(range(n0)))
        cols = (rnd(3 * n0 * k * 9, seed=n0 + 1), 3, n0 * k, 9, 1, torch.randperm(n0 * k, generator=g).tolist())
        rws = (rnd(n0 * k * 2, seed=n0 + 2), n0 * k, 2, 1, 0, torch.randperm(n0 * k, generator=g).tolist())
        groups.append((n0, [first, cols, rws]))
    members, gtab, idx_dev, total, keep = lay_out(groups)
    assert [m['fold'] for m in members] == [1, 2, 2, 1, 3, 3, 1, 2, 2]
    rows = torch.full((total,), float('nan'), device=DEV)
    ops.magnitude_rows(members, idx_dev, 2, True, rows)
    r32, off = host_rows32(groups, 2, True), 0
    for n0, ms in groups:
        want = MR.member_rows(ms, 2, True).reshape(-1)
        err, e32 = relerr(rows[off:off + 3 * n0], want), relerr(r32[off:off + 3 * n0], want)
        _line(report, 'rows/fold/n0_%d' % n0, err=err, bound=max(4 * e32, FLOOR), e_ref32=e32)
        assert err <= max(4 * e32, FLOOR)
        off += 3 * n0
    L = pkg('_lib')
    with pytest.raises(L.DpHipError):                                     # a fold without a list, a list shorter than n0 * fold
        ops.magnitude_rows([dict(members[1], idx_off=-1)], idx_dev, 2, True, rows)
    with pytest.raises(L.DpHipError):
        ops.magnitude_rows([dict(members[1], idx_off=idx_dev.numel() - 129)], idx_dev, 2, True, rows)


def test_rows_in_order_member_with_more_taps_than_the_tile(ops, report):
    """An in-order dim-1 member is read in 256-byte segments through a [64 * T] tile up to T = 16 taps; T = 16, 17 and 25 (a 5 x 5
    convolution) sit on both sides of that switch, at widths that end inside a block."""
    groups = [(70, [(rnd(70 * 2, seed=1), 70, 2, 1, 0, list(range(70)))] +
               [(rnd(5 * 70 * T, seed=T), 5, 70, T, 1, list(range(70))) for T in (16, 17, 25)]),
              (3, [(rnd(2 * 3 * 16, seed=40), 2, 3, 16, 1, list(range(3)))])]
    members, gtab, idx_dev, total, keep = lay_out(groups)
    assert idx_dev is None
    rows = torch.full((total,), float('nan'), device=DEV)
    ops.magnitude_rows(members, None, 1, False, rows)
    r32, off = host_rows32(groups, 1, False), 0
    for n0, ms in groups:
        want = MR.member_rows(ms, 1).reshape(-1)
        n = len(ms) * n0
        err, e32 = relerr(rows[off:off + n], want), relerr(r32[off:off + n], want)
        _line(report, 'rows/taps/n0_%d' % n0, err=err, bound=max(4 * e32, FLOOR), e_ref32=e32)
        assert err <= max(4 * e32, FLOOR)
        off += n


def finish_ref32(rows, gtab, red, norm, lamp):
    import mock_ops_magnitude as mock
    out = torch.empty(sum(n0 for _, n0, _ in gtab))
    return mock.magnitude_finish(gtab, rows.cpu(), red, norm, lamp, out)


@case('mg_finish_kernel')
def finish_case(ops, report, p=2, reductions=('mean',), normalizers=('mean',)):
    rows, gtab, groups, _ = rows_case(ops, report, p, False, widths_of(ops), 'finish')
    total = sum(n0 for _, n0, _ in gtab)
    names = []
    for red in reductions:
        for norm in normalizers:
            scores = torch.full((total,), float('nan'), device=DEV)
            _, names = launched(ops, lambda: ops.magnitude_finish(gtab, rows, red, norm, None, scores))
            assert names == ['mg_finish_kernel'], names
            again = torch.full((total,), float('nan'), device=DEV)
            ops.magnitude_finish(gtab, rows, red, norm, None, again)
            assert torch.equal(scores.nan_to_num(nan=-7.0), again.nan_to_num(nan=-7.0)), 'two calls differ'
            r32, off, worst = finish_ref32(rows, gtab, red, norm, None), 0, (0.0, 0.0, 0.0, 0)
            for row_off, n0, M in gtab:
                want = MR.finish(rows[row_off:row_off + M * n0].double().cpu().view(M, n0), red, norm)
                got = scores[off:off + n0]
                if n0 == 1 and norm == 'gaussian':                      # torch.std of one value: NaN there, NaN here
                    assert torch.isnan(got).all() and torch.isnan(want).all()
                else:
                    err, e32 = relerr(got, want), relerr(r32[off:off + n0], want)
                    bound = max(4 * e32, FLOOR)
                    assert err <= bound, (red, norm, n0, err, bound)
                    worst = max(worst, (err / bound, err, bound, n0))
                off += n0
            _line(report, 'finish/p%s/%s/%s' % (p, red, norm), err=worst[1], bound=worst[2], n0=worst[3])
    return names


@pytest.mark.parametrize('p', [1, 3])
def test_finish_every_reduction_normaliser_pair(ops, report, p):
    finish_case(ops, report, p, MR.REDUCTIONS, MR.NORMALIZERS)


def lamp64(x, order):
    x = x.double().cpu()
    a = torch.argsort(x, descending=True, stable=True)
    q = x[a] / torch.cumsum(x[a], 0)
    if order == 'vendored':
        return q[a]
    out = torch.empty_like(q)
    out[a] = q
    return out


def direct_finish(ops, vectors, lamp, norm=None):
    """Groups of one member whose row IS the vector: the finish on hand-made values."""
    rows = torch.cat(vectors).to(DEV)
    gtab, off = [], 0
    for v in vectors:
        gtab.append((off, len(v), 1))
        off += len(v)
    out = torch.full((off,), float('nan'), device=DEV)
    ops.magnitude_finish(gtab, rows, 'first', norm, lamp, out)
    again = torch.full((off,), float('nan'), device=DEV)
    ops.magnitude_finish(gtab, rows, 'first', norm, lamp, again)
    assert torch.equal(out.nan_to_num(nan=-7.0), again.nan_to_num(nan=-7.0)), 'two calls differ'
    return [out[a:a + n] for a, n, _ in gtab]


@pytest.mark.parametrize('order', ['vendored', 'paper'])
def test_lamp_stage_against_fp64(ops, report, order):
    """The sort, the scan, the division and the scatter on the normalised vectors the device itself produced (widths 1 .. cap), on
    vectors with ties, on an all-equal group and on a two-value group: exactly the fp64 result's order, values within the bound."""
    rows, gtab, groups, _ = rows_case(ops, report, 2, True, widths_of(ops), 'lamp')
    total = sum(n0 for _, n0, _ in gtab)
    x = torch.empty(total, device=DEV)
    ops.magnitude_finish(gtab, rows, 'mean', 'mean', None, x)
    got = torch.empty(total, device=DEV)
    _, names = launched(ops, lambda: ops.magnitude_finish(gtab, rows, 'mean', 'mean', order, got))
    assert names == ['mg_finish_kernel']
    off = 0
    for _, n0, _ in gtab:
        want = lamp64(x[off:off + n0], order)
        e32 = relerr(finish_ref32(x[off:off + n0], [(0, n0, 1)], 'first', None, order), want)
        err, bound = relerr(got[off:off + n0], want), max(4 * e32, FLOOR)
        _line(report, 'lamp/%s/n0_%d' % (order, n0), err=err, bound=bound, e_ref32=e32)
        assert err <= bound, (order, n0, err, bound)
        off += n0
    g = torch.Generator().manual_seed(5)
    ties = torch.rand(300, generator=g)
    ties[torch.randint(0, 300, (120,), generator=g)] = float(ties[3])
    ties[7], ties[8] = 0.0, -0.0
    vectors = [ties, torch.full((65,), 0.37), torch.tensor([2.0, 2.0]), torch.tensor([5.0]), torch.tensor([1.0, 3.0, 2.0, 3.0])]
    for v, s in zip(vectors, direct_finish(ops, vectors, order)):
        want = lamp64(v, order)
        err = relerr(s, want)
        _line(report, 'lamp/%s/ties_n%d' % (order, len(v)), err=err, bound=FLOOR)
        assert err <= FLOOR, (order, len(v), err)
    # the paper's order on [1, 3, 2, 3]: channel 1 (the first of the tied largest) scores 1, channel 3 gets 3 / 6, channel 2 2 / 8, channel 0 1 / 9
    s = direct_finish(ops, [torch.tensor([1.0, 3.0, 2.0, 3.0])], order)[0].cpu()
    want = [1 / 9, 1.0, 2 / 8, 3 / 6] if order == 'paper' else [3 / 6, 1 / 9, 2 / 8, 1.0]      # vendored: q = [1, 1/2, 1/4, 1/9] gathered at a = [1, 3, 2, 0]
    assert torch.allclose(s, torch.tensor(want, dtype=torch.float32), rtol=1e-6, atol=0), (order, s)


def test_all_zero_group_and_denormals(ops, report):
    """An all-zero group: the NaN pattern of the fp64 expression under every normaliser ('sum', 'mean', 'max' divide 0 by 0).  Denormal
    weights (1e-41) under p = 1: rows within the bound of fp64, and 'max'-normalised scores as fp64 gives them."""
    zero = [torch.zeros(5), torch.zeros(64), torch.zeros(1)]
    for norm in MR.NORMALIZERS:
        for v, s in zip(zero, direct_finish(ops, zero, None, norm)):
            want = MR.finish(v.double().view(1, -1), 'first', norm)
            assert torch.equal(torch.isnan(s).cpu(), torch.isnan(want)), (norm, len(v), s)
            assert torch.equal(s.cpu().nan_to_num().double(), want.nan_to_num()), (norm, len(v))
    g = torch.Generator().manual_seed(9)
    w = (torch.rand(65, 3, 9, generator=g) + 0.5) * 1e-41
    assert float(w.max()) < 1.2e-38 and float(w.min()) > 0
    members, gtab, idx_dev, total, keep = lay_out([(65, [(w.reshape(-1), 65, 3, 9, 0, list(range(65)))]), (3, [(w.reshape(-1), 65, 3, 9, 1, [0, 1, 2])])])
    rows = torch.empty(total, device=DEV)
    ops.magnitude_rows(members, idx_dev, 1, False, rows)
    want = torch.cat([MR.member_rows([(w, 65, 3, 9, 0, list(range(65)))], 1)[0], MR.member_rows([(w, 65, 3, 9, 1, [0, 1, 2])], 1)[0]])
    err = relerr(rows, want)
    _line(report, 'denormal/rows', err=err, bound=FLOOR, largest=float(want.max()))
    assert float(rows.min()) > 0 and err <= FLOOR
    out = torch.empty(total, device=DEV)
    ops.magnitude_finish(gtab, rows, 'sum', 'max', None, out)
    err = max(relerr(out[:65], want[:65] / want[:65].max()), relerr(out[65:], want[65:] / want[65:].max()))
    _line(report, 'denormal/sum_max', err=err, bound=FLOOR)
    assert err <= FLOOR


def test_launchers_refuse_what_they_cannot_take(ops):
    """cap + 1 channels, offsets past the buffers, a group table that does not tile the scores: hipErrorInvalidValue, nothing launched."""
    L = pkg('_lib')
    n = cap(ops) + 1
    rows = torch.zeros(n, device=DEV)
    out = torch.zeros(n, device=DEV)

    def refused(fn):
        (_, names) = launched(ops, lambda: pytest.raises(L.DpHipError, fn))
        assert names == []
    refused(lambda: ops.magnitude_finish([(0, n, 1)], rows, 'sum', None, None, out))
    refused(lambda: ops.magnitude_finish([(0, 8, 2)], rows[:15], 'sum', None, None, out[:8]))                 # 2 x 8 rows of 15 floats
    refused(lambda: ops.magnitude_finish([(0, 8, 1)], rows, 'sum', None, None, out[:9]))                      # 8 scores of 9
    w = torch.zeros(4, 3, 1, device=DEV)
    m = dict(w=w, R=4, C=3, T=1, dim=0, n0=4, idx_off=-1, row_off=0)
    idx = torch.zeros(3, dtype=torch.int64, device=DEV)
    refused(lambda: ops.magnitude_rows([dict(m, row_off=n - 3)], None, 1, False, rows))                        # the row ends past `rows`
    refused(lambda: ops.magnitude_rows([dict(m, n0=5)], None, 1, False, rows))                                 # 5 channels of a 4-channel layer
    refused(lambda: ops.magnitude_rows([dict(m, idx_off=0)], idx, 1, False, rows))                             # 4 indices of a 3-entry list
    refused(lambda: ops.magnitude_rows([dict(m, idx_off=0)], None, 1, False, rows))
    refused(lambda: ops.magnitude_rows([m], None, 0.0, False, rows))


def test_wider_than_the_cap_is_served_by_the_torch_path(ops, report):
    pruning = pkg('pruning')
    n = cap(ops) + 1
    conv = torch.nn.Conv2d(2, n, 1).to(DEV)
    group = pruning.Group([(pruning.Dependency(conv, 'wide', 'out'), list(range(n)))])
    imp = pruning.MagnitudeImportance(p=1, group_reduction='sum', normalizer='max')
    got, names = launched(ops, lambda: imp(group))
    assert names == [] and got.is_cuda and tuple(got.shape) == (n,)
    want = MR.finish(MR.member_rows([(conv.weight, n, 2, 1, 0, list(range(n)))], 1), 'sum', 'max')
    err = relerr(got, want)
    _line(report, 'wide/cap_plus_1', err=err, bound=FLOOR)
    assert err <= FLOOR
    narrow = torch.nn.Conv2d(2, n - 1, 1).to(DEV)
    _, names = launched(ops, lambda: imp(pruning.Group([(pruning.Dependency(narrow, 'cap', 'out'), list(range(n - 1)))])))
    assert names == ['mg_rows_kernel<1>', 'mg_finish_kernel']


@pytest.mark.parametrize('entry', BRANCHES)
def test_branch(ops, report, entry):
    """Every MG_LAUNCH site is reached by a case whose launches name it in the ring (the cases assert the whole name sequence)."""
    assert entry in CASES, 'no case reaches %s' % entry
    for fn in CASES[entry]:
        _, names = launched(ops, lambda: fn(ops, report))
        assert entry in names and set(names) <= set(BRANCHES), (entry, names)


# ====================================================================================================================== end to end
from test_magnitude_family_cpu import FX, build_model, check_mask_case, run_mask_case, score_errors, make_criterion, all_groups      # noqa: E402


def device_forward(name, model):
    if name == 'ldm':
        from test_cpu import _ldm_inputs
        x, ctx, _, t = _ldm_inputs()
        return model(x.to(DEV), t.to(DEV), context=ctx.to(DEV))
    cfg, cs, ns, t = (gc.TINY_CFG, 1, 2, [3, 500]) if name == 'tiny' else (load_json('groups_more.json')['heads8_4lvl']['cfg'], 81, 82, [5, 700])
    H = cfg['sample_size']
    clean, noise = torch.from_numpy(gc.det_clean((2, 3, H, H), cs)).to(DEV), torch.from_numpy(gc.det_noise((2, 3, H, H), ns)).to(DEV)
    tt = torch.tensor(t, device=DEV)
    return model(pkg('diffusion').DDPMScheduler().add_noise(clean, noise, tt), tt).sample


@pytest.mark.parametrize('name', sorted(FX['masks']))
def test_fixture_masks_from_device_weights(ops, report, name):
    """The reference's indices, shapes and threshold from device weights, and the pruned model's forward on the stored input within
    1e-5 of the reference's pruned model (the bound of tests/test_prune_global_gpu.py)."""
    case_ = FX['masks'][name]
    (model, pr), names = launched(ops, lambda: run_mask_case(name, DEV))
    assert 'mg_finish_kernel' in names and not [k for k in names if k.startswith(('pg_score', 'group_score', 'wg_'))], names
    check_mask_case(name, model, pr)
    with torch.no_grad():
        y = device_forward(case_['model'], model)
    e = float((y.cpu() - torch.from_numpy(FX['arrays'][case_['model']]['masks/%s/fwd_after' % name])).abs().max())
    _line(report, 'e2e/%s' % name, groups=len(pr.records), fwd_after_abs=e, bound=1e-5, gap=case_['gap'], err64=case_['err64'])
    assert e < 1e-5


@pytest.mark.parametrize('model_name,keys', [
    ('tiny', ['MagnitudeImportance/1/sum/max', 'MagnitudeImportance/0.5/prod/gaussian', 'MagnitudeImportance/3/max/standarization',
              'LAMPImportance/1/mean/mean', 'LAMPImportance/2/mean/mean']),
    ('ldm', ['MagnitudeImportance/1/mean/sum', 'MagnitudeImportance/2/first/None', 'MagnitudeImportance/3/sum/mean'])])
def test_fixture_scores_from_device_weights(ops, report, model_name, keys):
    """score_all on the device against the reference's stored scores: one rows launch and one finish launch for all groups."""
    model, kw = build_model(model_name, DEV)
    groups, chg = all_groups(model, kw)
    for key in keys:
        imp = make_criterion(key)
        got, names = launched(ops, lambda: imp.score_all(groups, chg))
        assert len(names) == 2 and names[1] == 'mg_finish_kernel' and names[0].startswith('mg_rows_kernel'), names
        err, bound = score_errors(model_name, key, got), max(4 * FX['models'][model_name]['scores'][key]['e_ref32'], FLOOR)
        _line(report, 'scores/%s/%s' % (model_name, key), err=err, bound=bound, groups=len(groups))
        assert err <= bound, (key, err, bound)


def test_global_prune_reads_nothing_back_but_the_selection(ops, report, monkeypatch):
    """A global prune with a string normaliser: the ring shows one rows launch, one finish launch and dp_select_smallest's kernels, and
    no tensor is read on the host on the way (Tensor.cpu / item / tolist / numpy / float() / int() / bool() on a device tensor are
    counted) -- the selection's own copy, inside the library, is the only one.  The default configuration on the same model reads one
    scalar per group."""
    from test_prune_global_gpu import SELECT_NAMES
    pruning = pkg('pruning')
    reads = []

    def counting(attr):
        real = getattr(torch.Tensor, attr)

        def wrapper(self, *a, **k):
            if self.is_cuda:
                reads.append(attr)
            return real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, attr, wrapper)
    for attr in ('cpu', 'item', 'tolist', 'numpy', '__float__', '__int__', '__bool__'):
        counting(attr)

    def scored_and_selected(imp):
        model, kw = build_model('tiny', DEV)
        pr = pruning.MagnitudePruner(model, None, importance=imp, global_pruning=True, ch_sparsity=0.3, **kw)
        del reads[:]
        picked, names = launched(ops, lambda: list(pr.step(interactive=True)))
        return pr, picked, names, list(reads)
    pr, picked, names, seen = scored_and_selected(pruning.MagnitudeImportance(p=1, group_reduction='mean', normalizer='max'))
    assert names == ['mg_rows_kernel<1>', 'mg_finish_kernel'] + SELECT_NAMES, names
    assert seen == [] and len(picked) == 50 and all(r[2].is_cuda for r in pr.records)
    _, _, names, seen_lamp = scored_and_selected(pruning.LAMPImportance(p=2))
    assert names == ['mg_rows_kernel<2>', 'mg_finish_kernel'] + SELECT_NAMES and seen_lamp == []
    _, _, _, seen_default = scored_and_selected(pruning.MagnitudeImportance())
    _line(report, 'reads/global_prune', new_path=len(seen), lamp=len(seen_lamp), default_path=len(seen_default))
    assert len(seen_default) >= 50
