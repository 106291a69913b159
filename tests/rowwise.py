"""The per-row error figure of the contraction kernels, the operand families it is measured on, and the three CPU references.

`helpers.relerr` divides the largest error of a tensor by the largest magnitude of the tensor: an error of 1e-6 of the largest row is
invisible in a row that is 1e-6 of it.  `rowwise` divides, row by row, the largest error of the row by the largest value in that row of
cond64 -- the same operation evaluated in fp64 on the absolute values of every operand (epilogue addends included): the figure is in
units of the rounding error a sum of that row's own products can have, and no row is excluded.

A Case holds fp32 CPU operands and three ways to evaluate them:
  plain(o)      the operation through torch's CPU operators on the operand dict o (fp64 -> ref64, fp64 |.| -> cond64, fp32 -> e_ref32);
  alg(o, rows)  the algorithm the kernel documents, written out, on the selected rows ([len(rows), row length]): the transforms of the
                kernel's header comment, then the products added ONE AFTER ANOTHER in contraction order (`chain`).  In fp64 it equals
                plain (tests/test_rowwise_cpu.py: 1e-12 of cond64), in fp32 it gives e_alg32;
  epilogue      out = post * (alpha * plain + sum(addends)).
`evaluate` gives ref64, cond64, e_ref32, e_alg32 and bound = 4 * max(e_ref32, e_alg32, 2 * 2^-24): from the references alone.

Families (FAMILIES), all seeded, all from randn: see `draw`.  Exponent range: 10^U(-4, 4) everywhere but the importance kernels
(wg_reduce, group_score: 10^U(-3, 3)), whose squared modes raise a product of four scales to the second power."""
import collections
import math

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
FAMILIES = ('randn', 'row scales', 'all scales', 'all scales + offsets')

# pads = (top, bottom, left, right) zeros round the (upsampled) input
Spec = collections.namedtuple('Spec', 'kh kw stride pads ups')
SAME3 = Spec(3, 3, 1, (1, 1, 1, 1), 0)
UPS3 = Spec(3, 3, 1, (1, 1, 1, 1), 1)


# ======================================================================================================================
# the figure
# ======================================================================================================================
def to_rows(t, row_dims):
    """[rows, elements of a row]: the dims `row_dims` index the rows (flattened in that order), the others the row's elements."""
    row_dims = tuple(row_dims)
    rest = tuple(d for d in range(t.dim()) if d not in row_dims)
    n = 1
    for d in row_dims:
        n *= t.shape[d]
    return t.permute(row_dims + rest).reshape(n, -1)


def rowwise(got, ref64, cond64, row_dims):
    """max over rows of max_{i in row} |got_i - ref64_i| / max_{i in row} cond64_i.  Every row counts; a row without a positive cond64
    is a mistake of the test."""
    got = torch.as_tensor(got).detach().double().cpu()
    assert got.shape == ref64.shape == cond64.shape, (tuple(got.shape), tuple(ref64.shape), tuple(cond64.shape))
    den = to_rows(cond64, row_dims).amax(1)
    assert bool(torch.isfinite(den).all()) and bool((den > 0).all()), 'a row whose cond64 maximum is 0 (or not finite)'
    return float((to_rows((got - ref64).abs(), row_dims).amax(1) / den).max())


def relerr(a, ref):
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ======================================================================================================================
# the families
# ======================================================================================================================
def draw(family, seed, specs, lo=-4.0, hi=4.0):
    """specs: name -> (shape, base scale, {axis: label}, activation channel axis or None).  Every tensor starts as randn * base.
    Labels name scale vectors 10^U(lo, hi), shared by every axis that carries the label:
      'row:*'  an axis that indexes output rows        -- applied from 'row scales' on;
      'con:*'  a contraction axis                      -- applied from 'all scales' on;
    'all scales + offsets' then shifts every channel of an activation by 3 x its own max |x| (same-sign products)."""
    assert family in FAMILIES, family
    g = torch.Generator().manual_seed(1000 * seed + FAMILIES.index(family))
    scales, out = {}, {}
    for name, (shape, base, axes, act) in specs.items():
        t = torch.randn(*shape, generator=g, dtype=torch.float64) * base
        for ax, label in sorted(axes.items()):
            on = family != 'randn' if label.startswith('row') else family.startswith('all scales')
            assert label.startswith(('row', 'con')), label
            if not on:
                continue
            if label not in scales:
                scales[label] = 10.0 ** (lo + (hi - lo) * torch.rand(shape[ax], generator=g, dtype=torch.float64))
            view = [1] * len(shape)
            view[ax] = shape[ax]
            t = t * scales[label].view(view)
        if act is not None and family.endswith('offsets'):
            t = t + 3.0 * t.abs().amax([d for d in range(len(shape)) if d != act], keepdim=True)
        out[name] = t.float()
    assert all(bool(torch.isfinite(t).all()) for t in out.values())
    return out


# ======================================================================================================================
# the chain and the cases
# ======================================================================================================================
def chain(a, b):
    """sum_j a[:, j] * b[:, j], the products added one after another in the operands' dtype (a / b: [R or 1, J, ...])."""
    acc = a[:, 0] * b[:, 0]
    for j in range(1, a.shape[1]):
        acc = acc + a[:, j] * b[:, j]
    return acc


class Case:
    def __init__(self, kind, shape, family, o, plain, alg, row_dims, alpha=1.0, post=1.0, addends=(), signed=()):
        self.kind, self.shape, self.family, self.o = kind, tuple(shape), family, o
        self.plain, self.alg, self.row_dims = plain, alg, tuple(row_dims)
        self.alpha, self.post, self.addends, self.signed = float(alpha), float(post), tuple(addends), set(signed)
        self._ev = None

    def _out(self, o, absval=False):
        a, p = (abs(self.alpha), abs(self.post)) if absval else (self.alpha, self.post)
        y = self.plain(o) * a
        for n in self.addends:
            y = y + o[n]
        return y * p

    def evaluate(self, n_alg=8):
        if self._ev is None:
            o64 = {n: t.double() for n, t in self.o.items()}
            oabs = {n: (t if n in self.signed else t.abs()) for n, t in o64.items()}
            ref64, cond64 = self._out(o64), self._out(oabs, True)
            e_ref32 = rowwise(self._out(self.o), ref64, cond64, self.row_dims)
            rows = pick_rows(to_rows(cond64, self.row_dims).amax(1), n_alg)
            e_alg32 = rowwise(self.alg_out(self.o, rows), *self.at_rows(rows, ref64, cond64), (0,))
            bound = 4.0 * max(e_ref32, e_alg32, 2.0 * EPS)
            self._ev = dict(ref64=ref64, cond64=cond64, e_ref32=e_ref32, e_alg32=e_alg32, bound=bound, rows=rows)
        return self._ev

    def at_rows(self, rows, *ts):
        return tuple(to_rows(t, self.row_dims)[rows] for t in ts)

    def alg_out(self, o, rows):
        """The restatement with the epilogue, on `rows`: [len(rows), row length] in o's dtype."""
        y = self.alg(o, rows)
        full = self.plain_shape
        assert y.shape[0] == len(rows), (tuple(y.shape), len(rows))
        y = y.reshape(len(rows), -1) * self.alpha
        for n in self.addends:
            y = y + to_rows(o[n].expand(full), self.row_dims)[rows]
        return y * self.post

    @property
    def plain_shape(self):
        if not hasattr(self, '_shape'):
            self._shape = tuple(self.plain(self.o).shape)
        return self._shape

    def figures(self, got):
        """e_hip, the old max-norm figure, and the references' figures for one kernel output."""
        ev = self.evaluate()
        return dict(family=self.family, kind=self.kind, shape=self.shape, e_hip=rowwise(got, ev['ref64'], ev['cond64'], self.row_dims),
                    e_ref32=ev['e_ref32'], e_alg32=ev['e_alg32'], bound=ev['bound'], maxnorm=relerr(got, ev['ref64']))


def pick_rows(scale, n=8):
    """At most n rows by their scale: the two smallest, the two largest and n - 4 evenly between."""
    order = torch.argsort(scale).tolist()
    if len(order) <= n:
        return sorted(order)
    mid = [order[2 + round(i * (len(order) - 5) / (n - 3))] for i in range(1, n - 3)]
    return sorted(set(order[:2] + order[-2:] + mid))


def leak(case, eps=1e-6):
    """The wrong result of the power check: ref64 + eps x (the largest row, broadcast to every row)."""
    ev = case.evaluate()
    r = to_rows(ev['ref64'], case.row_dims)
    big = r[int(r.abs().amax(1).argmax())]
    rest = tuple(d for d in range(ev['ref64'].dim()) if d not in case.row_dims)
    perm = case.row_dims + rest
    inv = [perm.index(d) for d in range(len(perm))]
    wrong = (r + eps * big[None]).reshape([ev['ref64'].shape[d] for d in perm]).permute(inv)
    return wrong.contiguous()


def _m(rows, like):
    return torch.tensor(rows, dtype=like.dtype)


def patches(x, kh, kw, sh, sw):
    """[N, C, tiles down, tiles across, kh, kw] windows of x."""
    return x.unfold(2, kh, sh).unfold(3, kw, sw)


# ---- convolution: plain forms -----------------------------------------------------------------------------------------------
def conv_input(x, spec):
    if spec.ups:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    t, b, l, r = spec.pads
    return F.pad(x, (l, r, t, b))


def conv_plain(x, w, spec):
    return F.conv2d(conv_input(x, spec), w, stride=spec.stride)


def out_hw(spec, H, W):
    t, b, l, r = spec.pads
    u = 2 if spec.ups else 1
    return (u * H + t + b - spec.kh) // spec.stride + 1, (u * W + l + r - spec.kw) // spec.stride + 1


def dgrad_as_conv(dy, w, spec, in_hw):
    """(z, wf): dx = the unpadded stride-1 correlation of z (dy with stride - 1 zeros between its pixels, zero-padded) with wf (w with
    its taps flipped and its channel axes exchanged) -- the gradient w.r.t. the input of size in_hw of conv(spec) without its upsample."""
    N, K, Ho, Wo = dy.shape
    s = spec.stride
    z = dy.new_zeros(N, K, (Ho - 1) * s + 1, (Wo - 1) * s + 1)
    z[:, :, ::s, ::s] = dy
    t, _, l, _ = spec.pads
    top, left = spec.kh - 1 - t, spec.kw - 1 - l
    bottom, right = in_hw[0] + spec.kh - 1 - top - z.shape[2], in_hw[1] + spec.kw - 1 - left - z.shape[3]
    return F.pad(z, (left, right, top, bottom)), w.flip(2, 3).transpose(0, 1).contiguous()


def dgrad_plain(dy, w, spec, in_hw):
    return F.conv2d(*dgrad_as_conv(dy, w, spec, in_hw))


def wgrad_plain(dy, x, spec):
    """[K, C, kh, kw] = sum over images and pixels of dy (x) the windows of conv_input(x)."""
    unf = F.unfold(conv_input(x, spec), (spec.kh, spec.kw), stride=spec.stride)
    d = dy.reshape(dy.shape[0], dy.shape[1], -1)
    return torch.einsum('nrl,nkl->rk', d, unf).view(dy.shape[1], x.shape[1], spec.kh, spec.kw)


# ---- convolution: the algorithms --------------------------------------------------------------------------------------------
def corr_chain(xin, w, stride, rows):
    """Direct implicit GEMM: out[r] = the chain over (tap, channel), taps outermost (the packed operand is [tap][channel][row])."""
    N, C = xin.shape[:2]
    kh, kw = w.shape[2:]
    T, R = kh * kw, len(rows)
    unf = F.unfold(xin, (kh, kw), stride=stride).view(N, C, T, -1)
    b = unf.permute(2, 1, 0, 3).reshape(1, T * C, N, -1)
    a = w[rows].reshape(R, C, T).permute(0, 2, 1).reshape(R, T * C, 1, 1)
    return chain(a, b).reshape(R, -1)


def wgrad_chain(dy, x, spec, rows):
    """Direct weight gradient: the chain over (image, pixel) for the (k, c) pairs `rows` (flat k * C + c)."""
    C, R = x.shape[1], len(rows)
    k, c = [r // C for r in rows], [r % C for r in rows]
    T = spec.kh * spec.kw
    unf = F.unfold(conv_input(x[:, c], spec), (spec.kh, spec.kw), stride=spec.stride).view(x.shape[0], R, T, -1)
    b = unf.permute(1, 0, 3, 2).reshape(R, -1, T)
    a = dy[:, k].reshape(dy.shape[0], R, -1).permute(1, 0, 2).reshape(R, -1, 1)
    return chain(a, b)


_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]           # csrc/winograd2d.hip: B^T, G, A^T of F(2x2, 3x3)
_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]
_TA = [[1, 0], [1, 1], [1, -1], [0, -1]]                                     # csrc/wgrad2d.hip: Ta and To of F(3x3, 2x2)
_TO = [[1, .5, .5, 0], [0, .5, -.5, 0], [0, .5, .5, 1]]
_GU = [[1, 0, 0], [1, 1, 1], [0, 0, 1]]                                      # csrc/ups9.hip: G; (p0 - p1, p1, p2 - p1); y = (m0 + m1, m1 + m2); R
_BD = [[1, -1, 0], [0, 1, 0], [0, -1, 1]]
_AU = [[1, 1, 0], [0, 1, 1]]
_RD = [[0, -1, 0, 1], [0, 1, 1, 0], [1, 0, -1, 0]]


def _even(x):
    assert x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0, tuple(x.shape)
    return F.pad(x, (1, 1, 1, 1))


def wino2d_fwd(x, w, rows):
    """F(2x2, 3x3): U = G g G^T, V = B^T d B, M = chain over c of U V, Y = A^T M A."""
    Bt, Gm, At = _m(_BT, x), _m(_G, x), _m(_AT, x)
    V = torch.einsum('ia,nctuab,jb->cntuij', Bt, patches(_even(x), 4, 4, 2, 2), Bt)
    U = torch.einsum('ia,rcab,jb->rcij', Gm, w[rows], Gm)
    M = chain(U[:, :, None, None, None], V[None])
    return torch.einsum('pi,rntuij,qj->rntpuq', At, M, At).reshape(len(rows), -1)


def wino1d_fwd(x, w, rows):
    """F(2, 3) along W, the kernel rows ky direct: M_pos = chain over (ky, c); y[2p] = M0 + M1 + M2, y[2p + 1] = M1 - M2 - M3."""
    Bt, Gm, At = _m(_BT, x), _m(_G, x), _m(_AT, x)
    N, C, H, W = x.shape
    V = torch.einsum('jb,ncyukb->kcnyuj', Bt, patches(_even(x), 3, 4, 1, 2)).reshape(1, 3 * C, N, H, W // 2, 4)
    U = torch.einsum('jb,rckb->rkcj', Gm, w[rows]).reshape(len(rows), 3 * C, 1, 1, 1, 4)
    return torch.einsum('qj,rnyuj->rnyuq', At, chain(U, V)).reshape(len(rows), -1)


def _pairs(dy, x, rows):
    C = x.shape[1]
    return dy[:, [r // C for r in rows]], x[:, [r % C for r in rows]]


def wino2d_wgrad(dy, x, rows):
    """F(3x3, 2x2): A_t = Ta dy Ta^T, V = B^T d B, G[i][j] = chain over the tiles of all images, dW = To G To^T."""
    Ta, Bt, To = _m(_TA, x), _m(_BT, x), _m(_TO, x)
    d, xs = _pairs(dy, x, rows)
    A = torch.einsum('ia,nrtuab,jb->rntuij', Ta, patches(d, 2, 2, 2, 2), Ta).reshape(len(rows), -1, 4, 4)
    V = torch.einsum('ia,nrtuab,jb->rntuij', Bt, patches(_even(xs), 4, 4, 2, 2), Bt).reshape(len(rows), -1, 4, 4)
    return torch.einsum('ai,rij,bj->rab', To, chain(A, V), To).reshape(len(rows), 9)


def wino1d_wgrad(dy, x, rows):
    """F(3, 2) per kernel row: a = Ta (dy0, dy1), v = B^T d, G_q = chain over the pairs of all images, dW[ky] = To G."""
    Ta, Bt, To = _m(_TA, x), _m(_BT, x), _m(_TO, x)
    d, xs = _pairs(dy, x, rows)
    A = torch.einsum('ja,nryua->rnyuj', Ta, patches(d, 1, 2, 1, 2)[..., 0, :]).reshape(len(rows), -1, 1, 4)
    V = torch.einsum('jb,nryukb->rnyukj', Bt, patches(_even(xs), 3, 4, 1, 2)).reshape(len(rows), -1, 3, 4)
    return torch.einsum('bj,rkj->rkb', To, chain(A, V)).reshape(len(rows), 9)


def ups9_fwd(x, w, rows):
    """U = G w G^T, V = the 3x3 low-resolution patch after (p0 - p1, p1, p2 - p1) along each axis, M = chain over ci, y = A^T M A."""
    Gu, Bd, Au = _m(_GU, x), _m(_BD, x), _m(_AU, x)
    V = torch.einsum('pa,ncijab,qb->cnijpq', Bd, patches(F.pad(x, (1, 1, 1, 1)), 3, 3, 1, 1), Bd)
    U = torch.einsum('pa,rcab,qb->rcpq', Gu, w[rows], Gu)
    M = chain(U[:, :, None, None, None], V[None])
    return torch.einsum('hp,rnijpq,vq->rnihjv', Au, M, Au).reshape(len(rows), -1)


def ups9_dgrad(dy, w, rows):
    """dx[ci] = chain over (co, a, b) of U[co][ci][a][b] T[co][a][b], T = R p R^T of the 4x4 high-resolution patch of dy."""
    Gu, Rd = _m(_GU, dy), _m(_RD, dy)
    N, K, H2, W2 = dy.shape
    T = torch.einsum('pa,nkijab,qb->kpqnij', Rd, patches(F.pad(dy, (1, 1, 1, 1)), 4, 4, 2, 2), Rd).reshape(1, 9 * K, N, H2 // 2, W2 // 2)
    U = torch.einsum('pa,kcab,qb->ckpq', Gu, w[:, rows], Gu).reshape(len(rows), 9 * K, 1, 1, 1)
    return chain(U, T).reshape(len(rows), -1)


def ups9_wgrad(dy, x, rows):
    """dU = chain over the low-resolution pixels of dM V, dM = A D A^T of the 2x2 block of dy, V as in the forward; dw = G^T dU G."""
    Gu, Bd, Au = _m(_GU, x), _m(_BD, x), _m(_AU, x)
    d, xs = _pairs(dy, x, rows)
    dM = torch.einsum('ap,nrijab,bq->rnijpq', Au, patches(d, 2, 2, 2, 2), Au).reshape(len(rows), -1, 3, 3)
    V = torch.einsum('pa,nrijab,qb->rnijpq', Bd, patches(F.pad(xs, (1, 1, 1, 1)), 3, 3, 1, 1), Bd).reshape(len(rows), -1, 3, 3)
    return torch.einsum('pa,rpq,qb->rab', Gu, chain(dM, V), Gu).reshape(len(rows), 9)


FWD_ALG = {'direct': None, 'wino1d': wino1d_fwd, 'wino2d': wino2d_fwd, 'ups9': ups9_fwd}
WGRAD_ALG = {'direct': None, 'wino1d': wino1d_wgrad, 'wino2d': wino2d_wgrad, 'ups9': ups9_wgrad}


# ---- the case builders ------------------------------------------------------------------------------------------------------
def conv_fwd_case(family, seed, N, C, M, H, W, spec=SAME3, alg='direct', epi='full', alpha=1.0, post=0.7):
    """epi 'full': post * (conv + bias + tadd + res); 'bias': conv + bias; 'acc': alpha * conv + prev; 'none'.  Rows: output channel."""
    Ho, Wo = out_hw(spec, H, W)
    specs = dict(x=((N, C, H, W), 1.0, {1: 'con:x'}, 1),
                 w=((M, C, spec.kh, spec.kw), 1.0 / math.sqrt(C * spec.kh * spec.kw), {0: 'row:k', 1: 'con:w'}, None))
    extra = {'full': ('bias', 'tadd', 'res'), 'bias': ('bias',), 'acc': ('prev',), 'none': ()}[epi]
    shapes = dict(bias=(1, M, 1, 1), tadd=(N, M, 1, 1), res=(N, M, Ho, Wo), prev=(N, M, Ho, Wo))
    for n in extra:
        specs[n] = (shapes[n], 1.0, {1: 'row:k'}, None)
    o = draw(family, seed, specs)
    if alg == 'direct':
        f = lambda o, rows: corr_chain(conv_input(o['x'], spec), o['w'], spec.stride, rows)
    else:
        assert spec in (SAME3, UPS3) and (alg == 'ups9') == bool(spec.ups)
        f = lambda o, rows: FWD_ALG[alg](o['x'], o['w'], rows)
    return Case('conv_fwd/' + alg, (N, C, M, H, W) + tuple(spec) + (epi,), family, o, lambda o: conv_plain(o['x'], o['w'], spec), f, (1,),
                alpha=alpha if epi == 'acc' else 1.0, post=post if epi == 'full' else 1.0, addends=extra)


def conv_dgrad_case(family, seed, N, K, C, Ho, Wo, spec=SAME3, alg='direct', in_hw=None, acc=False, alpha=1.0, lowres=False):
    """dx [N, C, in_hw] from dy [N, K, Ho, Wo] (K = the convolution's output channels); acc: alpha * dx + prev.  Rows: input channel.
    lowres (the nine-product kernel): the gradient w.r.t. the input BEFORE the nearest upsample."""
    in_hw = in_hw or (Ho, Wo)
    specs = dict(dy=((N, K, Ho, Wo), 1.0, {1: 'con:dy'}, 1),
                 w=((K, C, spec.kh, spec.kw), 1.0 / math.sqrt(K * spec.kh * spec.kw), {1: 'row:c', 0: 'con:w'}, None))
    if acc:
        specs['prev'] = ((N, C) + ((in_hw[0] // 2, in_hw[1] // 2) if lowres else tuple(in_hw)), 1.0, {1: 'row:c'}, None)
    o = draw(family, seed, specs)

    def plain(o):
        dx = dgrad_plain(o['dy'], o['w'], spec, in_hw)
        return dx.unfold(2, 2, 2).unfold(3, 2, 2).sum((4, 5)) if lowres else dx

    if alg == 'direct':
        f = lambda o, rows: corr_chain(*dgrad_as_conv(o['dy'], o['w'], spec, in_hw), 1, rows)
    elif alg == 'ups9':
        f = lambda o, rows: ups9_dgrad(o['dy'], o['w'], rows)
    else:
        f = lambda o, rows: FWD_ALG[alg](o['dy'], o['w'].flip(2, 3).transpose(0, 1).contiguous(), rows)
    return Case('conv_dgrad/' + alg, (N, K, C, Ho, Wo) + tuple(spec) + (acc,), family, o, plain, f, (1,), alpha=alpha if acc else 1.0,
                addends=('prev',) if acc else ())


def conv_wgrad_case(family, seed, N, C, K, H, W, spec=SAME3, alg='direct', acc=False, alpha=1.0):
    """gw [K, C, kh, kw] from dy [N, K, Ho, Wo] and x [N, C, H, W]; acc: alpha * gw + prev, prev scaled like its row.  Rows: (k, c)."""
    Ho, Wo = out_hw(spec, H, W)
    specs = dict(dy=((N, K, Ho, Wo), 1.0, {1: 'row:k', 0: 'con:n'}, 1), x=((N, C, H, W), 1.0, {1: 'row:c'}, 1))
    if acc:
        specs['prev'] = ((K, C, spec.kh, spec.kw), math.sqrt(N * Ho * Wo), {0: 'row:k', 1: 'row:c'}, None)
    o = draw(family, seed, specs)
    if alg == 'direct':
        f = lambda o, rows: wgrad_chain(o['dy'], o['x'], spec, rows)
    else:
        f = lambda o, rows: WGRAD_ALG[alg](o['dy'], o['x'], rows)
    return Case('conv_wgrad/' + alg, (N, C, K, H, W) + tuple(spec) + (acc,), family, o, lambda o: wgrad_plain(o['dy'], o['x'], spec), f,
                (0, 1), alpha=alpha if acc else 1.0, addends=('prev',) if acc else ())


def bmm_case(family, seed, which, Z, M, K, Nn, alpha=1.0, acc=False, col_bias=False):
    """out[z, m, n] = alpha * sum_k A[z, m, k] B[z, k, n] (+ prev | + col_bias[n]); tn: a is stored [Z, K, M]; nt: b is stored [Z, Nn, K].
    Rows: one output row of one batch; the rows of A carry the row scales."""
    a_shape, a_axes = ((Z, K, M), {2: 'row:m', 1: 'con:a'}) if which == 'tn' else ((Z, M, K), {1: 'row:m', 2: 'con:a'})
    b_shape, b_axes = ((Z, Nn, K), {2: 'con:b'}) if which == 'nt' else ((Z, K, Nn), {1: 'con:b'})
    specs = dict(a=(a_shape, 1.0, a_axes, None), b=(b_shape, 1.0, b_axes, 2 if which == 'nt' else 1))
    if acc:
        specs['prev'] = ((Z, M, Nn), 1.0, {1: 'row:m'}, None)
    if col_bias:
        specs['cb'] = ((1, 1, Nn), 1.0, {}, None)
    o = draw(family, seed, specs)
    A = (lambda o: o['a'].transpose(1, 2)) if which == 'tn' else (lambda o: o['a'])
    B = (lambda o: o['b'].transpose(1, 2)) if which == 'nt' else (lambda o: o['b'])

    def f(o, rows):
        a = A(o).reshape(Z * M, K)[rows]
        return chain(a[:, :, None], B(o)[[r // M for r in rows]])

    return Case('bmm_' + which, (Z, M, K, Nn, acc, col_bias), family, o, lambda o: torch.bmm(A(o), B(o)), f, (0, 1), alpha=alpha,
                addends=(('prev',) if acc else ()) + (('cb',) if col_bias else ()))


def linear_case(family, seed, what, N, Ci, Co, alpha=1.0, acc=False):
    """fwd: y[n, o] = x w^T + b, rows o; dgrad: dx[n, i] = dy w (+ prev), rows i; wgrad: gw[o, i] = alpha dy^T x + prev, rows (o, i)."""
    if what == 'fwd':
        specs = dict(x=((N, Ci), 1.0, {1: 'con:x'}, 1), w=((Co, Ci), Ci ** -0.5, {0: 'row:o', 1: 'con:w'}, None), b=((1, Co), 1.0, {1: 'row:o'}, None))
        plain, add, rd = (lambda o: o['x'] @ o['w'].t()), ('b',), (1,)
        f = lambda o, rows: chain(o['w'][rows][:, :, None], o['x'].t()[None])
    elif what == 'dgrad':
        specs = dict(dy=((N, Co), 1.0, {1: 'con:dy'}, 1), w=((Co, Ci), Ci ** -0.5, {1: 'row:i', 0: 'con:w'}, None))
        if acc:
            specs['prev'] = ((N, Ci), 1.0, {1: 'row:i'}, None)
        plain, add, rd = (lambda o: o['dy'] @ o['w']), (('prev',) if acc else ()), (1,)
        f = lambda o, rows: chain(o['w'].t()[rows][:, :, None], o['dy'].t()[None])
    else:
        specs = dict(dy=((N, Co), 1.0, {1: 'row:o', 0: 'con:n'}, 1), x=((N, Ci), 1.0, {1: 'row:i'}, 1),
                     prev=((Co, Ci), math.sqrt(N), {0: 'row:o', 1: 'row:i'}, None))
        plain, add, rd = (lambda o: o['dy'].t() @ o['x']), ('prev',), (0, 1)
        f = lambda o, rows: chain(o['dy'].t()[[r // Ci for r in rows]], o['x'].t()[[r % Ci for r in rows]])[:, None]
    return Case('linear_' + what, (N, Ci, Co, acc), family, draw(family, seed, specs), plain, f, rd, alpha=alpha, addends=add)


def attention_case(family, seed, N, heads, d, dv, H, W):
    """o[n, h dv + c, i] = sum_j v[n, h dv + c, j] softmax_j(scale q_i . k_j).  Rows: (image, value channel); cond = softmax64 |v|: q and k
    keep their signs and their scale (the V channels carry the row scales; the contraction runs over tokens: no channel scale to add)."""
    T, scale = H * W, float(d) ** -0.5
    o = draw(family, seed, dict(q=((N, heads * d, H, W), 1.0, {}, None), k=((N, heads * d, H, W), 1.0, {}, None),
                                v=((N, heads * dv, H, W), 1.0, {1: 'row:c'}, 1)))

    def probs(o):
        qd, kd = (o[n].reshape(N * heads, d, T) for n in ('q', 'k'))
        return (scale * torch.bmm(qd.transpose(1, 2), kd)).softmax(-1)                  # [N heads, i, j]

    def plain(o):
        return torch.bmm(o['v'].reshape(N * heads, dv, T), probs(o).transpose(1, 2)).reshape(N, heads * dv, H, W)

    def f(o, rows):
        v = o['v'].reshape(N * heads * dv, T)[rows]
        return chain(v[:, :, None], probs(o).transpose(1, 2)[[r // dv for r in rows]])

    return Case('attention', (N, heads, d, dv, T), family, o, plain, f, (0, 1), signed=('q', 'k'))


# ---- importance -------------------------------------------------------------------------------------------------------------
WG_LO, WG_HI = -3.0, 3.0          # (w g)^2 of four scales: 10^U(-4, 4) would reach 1e32 per term before the sum


def wg_terms(w, g, mode):
    t = w * g
    return {0: t * t, 1: t.abs(), 2: t, 3: t.abs(), 4: g * g, 5: t}[mode]


def wg_plain(w, g, dim, mode):
    t = wg_terms(w, g, mode)
    if mode == 3:
        return t
    s = (t if dim == 0 else t.transpose(0, 1)).flatten(1).sum(1)
    return s.abs() if mode == 2 else s


def wg_case(family, seed, shape, dim, mode, acc):
    """Taylor / Fisher channel reduction of one member; rows: each output element.  The reduced channel axis of w and of g carries a
    row scale each, the other one a contraction scale each."""
    if mode == 3:
        specs = dict(w=(shape, 1.0, {0: 'row:w'}, None), g=(shape, 1.0, {0: 'row:g'}, None))
    else:
        specs = dict(w=(shape, 1.0, {dim: 'row:w', 1 - dim: 'con:w'}, None), g=(shape, 1.0, {dim: 'row:g', 1 - dim: 'con:g'}, None))
    if acc:
        specs['prev'] = ((shape[0 if mode == 3 else dim],), 1.0, {}, None)
    o = draw(family, seed, specs, WG_LO, WG_HI)
    if acc:                                                    # the previous score, scaled like the row it is added to
        with torch.no_grad():
            o['prev'] = (o['prev'].double().abs() * wg_plain(o['w'].double().abs(), o['g'].double().abs(), dim, mode)).float()

    def f(o, rows):
        t = wg_terms(o['w'], o['g'], mode)
        if mode == 3:
            return t[rows][:, None]
        t = (t if dim == 0 else t.transpose(0, 1)).flatten(1)[rows]
        s = chain(t[:, :, None], torch.ones(1, t.shape[1], 1, dtype=t.dtype))
        return s.abs() if mode == 2 else s

    return Case('wg_reduce', tuple(shape) + (dim, mode, acc), family, o, lambda o: wg_plain(o['w'], o['g'], dim, mode), f, (0,),
                addends=('prev',) if acc else ())


def group_members(n0, n_members):
    """The member table of tests/test_dispatch_parity_gpu.py's group_score case: (shape, dim, mode, index list or None) per member."""
    out = []
    for i in range(n_members):
        kind, mode = i % 4, (0, 1, 2, 0, 4, 5)[i % 6]
        if kind == 0:
            out.append(((n0,), 0, 3, None))
        elif kind == 1:
            out.append(((n0, 5 + i, 3, 3), 0, mode, None))
        elif kind == 2:
            out.append(((7 + i, n0, 3, 3), 1, mode, None))
        else:
            out.append(((11, n0 + 16, 1, 1), 1, mode, sorted((3 * j + i) % (n0 + 16) for j in range(n0))))
    return out


def group_case(family, seed, n0, n_members):
    """One group's score: the sum over its members of their channel reductions (an index list picks the channels of a wider layer).
    Rows: each of the n0 scores.  Every member's pruned axis carries a row scale of its own per tensor."""
    members = group_members(n0, n_members)
    specs = {}
    for i, (shape, dim, mode, idxs) in enumerate(members):
        for t in 'wg':
            axes = {0: 'row:%s%d' % (t, i)} if mode == 3 else {dim: 'row:%s%d' % (t, i), 1 - dim: 'con:%s%d' % (t, i)}
            specs['%s%d' % (t, i)] = (shape, 1.0, axes, None)
    o = draw(family, seed, specs, WG_LO, WG_HI)

    def member(o, i, red):
        shape, dim, mode, idxs = members[i]
        s = red(o['w%d' % i], o['g%d' % i], dim, mode)
        return s if idxs is None else s[idxs]

    def plain(o):
        return sum(member(o, i, wg_plain) for i in range(n_members))

    def f(o, rows):
        def red(w, g, dim, mode):
            t = wg_terms(w, g, mode)
            if mode == 3:
                return t
            t = (t if dim == 0 else t.transpose(0, 1)).flatten(1)
            s = chain(t[:, :, None], torch.ones(1, t.shape[1], 1, dtype=t.dtype))[:, 0]
            return s.abs() if mode == 2 else s
        acc = member(o, 0, red)
        for i in range(1, n_members):
            acc = acc + member(o, i, red)
        return acc[rows][:, None]

    c = Case('group_score', (n0, n_members), family, o, plain, f, (0,))
    c.members = members
    return c
