"""fp64 restatement of the evaluation metrics beside FID that ldm_exp/test_diffusion.py reads from
torch_fidelity.calculate_metrics(isc, kid, prc): Inception Score, Kernel Inception Distance, precision / recall.

torch_fidelity is neither part of the reference tree nor installed, so its arithmetic is RECALLED, NOT PINNED (the position of
TaylorImportance(multivariable=...) and pytorch_msssim, VERDICT rows a10 / f3).  What follows is therefore the specification
diff-pruning_amd/metrics.py is held to; everything is evaluated in float64 with whole N x N matrices (test sizes only)."""
import numpy as np
import torch


def inception_score(logits, splits=10, shuffle=True, rng_seed=2020):
    """logits [N, C] (pool3 . fc.weight^T, no bias).  Returns (mean, population std, the per-split scores)."""
    logits = torch.as_tensor(logits).double()
    n = logits.shape[0]
    if shuffle:
        logits = logits[torch.from_numpy(np.random.RandomState(rng_seed).permutation(n))]
    p = torch.softmax(logits, 1)
    logp = torch.log_softmax(logits, 1)
    scores = []
    for i in range(splits):
        lo, hi = i * n // splits, (i + 1) * n // splits
        pk, lk = p[lo:hi], logp[lo:hi]
        q = pk.mean(0, keepdim=True)
        kl = (pk * (lk - q.log())).sum(1).mean()
        scores.append(float(kl.exp()))
    return float(np.mean(scores)), float(np.std(scores)), scores


def isc_rows(logits):
    """(lse_i, h_i = sum_c p_ic (l_ic - lse_i)) of every row, float64."""
    logits = torch.as_tensor(logits).double()
    lse = torch.logsumexp(logits, 1)
    logp = torch.log_softmax(logits, 1)
    return lse, (logp.exp() * logp).sum(1)


def isc_colmeans(logits, lo, hi):
    return torch.softmax(torch.as_tensor(logits).double()[lo:hi], 1).mean(0)


def kid_subsets(n1, n2, subsets, subset_size, rng_seed=2020):
    if subset_size > n1 or subset_size > n2:
        raise ValueError('subset larger than a set')
    rng = np.random.RandomState(rng_seed)
    out = []
    for _ in range(subsets):
        i1 = rng.choice(n1, subset_size, replace=False)
        i2 = rng.choice(n2, subset_size, replace=False)
        out.append((i1, i2))
    return out


def poly_kernel(x, y, degree=3, gamma=None, coef0=1):
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    return (gamma * (x @ y.t()) + coef0) ** degree


def poly_sums(g, gamma, coef0, degree):
    """(sum, diagonal sum) of (gamma g + coef0)^degree for a Gram block g in float64."""
    k = (gamma * g.double() + coef0) ** degree
    return float(k.sum()), float(torch.diagonal(k).sum())


def mmd2(kxx, kyy, kxy):
    m = kxx.shape[0]
    return float((kxx.sum() - torch.diagonal(kxx).sum() + kyy.sum() - torch.diagonal(kyy).sum()) / (m * (m - 1)) - 2 * kxy.sum() / (m * m))


def kernel_inception_distance(f1, f2, subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1, rng_seed=2020):
    """Returns (mean, population std, the per-subset mmd^2)."""
    f1, f2 = torch.as_tensor(f1).double(), torch.as_tensor(f2).double()
    vals = []
    for i1, i2 in kid_subsets(f1.shape[0], f2.shape[0], subsets, subset_size, rng_seed):
        x, y = f1[torch.from_numpy(i1)], f2[torch.from_numpy(i2)]
        vals.append(mmd2(poly_kernel(x, x, degree, gamma, coef0), poly_kernel(y, y, degree, gamma, coef0),
                         poly_kernel(x, y, degree, gamma, coef0)))
    return float(np.mean(vals)), float(np.std(vals)), vals


def dist2(x, y, gram=None):
    """Squared Euclidean distances in the Gram form max(|x|^2 + |y|^2 - 2 x.y, 0), float64; `gram` replaces x . y^T."""
    x, y = torch.as_tensor(x).double(), torch.as_tensor(y).double()
    g = x @ y.t() if gram is None else torch.as_tensor(gram).double()
    return ((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2 * g).clamp_min(0)


def ksmallest2(x, y, kk, gram=None):
    """The kk smallest squared distances from every row of x to the rows of y, ascending, [rows, kk]."""
    return torch.sort(dist2(x, y, gram), 1).values[:, :kk]


def radii2(a, k, gram=None):
    """Squared (k + 1)-th smallest distance from each row of `a` to all rows of `a`, itself included."""
    return ksmallest2(a, a, k + 1, gram)[:, k]


def inside(b, a, r2, gram=None):
    """bool [Nb]: any_j d2(b_i, a_j) <= r2_j."""
    return (dist2(b, a, gram) <= torch.as_tensor(r2).double()[None, :]).any(1)


def decided(b, a, r2, tau=1e-4):
    """Rows whose flag does not hang on a distance within tau (relative, in the distance itself) of its radius: some
    d_ij <= r_j (1 - tau), or every d_ij >= r_j (1 + tau)."""
    d = dist2(b, a).sqrt()
    r = torch.as_tensor(r2).double().sqrt()[None, :]
    return (d <= r * (1 - tau)).any(1) | (d >= r * (1 + tau)).all(1)


def precision_recall(f1, f2, k=3):
    f1, f2 = torch.as_tensor(f1).double(), torch.as_tensor(f2).double()
    p = float(inside(f1, f2, radii2(f2, k)).double().mean())
    r = float(inside(f2, f1, radii2(f1, k)).double().mean())
    return p, r, (2 * p * r / (p + r) if p + r > 0 else 0.0)
