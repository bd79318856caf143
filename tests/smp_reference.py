"""Host mirror of the SMP geometry, bases and triplet interaction (3dinfomax_amd/smp.py, csrc/smp.hip), written from the formulas:
numpy for the geometry, scipy.special.spherical_jn / lpmv for the bases, torch (autograd) for the interaction.  Every stage runs in
fp64 or in fp32 (`dtype`): the fp32 run is the yardstick of the device tests' bound  max |kernel - fp64| <= max(4 x max |fp32 - fp64|,
2^-20 x largest magnitude).

One decision is made in fp32 in BOTH runs, as on the device: which atoms lie within the cutoff (d2 = (dx dx + dy dy) + dz dz < cutoff^2 on
fp32 coordinates).  It defines the input lists; a pair within rounding of the cutoff would otherwise give the two runs different graphs.

Conventions (smp.py's module docstring): at most MAX_NBR in-neighbours per atom, the lowest indices kept; edges sorted by destination,
sources ascending; triplets (k -> j, j -> i), k != i, grouped by ji, k ascending; torsion = min over the in-neighbours k_n != i of j of the
wrapped dihedral, the candidate k_n == k being exactly 2 pi; harmonics per l as [m = 0, cos m = 1..l, sin m = l..1]; flat harmonic f
times the Bessel order f % n; no envelope.
"""
import math

import numpy as np
import torch
from scipy.optimize import brentq
from scipy.special import lpmv, spherical_jn

MAX_NBR = 32
TWO_PI = 2 * math.pi


# ---- lists -------------------------------------------------------------------------------------------------------------------------
def radius_graph(pos, sizes, cutoff):
    """pos [N, 3] fp32, sizes: atoms per molecule -> src, dst [E] int64 (edges src -> dst), in_ptr [N + 1]"""
    pos = np.asarray(pos, dtype=np.float32)
    r2 = np.float32(cutoff) * np.float32(cutoff)
    src, dst, deg = [], [], []
    a0 = 0
    for n in sizes:
        p = pos[a0:a0 + n]
        d = p[:, None, :] - p[None, :, :]                     # [i, j]: pos_i - pos_j
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        for i in range(n):
            near = [j for j in range(n) if j != i and d2[i, j] < r2][:MAX_NBR]
            src += [a0 + j for j in near]
            dst += [a0 + i] * len(near)
            deg.append(len(near))
        a0 += n
    in_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), in_ptr


def triplets(src, dst, in_ptr):
    """-> idx_kj, idx_ji [T], trip_ptr [E + 1]"""
    kj, ji, cnt = [], [], []
    for e in range(src.shape[0]):
        j, i = src[e], dst[e]
        ps = [p for p in range(in_ptr[j], in_ptr[j + 1]) if src[p] != i]
        kj += ps
        ji += [e] * len(ps)
        cnt.append(len(ps))
    return np.array(kj, dtype=np.int64), np.array(ji, dtype=np.int64), np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)


# ---- angle and torsion -----------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def angles(pos, src, dst, in_ptr, trip_ptr, dtype):
    """-> dist [E], angle [T], torsion [T] in `dtype`, margin [T] (fp64-meaningful: the smallest |raw dihedral| over the candidates
    k_n != k of a triplet, i.e. its distance to the 0 / 2 pi wrap; inf without such a candidate), single [T]: k_n == k is the only candidate"""
    pos = np.asarray(pos, dtype=np.float32).astype(dtype)
    two_pi = dtype(TWO_PI)
    E, T = src.shape[0], int(trip_ptr[-1])
    d = pos[dst] - pos[src]
    dist = np.sqrt(_dot(d, d))
    angle, torsion = np.zeros(T, dtype=dtype), np.zeros(T, dtype=dtype)
    margin, single = np.full(T, np.inf), np.zeros(T, dtype=bool)
    for e in range(E):
        t0, t1 = trip_ptr[e], trip_ptr[e + 1]
        if t1 == t0:
            continue
        j, i = src[e], dst[e]
        nb = src[in_ptr[j]:in_ptr[j + 1]]
        ks = nb[nb != i]
        ji = pos[i] - pos[j]
        jk = pos[ks] - pos[j]                                   # [K, 3]: the triplets' k and, the same set, the candidates k_n
        plane = _cross(ji[None, :], jk)                         # [K, 3]
        angle[t0:t1] = np.arctan2(np.sqrt(_dot(plane, plane)), _dot(ji[None, :], jk))
        a = _dot(plane[:, None, :], plane[None, :, :])          # [k, k_n]
        b = _dot(_cross(plane[:, None, :], plane[None, :, :]), ji[None, None, :]) / np.sqrt(_dot(ji, ji))
        raw = np.arctan2(b, a)
        tor = np.where(raw <= 0, raw + two_pi, raw).astype(dtype)
        same = np.eye(len(ks), dtype=bool)
        tor[same] = two_pi
        torsion[t0:t1] = tor.min(1)
        if len(ks) > 1:
            margin[t0:t1] = np.where(same, np.inf, np.abs(raw)).min(1)
        else:
            single[t0:t1] = True
    return dist.astype(dtype), angle, torsion, margin, single


# ---- bases -------------------------------------------------------------------------------------------------------------------------
def bessel_tables(n, k):
    """zeros [n, k] (fp32 values) and normalisers [n, k] fp64: the first k zeros of j_l by bracketing between those of j_(l-1)"""
    zeros = np.zeros((n, k), dtype=np.float32)
    zeros[0] = np.arange(1, k + 1) * np.pi
    points = np.arange(1, k + n) * np.pi
    for l in range(1, n):
        points = np.array([brentq(lambda x: spherical_jn(l, x), points[q], points[q + 1]) for q in range(k + n - 1 - l)])
        zeros[l] = points[:k]
    z = zeros.astype(np.float64)
    norm = np.stack([1.0 / np.sqrt(0.5 * spherical_jn(l + 1, z[l]) ** 2) for l in range(n)])
    return zeros, norm


def harmonics(angle, phi, n, dtype):
    """[T, n^2]: per l  [Y_l0, Y_l1^cos .. Y_ll^cos, Y_ll^sin .. Y_l1^sin]; every factor from scipy in fp64, rounded to `dtype`,
    the products in `dtype`"""
    a64, p64 = angle.astype(np.float64), phi.astype(np.float64)
    cols = []
    for l in range(n):
        def pre(m):
            return math.sqrt((2 * l + 1) * math.factorial(l - m) / (4 * math.pi * math.factorial(l + m)))
        cols.append((pre(0) * lpmv(0, l, np.cos(a64))).astype(dtype))
        side = {}
        for m in range(1, l + 1):
            leg = (math.sqrt(2.0) * pre(m) * lpmv(m, l, np.cos(a64))).astype(dtype)
            side[m] = (leg * np.cos(m * p64).astype(dtype), leg * np.sin(m * p64).astype(dtype))
        cols += [side[m][0] for m in range(1, l + 1)] + [side[m][1] for m in range(l, 0, -1)]
    return np.stack(cols, 1)


def bases(dist, angle, torsion, idx_kj, n, k, cutoff, dtype, tables=None):
    """-> sbf [T, n k], t [T, n n k] in `dtype`; tables = (zeros, norm) [n, k] to use instead of bessel_tables (the package rounds
    its normalisers as the reference does, smp.bessel_normalizers: up to 1e-7 off the exact ones)"""
    zeros, norm = bessel_tables(n, k) if tables is None else (np.asarray(tables[0], dtype=np.float32), np.asarray(tables[1], dtype=np.float64))
    x = (dist.astype(dtype) / dtype(cutoff))[:, None, None] * zeros.astype(dtype)[None]            # [E, n, k]
    order = np.arange(n)[None, :, None]
    rbf = (norm[None] * spherical_jn(np.broadcast_to(order, x.shape), x.astype(np.float64))).astype(dtype)
    Y = harmonics(angle, torsion, n, dtype)                                                        # [T, n^2]
    rk = rbf[idx_kj]                                                                               # [T, n, k]
    sbf = rk * Y[:, [l * l for l in range(n)], None]
    t = rk[:, None, :, :] * Y.reshape(-1, n, n)[:, :, :, None]                                     # [T, a, b, k]: harmonic a n + b, order b
    return sbf.reshape(-1, n * k).astype(dtype), t.reshape(-1, n * n * k).astype(dtype)


def geometry(pos, sizes, cutoff, n, k, dtype, tables=None):
    src, dst, in_ptr = radius_graph(pos, sizes, cutoff)
    idx_kj, idx_ji, trip_ptr = triplets(src, dst, in_ptr)
    dist, angle, torsion, margin, single = angles(pos, src, dst, in_ptr, trip_ptr, dtype)
    sbf, t = bases(dist, angle, torsion, idx_kj, n, k, cutoff, dtype, tables)
    return dict(src=src, dst=dst, in_ptr=in_ptr, idx_kj=idx_kj, idx_ji=idx_ji, trip_ptr=trip_ptr, dist=dist, angle=angle,
                torsion=torsion, margin=margin, single=single, sbf=sbf, t=t)


# ---- the triplet interaction -----------------------------------------------------------------------------------------------------------
def interaction(x, s8, t8, w1, w2, idx_kj, idx_ji, grad, dtype):
    """out [E, I] = sum over the triplets of a ji edge of x[idx_kj] * (s8 w1^T) * (t8 w2^T), and the gradients of <out, grad>"""
    leaves = [a.detach().to(dtype).clone().requires_grad_() for a in (x, s8, t8, w1, w2)]
    x, s8, t8, w1, w2 = leaves
    m = x[idx_kj] * (s8 @ w1.T) * (t8 @ w2.T)
    out = torch.zeros_like(x).index_add(0, idx_ji, m)
    g = torch.autograd.grad(out, leaves, grad.to(dtype))
    return dict(out=out.detach(), dx=g[0], ds8=g[1], dt8=g[2], dw1=g[3], dw2=g[4])


SHAPES = [(64, 8), (24, 4), (128, 8), (8, 1)]


def make_interaction_case(I, Bs, seed, lists):
    """inputs of the interaction on the lists of a geometry: x [E, I], s8, t8 [T, Bs], w1, w2 [I, Bs], grad [E, I]"""
    g = torch.Generator().manual_seed(seed)
    E, T = lists['src'].shape[0], lists['idx_kj'].shape[0]
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    return dict(x=r(E, I), s8=r(T, Bs), t8=r(T, Bs), w1=r(I, Bs) / math.sqrt(Bs), w2=r(I, Bs) / math.sqrt(Bs), grad=r(E, I))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def cluster(n=40, radius=2.4, seed=0):
    """n atoms inside a ball whose diameter is below the 5 A cutoff: every atom sees all others, the cap cuts"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * radius * rng.random((n, 1)) ** (1 / 3)).astype(np.float32)
