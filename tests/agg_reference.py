"""fp64 reference of the PNA aggregation / readout (csrc/aggregate.hip: K4, K6) with a DERIVED per-element error bound,
and the one input set the bound tests share (tests/test_aggregate_bounds_cpu.py, tests/test_gpu_aggregate.py).

numpy / torch on the CPU only; the HIP library is never loaded from here.

The operation (top of the kernels): per destination node v with the D message rows x_0 .. x_{D-1} = m[in_ptr[v] : in_ptr[v+1]]
    sum, mean = sum / D, max, min, var = max(mean(x^2) - mean^2, 0), std = sqrt(var + eps)          eps = float32(1e-5)
each times the degree scalers {1, log(D+1)/avg, avg/log(D+1)} (scaler-major, aggregator-minor blocks of F columns); nodes
without rows give zero rows; a single configured scaler is not applied unless forced.  avg is the float the C ABI takes.
Backward: d x_j = g_mean/D + g_sum + g_max [j = first argmax] + g_min [j = first argmin] + k (x_j - mean),
    k = [var > 0] (g_std / (D std) + 2 g_var / D),    g_a = sum over scaler blocks of scale_s * grad_out[s, a].

The tolerance is no chosen number: it is the first-order rounding bound of ANY fp32 evaluation of these formulas (any
summation order), per output element, computed in fp64 from the inputs with u = 2^-24 and a slack of 1.01 on every u.
With S1 = sum |x|, S2 = sum x^2, msq = S2 / D:
    e_sum  = (D-1) u S1
    e_mean = e_sum / D + u |mean|
    e_msq  = D u S2 / D + u msq
    e_var  = e_msq + 2 |mean| e_mean + e_mean^2 + u mean^2 + u (|msq - mean^2| + e_msq)
    e_std  = e_var / (sqrt(max(var - e_var, 0) + eps) + std) + 3 u std
    max, min: 0 (comparisons of fp32 values are exact);   a scaled block a * s: |s| e_a + 2 u |a s|
    backward element (j, f):
      8 u (G_mean/D + G_sum + K |x_j - mean| + [j = amax] G_max + [j = amin] G_min)
      + |k| (e_mean + u |x_j|) + e_k (|x_j - mean| + e_mean),
      e_k = |g_std| / (D std) (e_std / (std - e_std) + 3 u) + 6 u |g_var| / D
      G_a = sum over scaler blocks of |scale_s * grad_out[s, a]| and K = k formed from G_std, G_var: g_a is itself an fp32 sum
      of rounded products, accurate to the sum of its |terms| and not to its own size (with one block per aggregator
      G_a = |g_a|; with the three blocks of the standard configuration the terms cancel to 1 % of their size in 1 % of the
      elements, and an evaluation in the kernels' own order is then outside a bound that has |g_a| in this place)
    and where var <= e_var the fp32 `raw > 0` test can fall either way: the element is AMBIGUOUS and gets
      (|g_std| / (D sqrt(eps)) + 2 |g_var| / D) (|x_j - mean| + e_mean) IN PLACE of the e_k term (e_k divides by
      std - e_std, which is not positive next to var = 0; the reference's and the computed k both lie between 0 and that
      factor there, with the same sign, so it bounds their distance by itself).
amax / amin are the first index of the extremum of m - from m alone, never from the output under test.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

U = 1.01 * 2.0 ** -24
EPS = float(np.float32(1e-5))


def _np64(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def effective_scalers(scalers, force_scalers):
    """reference models/pna.py:232: scalers are only applied when more than one is configured"""
    return list(scalers) if (len(scalers) > 1 or force_scalers) else ['identity']


def scaler_value(name, D, avg_d_log):
    """fp64 factor of a scaler block (None: identity, no product at all); avg is the fp32 value the C ABI receives"""
    if name == 'identity':
        return None
    avg = float(np.float32(avg_d_log))
    l = math.log(D + 1)
    return l / avg if name == 'amplification' else avg / l


def _node_stats(x):
    """fp64 statistics and error terms of one node's rows x [D, F]"""
    D = x.shape[0]
    s = SimpleNamespace(D=D)
    S1, S2 = np.abs(x).sum(0), (x * x).sum(0)
    s.sum = x.sum(0)
    s.mean = s.sum / D
    s.msq = S2 / D
    s.const = (x == x[0]).all(0)                                    # var == 0 exactly, and only there
    s.var = np.where(s.const, 0.0, ((x - s.mean) ** 2).mean(0))      # (centred form: no cancellation in the reference itself)
    s.std = np.sqrt(s.var + EPS)
    s.max, s.min = x.max(0), x.min(0)
    s.e_sum = (D - 1) * U * S1
    s.e_mean = s.e_sum / D + U * np.abs(s.mean)
    s.e_msq = D * U * S2 / D + U * s.msq
    s.e_var = (s.e_msq + 2 * np.abs(s.mean) * s.e_mean + s.e_mean ** 2 + U * s.mean ** 2
               + U * (np.abs(s.msq - s.mean ** 2) + s.e_msq))
    s.e_std = s.e_var / (np.sqrt(np.maximum(s.var - s.e_var, 0.0) + EPS) + s.std) + 3 * U * s.std
    return s


def reference_fwd(m, in_ptr, aggs, scalers, avg_d_log=1.0, force_scalers=False):
    """(ref64, bound), both [N, n_scaler_blocks * len(aggs) * F] float64 arrays; m [E, F]: the messages as the kernel sees them"""
    x_all = _np64(m)
    ptr = np.asarray(in_ptr, dtype=np.int64)
    N, F = ptr.shape[0] - 1, x_all.shape[1]
    eff = effective_scalers(scalers, force_scalers)
    nblk = len(eff) * len(aggs)
    ref, bound = np.zeros((N, nblk, F)), np.zeros((N, nblk, F))
    zero = np.zeros(F)
    for v in range(N):
        beg, end = int(ptr[v]), int(ptr[v + 1])
        if end <= beg:
            continue
        st = _node_stats(x_all[beg:end])
        val = {'sum': (st.sum, st.e_sum), 'mean': (st.mean, st.e_mean), 'max': (st.max, zero), 'min': (st.min, zero),
               'var': (st.var, st.e_var), 'std': (st.std, st.e_std)}
        for si, sname in enumerate(eff):
            sc = scaler_value(sname, st.D, avg_d_log)
            for k, a in enumerate(aggs):
                a_val, a_err = val[a]
                b = si * len(aggs) + k
                if sc is None:
                    ref[v, b], bound[v, b] = a_val, a_err
                else:
                    ref[v, b] = a_val * sc
                    bound[v, b] = abs(sc) * a_err + 2 * U * np.abs(a_val * sc)
    return ref.reshape(N, nblk * F), bound.reshape(N, nblk * F)


def reference_bwd(m, in_ptr, grad_out, aggs, scalers, avg_d_log=1.0, force_scalers=False, return_ambiguous=False):
    """(ref64, bound) [E, F] float64 arrays (and the boolean mask of the ambiguous elements on request);
    grad_out [N, n_scaler_blocks * len(aggs) * F] in the [block][feature] column order"""
    x_all = _np64(m)
    ptr = np.asarray(in_ptr, dtype=np.int64)
    N, F = ptr.shape[0] - 1, x_all.shape[1]
    eff = effective_scalers(scalers, force_scalers)
    nblk = len(eff) * len(aggs)
    go = _np64(grad_out).reshape(N, nblk, F)
    ref, bound = np.zeros_like(x_all), np.zeros_like(x_all)
    amb = np.zeros(x_all.shape, dtype=bool)
    for v in range(N):
        beg, end = int(ptr[v]), int(ptr[v + 1])
        if end <= beg:
            continue
        x = x_all[beg:end]
        st = _node_stats(x)
        D = st.D
        g = {a: np.zeros(F) for a in ('sum', 'mean', 'max', 'min', 'var', 'std')}
        G = {a: np.zeros(F) for a in g}                   # sum of the |terms| of g_a: what an fp32 sum of them is accurate to
        for si, sname in enumerate(eff):
            sc = scaler_value(sname, D, avg_d_log)
            for k, a in enumerate(aggs):
                term = go[v, si * len(aggs) + k] * (1.0 if sc is None else sc)
                g[a], G[a] = g[a] + term, G[a] + np.abs(term)
        rows = np.arange(D)[:, None]
        is_max = rows == np.argmax(x, 0)[None, :]          # np.argmax / argmin: the first occurrence
        is_min = rows == np.argmin(x, 0)[None, :]
        k_ = np.where(st.const, 0.0, g['std'] / (D * st.std) + 2 * g['var'] / D)     # relu'(0) = 0
        dx = x - st.mean
        ref[beg:end] = g['mean'] / D + g['sum'] + is_max * g['max'] + is_min * g['min'] + k_ * dx
        a_ = st.var <= st.e_var
        # (e_k is a relative-error form: it needs e_std < std, which fails next to var = 0 - there both the reference's and the
        # computed factor lie between 0 and the ambiguous term's factor, which bounds their distance by itself)
        e_k = np.where(a_, 0.0, np.abs(g['std']) / (D * st.std) * (st.e_std / np.where(a_, 1.0, st.std - st.e_std) + 3 * U)
                       + 6 * U * np.abs(g['var']) / D)
        K_ = np.where(st.const, 0.0, G['std'] / (D * st.std) + 2 * G['var'] / D)
        b = (8 * U * (G['mean'] / D + G['sum'] + K_ * np.abs(dx) + is_max * G['max'] + is_min * G['min'])
             + np.abs(k_) * (st.e_mean + U * np.abs(x)) + e_k * (np.abs(dx) + st.e_mean))
        b = b + a_ * (np.abs(g['std']) / (D * math.sqrt(EPS)) + 2 * np.abs(g['var']) / D) * (np.abs(dx) + st.e_mean)
        bound[beg:end] = b
        amb[beg:end] = a_[None, :]
    return (ref, bound, amb) if return_ambiguous else (ref, bound)


def worst_ratio(out, ref, bound):
    """max over the elements of |out - ref| / bound (inf where an element with bound 0 is not exact, or is not finite)"""
    err = np.abs(_np64(out) - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(err), ratio, np.inf)
    return float(ratio.max()) if ratio.size else 0.0


def zero_rows_are_plus_zero(out, in_ptr):
    """rows of nodes without messages: exactly +0.0 in every column"""
    o = _np64(out)
    deg = np.diff(np.asarray(in_ptr, dtype=np.int64))
    z = o[deg == 0]
    return bool(np.all(z == 0.0) and not np.signbit(z).any())


# ---- the shared inputs ------------------------------------------------------------------------------------------------------
AVG = float(np.float32(1.3))
DEGREE_CYCLE = [0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 31, 32, 33, 64, 101]
CONSTANT_DEGREE = 9                      # the three nodes of this degree have all rows equal: the ambiguous class

STD_AGGS = ('mean', 'max', 'min', 'std')
GEN_AGGS = ('sum', 'var', 'max', 'mean', 'min', 'std')
CONFIGS = {                              # name: (aggregators, scalers, force_scalers)
    'std12': (STD_AGGS, ('identity', 'amplification', 'attenuation'), False),      # MODE 1
    'ident4': (STD_AGGS, ('identity',), False),                                    # MODE 2
    'general': (GEN_AGGS, ('attenuation', 'identity'), False),                     # MODE 0
    'forced_amp': (GEN_AGGS, ('amplification',), True),                            # MODE 0, one scaler, applied
    'readout': (('min', 'max', 'mean', 'sum'), ('identity',), False),              # K6
}


def _case(config, F, form, tower_feat=0):
    return SimpleNamespace(id=f'{config}-F{F}-{form}', config=config, F=F, form=form, tower_feat=tower_feat)


CASES = ([_case('std12', F, form) for F in (4, 20, 200) for form in ('fp32', 'bf16', 'aff', 'aff_bf16')]
         + [_case('ident4', F, form) for F in (20, 200) for form in ('fp32', 'bf16', 'aff')]
         + [_case(c, F, 'fp32') for F in (20, 7) for c in ('general', 'forced_amp')]
         + [_case('std12', F, 'aff') for F in (340, 344)]
         + [_case(c, 36, 'tower', 12) for c in ('std12', 'ident4', 'general', 'forced_amp')]
         + [_case('readout', F, 'readout') for F in (200, 7)])
CASE_IDS = [c.id for c in CASES]


def graph_in_ptr():
    deg = [0] + DEGREE_CYCLE * 3 + [0]
    ptr = np.zeros(len(deg) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(deg)
    return ptr


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def make_messages(F, in_ptr, seed):
    """randn * 3 + 1; row 1 of every node with D >= 2 copies row 0 (an exact tie); row D-1 of those nodes holds the column's
    maximum + 10 in feature 0 and its minimum - 10 in feature 1 (the extremum and its gradient sit in the tail of the last
    trip); the nodes of degree 9 are constant; the third row of a node of degree 3 is at least 0.5 away from the tied pair"""
    e = _randn(int(in_ptr[-1]), F, seed=seed) * 3 + 1
    for v in range(in_ptr.shape[0] - 1):
        beg, end = int(in_ptr[v]), int(in_ptr[v + 1])
        if end - beg < 2:
            continue
        e[beg + 1] = e[beg]
        if end - beg == 3:               # the one free row keeps its distance from the tied pair: no column is constant to
            d = e[beg + 2] - e[beg]      # within fp32 rounding by chance (at F = 200 that happens in every second draw)
            e[beg + 2] = e[beg] + torch.where(d >= 0, d + 0.5, d - 0.5)
        e[end - 1, 0] = e[beg:end, 0].max() + 10
        e[end - 1, 1] = e[beg:end, 1].min() - 10
        if end - beg == CONSTANT_DEGREE:
            e[beg:end] = e[beg]
    return e.contiguous()


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """Everything a case needs, built once: e (what the kernel is given: fp32 or bf16), aff ([3, F] or None), m (fp32: the messages
    as the kernel sees them), in_ptr (int32 numpy), cot ([N, blocks * F], [block][feature] columns), the configuration, and the
    fp64 references with their bounds.  Nothing in it may be modified."""
    case = CASES[CASE_IDS.index(case_id)]
    aggs, scalers, force = CONFIGS[case.config]
    F = case.F
    in_ptr = graph_in_ptr()
    e = make_messages(F, in_ptr, seed=3000 + F)
    aff = None
    if case.form in ('bf16', 'aff_bf16'):
        e = e.bfloat16()                 # bf16-representable values; copies stay copies, the +-10 gaps stay gaps
    m = e.float()
    if case.form in ('aff', 'aff_bf16'):
        aff = torch.stack([_randn(F, seed=4) + 1.0, 1 + 0.3 * _randn(F, seed=5), 0.3 * _randn(F, seed=6)])
        aff[1, ::7] *= -1                # negative scales: max and min swap roles
        aff = aff.contiguous()
        m = ((m - aff[0]) * aff[1] + aff[2]).contiguous()      # the kernel's arithmetic: sub, mul, add, each rounded to fp32
    avg = 1.0 if case.config == 'readout' else AVG
    nblk = len(effective_scalers(scalers, force)) * len(aggs)
    N = in_ptr.shape[0] - 1
    cot = _randn(N, nblk * F, seed=2000 + F).contiguous()
    fwd = reference_fwd(m, in_ptr, aggs, scalers, avg, force)
    bwd = reference_bwd(m, in_ptr, cot, aggs, scalers, avg, force, return_ambiguous=True)
    return SimpleNamespace(case=case, aggs=list(aggs), scalers=list(scalers), force=force, avg=avg, F=F, N=N, nblk=nblk,
                           in_ptr=in_ptr, e=e, aff=aff, m=m, cot=cot, ref_fwd=fwd[0], bound_fwd=fwd[1], ref_bwd=bwd[0],
                           bound_bwd=bwd[1], ambiguous=bwd[2])


def constant_elements(m, in_ptr):
    """mask [E, F] of the elements whose column is constant inside its node (var = 0 exactly): by construction the nodes of
    degree 1, the nodes of degree 2 outside features 0 / 1 (row 1 copies row 0) and the constant nodes of degree 9"""
    x = _np64(m)
    out = np.zeros(x.shape, dtype=bool)
    for v in range(in_ptr.shape[0] - 1):
        beg, end = int(in_ptr[v]), int(in_ptr[v + 1])
        if end > beg:
            out[beg:end] = (x[beg:end] == x[beg]).all(0)[None, :]
    return out


def to_tower_major(t, nblk, tower_feat):
    """[N, [block][tower][feature]] -> [N, [tower][block][feature]] (i3d_pna_aggregate_fwd_towers' row)"""
    N = t.shape[0]
    T = t.shape[1] // (nblk * tower_feat)
    return t.reshape(N, nblk, T, tower_feat).transpose(0, 2, 1, 3).reshape(N, -1) if isinstance(t, np.ndarray) \
        else t.reshape(N, nblk, T, tower_feat).permute(0, 2, 1, 3).reshape(N, -1).contiguous()
