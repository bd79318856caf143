"""fp64 references of the degree-grouped posttrans products (csrc/gemm.hip: i3d_gemm_f32_grouped, i3d_gemm_f32_fused_src with
m_rows / tile_group / c_in, i3d_gemm_f32_rowsubset_multi, i3d_gemm_f32_grouped_batched; csrc/grouped.hip: the combined weights)
with DERIVED elementwise bounds, and the one set of layouts, shapes and inputs the bound tests share
(tests/test_grouped_bounds_cpu.py, tests/test_gpu_grouped.py).

numpy / torch on the CPU only; the HIP library is never loaded from here (3dinfomax_amd.graph is plain numpy).

The operations, for the rows r listed in m_rows (64-padded per in-degree group with -1, g(r) = tile_group[position / 64]):
    forward        C[r] = act(c_in[r] + bias + A[r] . op(B_g(r)))        op = transpose (trans_b = 1: B_g is [N, K])
    data gradient  the same with trans_b = 0 (B_g is [K, N])
    batched        the T diagonal blocks of it: tower t reads A[r, t a_batch ..], B_g + t b_batch, writes C[r, t c_batch ..]
    weight grad    dW_g = sum_{j in group g} A[k_rows[j]]^T B[k_rows[j]]      (+ the old content when accumulating)
    statistics     per 64-row tile and column {sum, M2 about the tile's own mean, count} of the values that were STORED
    combined W     WD[g] = sum_s c[g][s] W_s      and      dW_s = sum_g c[g][s] dWD[g]
Every reference is a pair (ref, mag): ref the fp64 value, mag the same expression with every operand replaced by its absolute
value, |c_in| + |bias| + sum_k |a_rk| |w_nk|.

Bounds, u = 2^-24, none of them chosen from what a kernel gives:
  products      |out - ref| <= (K + 6) u mag, K the reduction length (a weight gradient: the group's row count).  An fp32 sum of K
                exact or once-rounded products in ANY order, through fp32 atomics or slices, makes at most K - 1 + 1 roundings of
                at most u (partial sum) <= u mag each; the addend, the bias and LeakyReLU's slope add one each; the split form
                (operands in three bf16 parts, six exact part products, gemm.hip:872) drops three part products <= u |a b| each.
                ReLU and LeakyReLU are 1-Lipschitz.  Where mag = 0 (the zero weight of the D = 0 group on top of nothing) the
                output must be exactly 0.
  bf16 mode     the same bound against the fp64 product of the RNE-bf16-rounded operands (products of bf16 values are exact in
                fp32): the rounding is in the reference, the bound is not widened.
  statistics    count exact;  |sum - ref| <= cnt u sum|x|;  |M2 - ref| <= (cnt + 4) u M2_ref + 4 cnt (u sum|x|)^2: the M2 about a
                mean that is off by e is M2 + cnt e^2 and the fp32 tile mean is within 2 u sum|x| of the true one; every
                d = x - mean, d d and the cnt additions round once.  A tile with one valid row: sum is the stored value bit for
                bit and M2 == 0.0.
  combined W    (S + 1) u sum |c| |w|: S products and S additions of which the first is exact.
  fp32 mode additionally keeps the figure of test_split_products_are_fp32_products: the rms relative error of every output
  block against fp64 is < 1e-6 (the elementwise bound is a worst case and cannot see a lost low part of the split).
No element of a listed row is left out of a comparison; there is no masking of small references.
"""
import functools
import importlib
from types import SimpleNamespace

import numpy as np
import torch

graph = importlib.import_module('3dinfomax_amd.graph')

U = 2.0 ** -24
POISON = 7.0
PAD = 8                                   # output row pitch ldc = N + PAD
RMS_FP32 = 1e-6
OFF_DIAGONAL = 1e3                        # the blocks of WD the batched products must not read
LEAKY = float(np.float32(0.01))

EDGES_COUNTS = {0: 5, 1: 1, 2: 63, 3: 64, 4: 65, 5: 128, 7: 129, 9: 2}


def _np64(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def bf16_round(t):
    """the operand as the bf16 matmul mode sees it (round to nearest even), fp64"""
    return _np64(torch.as_tensor(t).float().bfloat16())


def act64(x, act):
    if act in (None, 'none'):
        return x
    return np.where(x > 0, x, 0.0 if act == 'relu' else LEAKY * x)


# ---- degree layouts ------------------------------------------------------------------------------------------------------------
def layout(name):
    """in-degree of every node of a named layout, int64 [n]"""
    if name == 'edges':      # groups of 1 and 2 rows, of exactly one tile, tiles with 1 and with 63 valid rows, nodes in no group
        indeg = np.concatenate([np.full(c, d, dtype=np.int64) for d, c in EDGES_COUNTS.items()])
        return np.random.default_rng(11).permutation(indeg)
    if name == 'one_group':
        return np.full(70, 3, dtype=np.int64)
    if name == 'max_groups':      # 32 groups: the limit of Coef / I3dGroupedFcArgs
        indeg = np.concatenate([np.full(1 + d % 3, d, dtype=np.int64) for d in range(1, 33)])
        return np.random.default_rng(12).permutation(indeg)
    if name == 'long':            # the weight-gradient segment table only
        return np.random.default_rng(13).permutation(np.repeat(np.array([2, 5], dtype=np.int64), 3100))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def grouping(name, include_zero):
    """rows [m_padded] int32 (-1 = padding), tiles [m_padded / 64] int32, groups ((D, start, count), ...), listed [n] bool,
    group_of [n] (-1: in no group)"""
    indeg = layout(name)
    rows, tiles, groups = graph.group_nodes_by_degree(indeg, include_zero=include_zero)
    n = indeg.shape[0]
    group_of = np.full(n, -1, dtype=np.int64)
    for gi, (_, start, count) in enumerate(groups):
        group_of[rows[start:start + count]] = gi
    return SimpleNamespace(name=name, include_zero=include_zero, indeg=indeg, n=n, rows=rows, tiles=tiles, groups=groups,
                           n_groups=len(groups), m_padded=rows.shape[0], listed=group_of >= 0, group_of=group_of)


def last_tile_rows(gr, gi):
    """node ids in the last 64-row tile of group gi"""
    _, start, count = gr.groups[gi]
    first = start + (count - 1) // 64 * 64
    return gr.rows[first:start + count]


# ---- the case matrix -----------------------------------------------------------------------------------------------------------
BIG_SHAPES = [(800, 200), (800, 256), (200, 800)]                   # (K, N): Cfg11, Cfg9, the data-gradient shape
SMALL_SHAPES = [(8, 8), (20, 36), (48, 64), (80, 20), (18, 7)]      # K < K-tile; K tail 4, ragged N; < 4 K-tiles; tower K; unaligned
SMALL_LAYOUTS = ('edges', 'one_group', 'max_groups')
PRODUCT_CASES = [('edges', K, N) for K, N in BIG_SHAPES] + [(l, K, N) for l in SMALL_LAYOUTS for K, N in SMALL_SHAPES]
BF16_CASES = [('edges', K, N) for K, N in [(8, 8), (40, 36), (800, 200)]]
FUSED_CASES = [('edges', K, N) for K, N in [(800, 200), (800, 256), (20, 36)]] + [(l, 20, 36) for l in ('one_group', 'max_groups')]
FUSED_FORMS = ('inplace', 'separate', 'wide')
FUSED_ACTS = (None, 'relu', 'leakyrelu')
FUSED_EDGE_WIDTH = 10                     # Fo of the edge block in the merged product: c_in = PL + 2 Fo, ldcin = 2 Fo + Fp
TOWERS = [(3, 8, 16), (5, 20, 80)]        # (T, Fo, nA Ft)
WGRAD_CASES = [('edges', 200, 800), ('edges', 36, 20), ('max_groups', 16, 16), ('long', 16, 16)]      # (layout, M, N)
WGRAD_CFGS = (-1, 2, 3, 4)
WGRAD_SEG_ROWS = {'edges': (0, 64), 'max_groups': (0, 64), 'long': (0, 64, 96)}
# (on `long` 64 needs 98 segments > MAX_SEGS: the doubling loop, then 50 slices; 96 gives 66 slices >= 4 ZL: the small slab reduction)
COMBINE_CASES = [(S, G) for S in (1, 2, 3, 4) for G in (1, 32)]


@functools.lru_cache(maxsize=None)
def product_inputs(name, include_zero, K, N, trans_b):
    """A [n, K], B [G, N, K] (trans_b) or [G, K, N], the addend c0 [n, N]; the D = 0 group has a zero weight; the last K element of
    every row of A is at least 0.5 in size (a dropped K-tail then shows in every row, not only in most).  Not to be modified."""
    gr = grouping(name, include_zero)
    A = _randn(gr.n, K, seed=100 + K)
    A[:, -1] += torch.where(A[:, -1] >= 0, 0.5, -0.5)
    B = _randn(gr.n_groups, *((N, K) if trans_b else (K, N)), seed=200 + N + trans_b) * K ** -0.5
    if gr.groups[0][0] == 0:
        B[0] = 0
    c0 = _randn(gr.n, N, seed=300 + N)
    return SimpleNamespace(gr=gr, K=K, N=N, trans_b=trans_b, A=A.contiguous(), B=B.contiguous(), c0=c0.contiguous())


def ref_grouped(A, B, gr, trans_b, c_in=None, act=None, bf16=False):
    """(ref, mag) [n, N] float64; rows in no group are 0 in both (they are compared with the poison, not with these)"""
    a = bf16_round(A) if bf16 else _np64(A)
    b = bf16_round(B) if bf16 else _np64(B)
    N = b.shape[1] if trans_b else b.shape[2]
    ref, mag = np.zeros((gr.n, N)), np.zeros((gr.n, N))
    for gi, (_, start, count) in enumerate(gr.groups):
        r = gr.rows[start:start + count]
        w = b[gi].T if trans_b else b[gi]
        ref[r], mag[r] = a[r] @ w, np.abs(a[r]) @ np.abs(w)
    if c_in is not None:
        c = _np64(c_in)
        ref[gr.listed] += c[gr.listed]
        mag[gr.listed] += np.abs(c[gr.listed])
    return act64(ref, act), mag


@functools.lru_cache(maxsize=None)
def product_reference(name, include_zero, K, N, trans_b, accumulate, bf16=False, act=None):
    inp = product_inputs(name, include_zero, K, N, trans_b)
    return ref_grouped(inp.A, inp.B, inp.gr, trans_b, inp.c0 if accumulate else None, act, bf16)


@functools.lru_cache(maxsize=None)
def tower_inputs(name, include_zero, T, Fo, KA):
    """agg [n, T KA], gl [n, T Fo], WD [G, T Fo, T KA] with 1e3 in every block off the diagonal, lin0 [n, T Fo]"""
    gr = grouping(name, include_zero)
    AW, Mq = T * KA, T * Fo
    WD = torch.full((gr.n_groups, Mq, AW), OFF_DIAGONAL)
    blocks = _randn(gr.n_groups, T, Fo, KA, seed=400 + T) * KA ** -0.5
    for t in range(T):
        WD[:, t * Fo:(t + 1) * Fo, t * KA:(t + 1) * KA] = blocks[:, t]
    return SimpleNamespace(gr=gr, T=T, Fo=Fo, KA=KA, AW=AW, Mq=Mq, agg=_randn(gr.n, AW, seed=401).contiguous(),
                           gl=_randn(gr.n, Mq, seed=402).contiguous(), WD=WD.contiguous(), lin0=_randn(gr.n, Mq, seed=403).contiguous())


def ref_batched(inp, trans_b, c_in=None):
    """trans_b = 1: lin[r, t Fo ..] = c_in + agg[r, t KA ..] WD_g[t Fo .., t KA ..]^T  (K = KA);
    trans_b = 0: g_agg[r, t KA ..] = gl[r, t Fo ..] WD_g[t Fo .., t KA ..]  (K = Fo)    -> (ref, mag)"""
    gr, T, Fo, KA = inp.gr, inp.T, inp.Fo, inp.KA
    A, WD = _np64(inp.agg if trans_b else inp.gl), _np64(inp.WD)
    width = inp.Mq if trans_b else inp.AW
    ref, mag = np.zeros((gr.n, width)), np.zeros((gr.n, width))
    for gi, (_, start, count) in enumerate(gr.groups):
        r = gr.rows[start:start + count]
        for t in range(T):
            w = WD[gi, t * Fo:(t + 1) * Fo, t * KA:(t + 1) * KA]
            if trans_b:
                a, w, cols = A[r, t * KA:(t + 1) * KA], w.T, slice(t * Fo, (t + 1) * Fo)
            else:
                a, cols = A[r, t * Fo:(t + 1) * Fo], slice(t * KA, (t + 1) * KA)
            ref[r, cols], mag[r, cols] = a @ w, np.abs(a) @ np.abs(w)
    if c_in is not None:
        c = _np64(c_in)
        ref[gr.listed] += c[gr.listed]
        mag[gr.listed] += np.abs(c[gr.listed])
    return ref, mag


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name, M, N):
    """dY [n, M], a [n, N], the known matrix c0 [G, M, N] of the accumulate runs; groups with the D = 0 nodes included"""
    gr = grouping(name, True)
    return SimpleNamespace(gr=gr, M=M, N=N, dY=_randn(gr.n, M, seed=500 + M).contiguous(), a=_randn(gr.n, N, seed=600 + N).contiguous(),
                           c0=_randn(gr.n_groups, M, N, seed=700 + M).contiguous())


def ref_wgrad(A, B, rows, c0=None, bf16=False):
    """(ref, mag) [M, N] of A[rows]^T B[rows] (+ c0); the reduction length of the bound is len(rows)"""
    a = (bf16_round(A) if bf16 else _np64(A))[rows]
    b = (bf16_round(B) if bf16 else _np64(B))[rows]
    ref, mag = a.T @ b, np.abs(a).T @ np.abs(b)
    if c0 is not None:
        ref, mag = ref + _np64(c0), mag + np.abs(_np64(c0))
    return ref, mag


@functools.lru_cache(maxsize=None)
def wgrad_reference(name, M, N, accumulate, bf16=False):
    """[(ref, mag, count) per group]"""
    inp = wgrad_inputs(name, M, N)
    return [ref_wgrad(inp.dY, inp.a, inp.gr.rows[start:start + count], inp.c0[gi] if accumulate else None, bf16) + (count,)
            for gi, (_, start, count) in enumerate(inp.gr.groups)]


@functools.lru_cache(maxsize=None)
def combine_inputs(S, G):
    """W [f_out, S A] (the scaler blocks), coef [G, S] as log-degree scalers, dWD [G, f_out, A]"""
    f_out, A = 12, 20
    coef = np.array([[1.0, np.log(d + 2), 1 / np.log(d + 2), -0.5 * d][:S] for d in range(G)], dtype=np.float32)
    return SimpleNamespace(S=S, G=G, f_out=f_out, A=A, W=_randn(f_out, S * A, seed=800 + S).contiguous(), coef=coef,
                           dWD=_randn(G, f_out, A, seed=900 + G).contiguous())


def ref_combine_fwd(W, coef, A):
    """WD[g] = sum_s coef[g][s] W[:, s A : (s + 1) A] -> (ref, mag) [G, f_out, A]"""
    w, c = _np64(W), _np64(coef)
    blocks = np.stack([w[:, s * A:(s + 1) * A] for s in range(c.shape[1])])                     # [S, f_out, A]
    return np.einsum('gs,sna->gna', c, blocks), np.einsum('gs,sna->gna', np.abs(c), np.abs(blocks))


def ref_combine_bwd(dWD, coef):
    """dW[:, s A : (s + 1) A] = sum_g coef[g][s] dWD[g] -> (ref, mag) [f_out, S A]"""
    d, c = _np64(dWD), _np64(coef)
    f_out = d.shape[1]
    ref = np.einsum('gs,gna->nsa', c, d).reshape(f_out, -1)
    return ref, np.einsum('gs,gna->nsa', np.abs(c), np.abs(d)).reshape(f_out, -1)


# ---- checks ----------------------------------------------------------------------------------------------------------------------
def worst(out, ref, bound):
    """(max |out - ref| / bound, its index); inf where an element with bound 0 is not exact or the output is not finite"""
    err = np.abs(_np64(out) - ref)
    ok = bound > 0
    ratio = np.where(ok, err / np.where(ok, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(err), ratio, np.inf)
    if ratio.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i]), tuple(int(v) for v in i)


def check(out, ref, mag, K):
    """worst err / ((K + 6) u mag) and the offending index"""
    return worst(out, ref, (K + 6) * U * mag)


def flagged_rows(out, ref, mag, K):
    """bool per row: at least one element outside the product bound"""
    err = np.abs(_np64(out) - ref)
    return (err > (K + 6) * U * mag).any(1)


def rms_rel(out, ref):
    den = np.sqrt(np.mean(ref ** 2)) if ref.size else 0.0
    num = np.sqrt(np.mean((_np64(out) - ref) ** 2)) if ref.size else 0.0
    return float(num / den) if den > 0 else (0.0 if num == 0 else np.inf)


def verdict(C, ref, mag, gr, K, before=None):
    """Everything a grouped product's output [n, N + PAD] is held to.  before: the buffer's content when the launch accumulates
    onto it (rows in no group must be bit-unchanged); None: it was all poison (they must still hold it).
    -> ratio, index (row, column), rms over the listed rows, pad_ok, unlisted_ok"""
    C = C.detach().cpu() if isinstance(C, torch.Tensor) else torch.as_tensor(C)
    N = ref.shape[1]
    out = C[:, :N].numpy()
    listed = gr.listed
    ratio, idx = check(out[listed], ref[listed], mag[listed], K)
    if idx:
        idx = (int(np.nonzero(listed)[0][idx[0]]), idx[1])
    if before is None:
        unlisted_ok = bool(np.all(out[~listed] == np.float32(POISON)))
    else:
        b = (before.detach().cpu() if isinstance(before, torch.Tensor) else torch.as_tensor(before))[:, :N].numpy()
        unlisted_ok = bool(np.array_equal(out[~listed].view(np.int32), b[~listed].view(np.int32)))
    return SimpleNamespace(ratio=ratio, index=idx, rms=rms_rel(out[listed], ref[listed]),
                           pad_ok=bool(torch.all(C[:, N:] == POISON)), unlisted_ok=unlisted_ok)


def tile_stats(stored, rows):
    """fp64 per-tile statistics of the stored values [n, N] for the 64-padded row list: sum, M2, count [T], sum|x| ([T, N])"""
    x_all = _np64(stored)
    T, N = rows.shape[0] // 64, x_all.shape[1]
    s, m2, ab, cnt = np.zeros((T, N)), np.zeros((T, N)), np.zeros((T, N)), np.zeros(T)
    for t in range(T):
        r = rows[t * 64:(t + 1) * 64]
        x = x_all[r[r >= 0]]
        cnt[t] = x.shape[0]
        if x.shape[0]:
            s[t], ab[t] = x.sum(0), np.abs(x).sum(0)
            m2[t] = ((x - x.mean(0)) ** 2).sum(0)
    return s, m2, cnt, ab


def stats_verdict(partial, stored, rows):
    """partial [T, 3, N] against the values that were stored -> sum_ratio, m2_ratio (with their (tile, column)), count_ok,
    single_ok (tiles with one valid row: sum bit-equal to the stored value, M2 == 0.0), n_single"""
    p = _np64(partial)
    st = _np64(stored)
    s, m2, cnt, ab = tile_stats(st, rows)
    c = cnt[:, None]
    sum_ratio, sum_idx = worst(p[:, 0], s, c * U * ab)
    m2_ratio, m2_idx = worst(p[:, 1], m2, (c + 4) * U * m2 + 4 * c * (U * ab) ** 2)
    count_ok = bool(np.all(p[:, 2] == c))
    single_ok, n_single = True, 0
    for t in np.nonzero(cnt == 1)[0]:
        r = rows[t * 64:(t + 1) * 64]
        x = st[r[r >= 0][0]]
        n_single += 1
        single_ok = single_ok and bool(np.array_equal(p[t, 0], x) and np.all(p[t, 1] == 0.0))
    return SimpleNamespace(sum_ratio=sum_ratio, sum_index=sum_idx, m2_ratio=m2_ratio, m2_index=m2_idx, count_ok=count_ok,
                           single_ok=single_ok, n_single=n_single)


def fused_addend(form, c0, N):
    """The addend's buffer in the three forms the product uses -> (buffer [n, pitch], column offset, ldcin).  The columns that do
    not belong to the addend hold 1e3: a read at the wrong pitch or offset breaks the bound."""
    n = c0.shape[0]
    if form == 'inplace':
        return None, 0, 0
    off, pitch = (0, N + 4) if form == 'separate' else (2 * FUSED_EDGE_WIDTH, 2 * FUSED_EDGE_WIDTH + N)
    buf = torch.full((n, pitch), OFF_DIAGONAL)
    buf[:, off:off + N] = c0
    return buf.contiguous(), off, pitch
