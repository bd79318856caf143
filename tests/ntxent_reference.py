"""fp64 reference of the NT-Xent loss (csrc/ntxent.hip) with a DERIVED per-element error bound, an fp32 emulation of the kernels'
evaluation order (both backward generations), and the one input set the bound tests share
(tests/test_ntxent_bounds_cpu.py, tests/test_gpu_ntxent.py).

numpy / torch on the CPU only; the HIP library is never loaded from here.

The operation (top of csrc/ntxent.hip; reference commons/losses.py:143-155, :225-247), for the local rows i of z1 and the
columns j of the gathered z2 (conformer-minor), a_i = |z1_i|, b_j = |z2_j|:
    nrm_ij = a_i b_j + eps,  s_ij = sim_ij / nrm_ij,  t_ij = s_ij / tau,  p_ij = exp(t_ij)
    rowsum_i = sum_j p_ij,  pos_i = sum of p_ij over the conf columns from (pos_offset + i) conf,  den_i = rowsum_i - pos_i
    l_i = -log(pos_i / den_i),  loss = loss_scale sum_i l_i
    gs = loss_scale * upstream,  H_ij = dL/dsim_ij = (j positive ? -gs / pos_i : gs / den_i) p_ij / (tau nrm_ij)
    ca_i = -(1 / a_i) sum_j H_ij s_ij b_j   (0 where a_i = 0),   cb_j = -(1 / b_j) sum_i H_ij s_ij a_i   (0 where b_j = 0)
    dz1 = H z2 + ca z1,  dz2 = H^T z1 + cb z2        (norm=False: a = b = 1, eps = 0, no ca / cb terms)
tau, eps are the floats the C ABI receives.  The reference forms den as the sum of the negatives (no cancellation in fp64).

The tolerance is no chosen number: it is the first-order rounding bound of an fp32 evaluation of these formulas with the sums in
ANY order (the (n-1) u form, not the depth of the kernels' trees: torch's own order has to fit under it too), per output element,
in fp64 from the inputs, u = 2^-24 with a slack of 1.01 on every u.  r_x is a relative error, e_x an absolute one:
    r_a, r_b   0 when the norms are given; from z: (dim/2 + 1) u   (dim squares and adds under a square root, the root's rounding)
    e_sim      0 when sim is given; from z: GEMM_U(dim) u (|z1| |z2|^T)_ij
    e_s  = |s| (3 u + r_a + r_b) + e_sim / nrm          (product, add of eps, quotient)
    e_t  = e_s / tau + 2 u |t|                          (the rounding of 1 / tau and the product with it)
    r_p  = expm1(e_t) + 2 K_EXP u                       (argument error amplified by |t| inside e_t; an ulp is at most 2 u)
    e_rowsum = sum_j p r_p + (n-1) u rowsum,   e_pos = sum_pos p r_p + (conf-1) u pos
    e_den = sum_neg p r_p + (n-1) u rowsum + (conf-1) u pos + u den
        the cancellation of rowsum - pos: the roundings of the two SUMS are amplified by rowsum / den.  The positives' own value
        errors are not: both sums add the same fp32 numbers p_ij (kernels: one register, the oracle: one tensor), so they drop
        out of the difference exactly.  (The first draft had e_rowsum + e_pos + u den, which counts them twice; from z the GEMM's
        part of them alone is larger than den on the aligned inputs, and the draft then bounds nothing.)
    r_q  = e_pos / pos + e_den / den + u,   e_l = -log1p(-r_q) + 2 K_LOG u |l|
    e_loss = loss_scale (sum e_l + (b1-1) u sum |l|) + 2 u |loss|
    r_H  = r_g + r_p + 6 u + r_a + r_b,   r_g = 3 u + e_den / (den - e_den)  resp.  3 u + e_pos / (pos - e_pos)
    ca:  terms T_j = H s b,  e_T = |H b| e_s + |T| (r_H + r_b + 2 u),
         e_ca = (sum e_T + (n-1) u sum |T|) / a + (u + r_a) sum |T| / a        (sizes of the terms, not of the result)
    cb:  the same over the rows, with a and b exchanged
    dz1: GEMM_U(ncol) u (|H| |z2|) + e_H |z2| + e_ca |z1| + u |ca z1| + u (|H| |z2| + |ca z1|);  dz2 likewise with K = b1
GEMM_U(K) = 6 K + 3, written (K + c) with c = 5 K + 3: in fp32 mode the library's GEMM forms a product from six exact bf16
part products (csrc/gemm.hip, split products) and drops three of at most 2^-24 |a b| each (the 3); each of the 6 K part
products is one fp32 accumulation of its own, in an order the MFMA unit chooses, so the any-order bound counts 6 K - 1 additions
of terms whose sizes sum to at most sum |a| |b| (1 + 2^-8)^2.  c is therefore no constant per product: it grows with K, because
the split form pays with accumulations, not with the accuracy of a product.  The native fp32 MFMA and a BLAS GEMM (K - 1
additions, K roundings of the products) are inside the same bound.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

U = 1.01 * 2.0 ** -24
# The two device constants (ulp of the result; measured once on the MI355X, rounded up to whole ulp): expf over
# [-20, 20] was off by at most 0.84 ulp, logf over [1e-4, 1e10] by at most 1.88 ulp.  Every other number of the bound is derived.
K_EXP = 1
K_LOG = 2
f32 = np.float32


def GEMM_U(K):
    return 6 * K + 3


def _np64(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def _np32(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().float().numpy()
    return np.asarray(t, dtype=np.float32)


def pos_mask(b1, ncol, conf, pos_offset, defect=None):
    i = np.arange(b1)[:, None]
    p0 = (pos_offset * conf + i) if defect == 'p0' else (pos_offset + i) * conf
    j = np.arange(ncol)[None, :]
    return (j >= p0) & (j < p0 + conf)


# ---- fp64 reference and bound -------------------------------------------------------------------------------------------------
def reference(sim, n1, n2, conf, pos_offset, tau, eps, loss_scale, upstream=1.0, z1=None, z2=None, norm=True,
              e_sim=None, r_a=0.0, r_b=0.0):
    """Values and bounds (float64 arrays; `x` and `e_x`) of every output of the row kernels from sim [b1, ncol], n1, n2 as given
    (e_sim, r_a, r_b: what these inputs themselves are off by), and with z1, z2 of dz1, dz2."""
    S, a, b = _np64(sim), _np64(n1)[:, None], _np64(n2)[None, :]
    b1, ncol = S.shape
    tau, eps = float(f32(tau)), float(f32(eps))
    e_sim = np.zeros_like(S) if e_sim is None else e_sim
    ra = np.where(a > 0, r_a, 0.0) + np.zeros_like(a)
    rb = np.where(b > 0, r_b, 0.0) + np.zeros_like(b)
    o = SimpleNamespace(b1=b1, ncol=ncol)
    nrm = a * b + eps
    s = S / nrm
    e_s = np.abs(s) * (3 * U + ra + rb) + e_sim / nrm
    t = s / tau
    e_t = e_s / tau + 2 * U * np.abs(t)
    p = np.exp(t)
    r_p = np.expm1(e_t) + 2 * K_EXP * U
    e_p = p * r_p
    m = pos_mask(b1, ncol, conf, pos_offset)
    o.mask = m
    o.row_sum, o.row_pos, o.den = p.sum(1), (p * m).sum(1), (p * ~m).sum(1)
    e_rs_sum = (ncol - 1) * U * o.row_sum
    e_ps_sum = (conf - 1) * U * o.row_pos
    o.e_row_sum = e_p.sum(1) + e_rs_sum
    o.e_row_pos = (e_p * m).sum(1) + e_ps_sum
    o.e_den = (e_p * ~m).sum(1) + e_rs_sum + e_ps_sum + U * o.den
    o.r_q = o.e_row_pos / o.row_pos + o.e_den / o.den + U
    o.row_loss = np.log(o.den) - np.log(o.row_pos)
    with np.errstate(invalid='ignore', divide='ignore'):
        o.e_row_loss = -np.log1p(-o.r_q) + 2 * K_LOG * U * np.abs(o.row_loss)
    o.loss = loss_scale * o.row_loss.sum()
    o.e_loss = abs(loss_scale) * (o.e_row_loss.sum() + (b1 - 1) * U * np.abs(o.row_loss).sum()) + 2 * U * abs(o.loss)
    o.sum_abs_row_loss = abs(loss_scale) * np.abs(o.row_loss).sum()
    # backward
    gs = loss_scale * upstream
    with np.errstate(invalid='ignore', divide='ignore'):
        r_gn = (3 * U + o.e_den / (o.den - o.e_den))[:, None]
        r_gp = (3 * U + o.e_row_pos / (o.row_pos - o.e_row_pos))[:, None]
    g = np.where(m, (-gs / o.row_pos)[:, None], (gs / o.den)[:, None])
    H = g * p / tau / nrm
    r_H = np.where(m, r_gp, r_gn) + r_p + 6 * U + ra + rb
    o.dsim, o.e_dsim = H, np.abs(H) * r_H
    T = H * s * b
    e_T = np.abs(H * b) * e_s + np.abs(T) * (r_H + rb + 2 * U)
    sT = np.abs(T).sum(1)
    a1, ra1 = a[:, 0], ra[:, 0]
    an = np.where(a1 > 0, a1, 1.0)
    o.ca = np.where(a1 > 0, -T.sum(1) / an, 0.0)
    o.e_ca = np.where(a1 > 0, (e_T.sum(1) + (ncol - 1) * U * sT) / an + (U + ra1) * sT / an, 0.0)
    o.ca_abs = np.where(a1 > 0, sT / an, 0.0)
    Tc = H * s * a
    e_Tc = np.abs(H * a) * e_s + np.abs(Tc) * (r_H + ra + 2 * U)
    sTc = np.abs(Tc).sum(0)
    b0, rb0 = b[0], rb[0]
    bn = np.where(b0 > 0, b0, 1.0)
    o.cb = np.where(b0 > 0, -Tc.sum(0) / bn, 0.0)
    o.e_cb = np.where(b0 > 0, (e_Tc.sum(0) + (b1 - 1) * U * sTc) / bn + (U + rb0) * sTc / bn, 0.0)
    o.cb_abs = np.where(b0 > 0, sTc / bn, 0.0)
    if z1 is not None:
        Z1, Z2 = _np64(z1), _np64(z2)
        ca, e_ca, ca_abs = (o.ca, o.e_ca, o.ca_abs) if norm else (0 * o.ca, 0 * o.ca, 0 * o.ca)
        cb, e_cb, cb_abs = (o.cb, o.e_cb, o.cb_abs) if norm else (0 * o.cb, 0 * o.cb, 0 * o.cb)
        M1, M2 = np.abs(H) @ np.abs(Z2), np.abs(H).T @ np.abs(Z1)
        o.dz1 = H @ Z2 + ca[:, None] * Z1
        o.dz2 = H.T @ Z1 + cb[:, None] * Z2
        c1, c2 = np.abs(ca[:, None] * Z1), np.abs(cb[:, None] * Z2)
        o.e_dz1 = GEMM_U(ncol) * U * M1 + o.e_dsim @ np.abs(Z2) + e_ca[:, None] * np.abs(Z1) + U * c1 + U * (M1 + c1)
        o.e_dz2 = GEMM_U(b1) * U * M2 + o.e_dsim.T @ np.abs(Z1) + e_cb[:, None] * np.abs(Z2) + U * c2 + U * (M2 + c2)
        # sizes of the terms of an element: what further fp32 additions (shards summed by autograd) are accurate to
        o.m_dz1 = M1 + ca_abs[:, None] * np.abs(Z1)
        o.m_dz2 = M2 + cb_abs[:, None] * np.abs(Z2)
    return o


def reference_from_z(z1, z2, conf, pos_offset, tau, eps, loss_scale, upstream=1.0, norm=True):
    """The same from the embeddings: z1 [b1, dim] the local rows, z2 [b2 conf, dim]; norms and similarities in fp64, with what an
    fp32 evaluation of them is off by carried through the exponential"""
    Z1, Z2 = _np64(z1), _np64(z2)
    dim = Z1.shape[1]
    sim = Z1 @ Z2.T
    e_sim = GEMM_U(dim) * U * (np.abs(Z1) @ np.abs(Z2).T)
    if norm:
        n1, n2 = np.sqrt((Z1 * Z1).sum(1)), np.sqrt((Z2 * Z2).sum(1))
        r_n = (dim / 2 + 1) * U
    else:
        n1, n2, r_n, eps = np.ones(Z1.shape[0]), np.ones(Z2.shape[0]), 0.0, 0.0
    o = reference(sim, n1, n2, conf, pos_offset, tau, eps, loss_scale, upstream, z1=z1, z2=z2, norm=norm, e_sim=e_sim,
                  r_a=r_n, r_b=r_n)
    o.sim, o.e_sim = sim, e_sim
    o.n1, o.n2, o.e_n1, o.e_n2 = n1, n2, n1 * r_n, n2 * r_n
    return o


def worst(out, ref, bound):
    """(max over the elements of |out - ref| / bound, flat index of that element); inf where an element with bound 0 is not exact,
    or is not finite"""
    out = _np64(out).reshape(np.shape(ref))
    ref, bound = np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.abs(out - ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(err) & np.isfinite(bound), ratio, np.inf)
    if ratio.size == 0:
        return 0.0, 0
    k = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[k]), k


def check(name, out, ref, bound):
    """print the worst error / bound ratio of one quantity, the element where it occurs and the largest absolute error, then
    assert the ratio"""
    r, k = worst(out, ref, bound)
    at = np.unravel_index(k, np.shape(ref)) if np.ndim(ref) else ()
    err = np.abs(_np64(out).reshape(-1) - np.asarray(ref, dtype=np.float64).reshape(-1))
    print(f'  {name}: worst error/bound {r:.3f} at {tuple(int(x) for x in at)} (max abs err {float(err.max()):.3e})')
    assert r <= 1.0, f'{name}: error / bound = {r} at {at}'
    return r


# ---- fp32 emulation of the kernels' evaluation order --------------------------------------------------------------------------
DEFECTS = ('drop_last', 'p0', 'ca_tail', 'col256', 'cb_sign', 'gpos_den')


def _stride_sum(x, lanes):
    """per-lane partial sums of `for (j = lane; j < n; j += lanes) acc += x[j]`, [..., n] -> [..., lanes]"""
    n = x.shape[-1]
    trips = -(-n // lanes)
    pad = np.zeros(x.shape[:-1] + (trips * lanes,), dtype=f32)
    pad[..., :n] = x
    pad = pad.reshape(x.shape[:-1] + (trips, lanes))
    acc = np.zeros(x.shape[:-1] + (lanes,), dtype=f32)
    for k in range(trips):
        acc = acc + pad[..., k, :]
    return acc


def _wave_tree(v):
    """lane 0 after `for (o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64)`, [..., 64] -> [...]"""
    v = v.astype(f32).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _block_sum(v):
    """block_sum of 256 threads: four wave trees, then sm[0] + sm[1] + sm[2] + sm[3]"""
    w = _wave_tree(v.reshape(v.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _seq_sum(v):
    acc = np.zeros(v.shape[:-1], dtype=f32)
    for k in range(v.shape[-1]):
        acc = acc + v[..., k]
    return acc


def emulate_norms(z, generation):
    """row_norms_pair_kernel ('fused': one wave per row, float4 lanes when dim % 4 == 0) / row_norms_kernel ('sequenced')"""
    z = _np32(z)
    rows, dim = z.shape
    if generation == 'sequenced':
        return np.sqrt(_block_sum(_stride_sum(z * z, 256)))
    if dim % 4 == 0:
        trips = -(-dim // 256)
        pad = np.zeros((rows, trips * 256), dtype=f32)
        pad[:, :dim] = z
        v = pad.reshape(rows, trips, 64, 4)
        q = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]) + v[..., 3] * v[..., 3]
        acc = np.zeros((rows, 64), dtype=f32)
        for k in range(trips):
            acc = acc + q[:, k]
    else:
        acc = _stride_sum(z * z, 64)
    return np.sqrt(_wave_tree(acc))


def emulate(z1, z2, conf, pos_offset, tau, eps, loss_scale, upstream=1.0, generation='fused', norm=True, defect=None,
            given=None):
    """fp32 evaluation in the kernels' order.  generation 'fused': i3d_ntxent_loss_fwd / _bwd (row_norms_pair_kernel,
    ntxent_bwd_fused_kernel with H recomputed in the column workgroups, the GEMMs accumulating on ca z1 / cb z2); 'sequenced':
    row_norms_kernel, ntxent_bwd_row_kernel, ntxent_bwd_col_kernel, row_axpy.  given = (sim, n1, n2): the row kernels alone on
    these inputs.  The similarity and gradient GEMMs are fp32 matrix products in numpy's order."""
    with np.errstate(all='ignore'):
        return _emulate(z1, z2, conf, pos_offset, tau, eps, loss_scale, upstream, generation, norm, defect, given)


def _emulate(z1, z2, conf, pos_offset, tau, eps, loss_scale, upstream, generation, norm, defect, given):
    o = SimpleNamespace()
    if given is not None:
        sim, n1, n2 = (_np32(x) for x in given)
    else:
        z1, z2 = _np32(z1), _np32(z2)
        if norm:
            n1, n2 = emulate_norms(z1, generation), emulate_norms(z2, generation)
        else:
            n1, n2, eps = np.ones(z1.shape[0], dtype=f32), np.ones(z2.shape[0], dtype=f32), 0.0
        sim = z1 @ z2.T
    b1, ncol = sim.shape
    o.sim, o.n1, o.n2 = sim, n1, n2
    inv_tau, eps = f32(1) / f32(tau), f32(eps)
    a, b = n1[:, None], n2[None, :]
    nrm = a * b + eps
    s = sim / nrm
    p = np.exp(s * inv_tau)
    m = pos_mask(b1, ncol, conf, pos_offset, defect)
    prs = p.copy()
    if defect == 'drop_last':
        prs[:, -1] = 0
    o.row_sum = _block_sum(_stride_sum(prs, 256))
    o.row_pos = _block_sum(_stride_sum(np.where(m, p, f32(0)), 256))
    o.row_loss = -np.log(o.row_pos / (o.row_sum - o.row_pos))
    o.loss = _block_sum(_stride_sum(o.row_loss, 256)) * f32(loss_scale)
    # backward
    gs = f32(loss_scale) * f32(upstream)
    pos, den = o.row_pos, o.row_sum - o.row_pos
    g_neg, g_pos = gs / den, (-gs / den if defect == 'gpos_den' else -gs / pos)
    G = np.where(m, g_pos[:, None], g_neg[:, None]) * p * inv_tau
    H = G / nrm
    o.dsim = H
    da = _block_sum(_stride_sum(-(H * s * b), 256))
    o.ca = np.where(n1 > 0, da / np.where(n1 > 0, n1, f32(1)), f32(0)).astype(f32)
    x = -(H * s * a)
    if generation == 'fused':              # 32 row lanes, rows ry, ry + 32, ...: the FC_U groups of a trip keep that order
        if defect == 'col256':
            x = x[:256]
        t = _seq_sum(_stride_sum(np.ascontiguousarray(x.T), 32))
    else:                                  # 16 row lanes over the stored dsim
        t = _seq_sum(_stride_sum(np.ascontiguousarray(x.T), 16))
    o.cb = np.where(n2 > 0, t / np.where(n2 > 0, n2, f32(1)), f32(0)).astype(f32)
    if defect == 'cb_sign':
        o.cb = -o.cb
    if given is not None:
        return o
    if generation == 'fused' and norm:
        d1 = o.ca[:, None] * z1
        if defect == 'ca_tail':
            d1[:, 256:] = 0
        o.dz1 = d1 + H @ z2
        o.dz2 = o.cb[:, None] * z2 + H.T @ z1
    else:
        o.dz1, o.dz2 = H @ z2, H.T @ z1
        if norm:
            o.dz1 = o.dz1 + o.ca[:, None] * z1
            o.dz2 = o.dz2 + o.cb[:, None] * z2
    return o


# ---- the shared inputs ----------------------------------------------------------------------------------------------------------
def _case(id, b1, b2, conf, dim, pos_offset, tau=0.1, shards=None):
    return SimpleNamespace(id=id, b1=b1, b2=b2, conf=conf, dim=dim, pos_offset=pos_offset, tau=tau, shards=shards)


CASES = [
    _case('min', 2, 2, 1, 7, 0),
    _case('c3wide', 9, 9, 3, 516, 0),
    _case('tail1', 65, 65, 1, 300, 0),
    _case('stride', 257, 257, 1, 64, 0),
    _case('posacross', 86, 86, 3, 36, 0),
    _case('shard_last', 16, 67, 1, 40, 51, shards=(17, 17, 17, 16)),      # the last shard of a plan that keeps the remainder
    _case('shard_c3', 5, 21, 3, 20, 16, shards=(6, 5, 5, 5)),
    _case('tau0.05', 33, 33, 1, 64, 0, tau=0.05),
    _case('tau0.5', 33, 33, 1, 64, 0, tau=0.5),
]
CASE_BY_ID = {c.id: c for c in CASES}
UNNORMALISED_ON = ('min', 'tail1', 'shard_c3')


def kinds_of(case):
    """The input kinds that are defined for a case.  zero_rows needs the epsilon of the single-positive loss (0 / 0 without
    it, in the reference too).  aligned at tau 0.05 is no fp32 problem: the positive's term is e^20 = 5e8, an ulp of rowsum is
    32, and the 32 negatives sum to a few hundred - rowsum - pos has no correct digit in ANY fp32 evaluation, the reference's
    included (den <= e_den there; the condition is asserted on every kind that is kept)."""
    k = ['random']
    if case.tau >= 0.1:
        k.append('aligned')
    k.append('collapsed')
    if case.conf == 1:
        k.append('zero_rows')
    if case.id in UNNORMALISED_ON:
        k.append('unnormalised')
    return k


COMBOS = [(c.id, k) for c in CASES for k in kinds_of(c)]
COMBO_IDS = [f'{c}-{k}' for c, k in COMBOS]


def make_embeddings(case, kind):
    """(z1 [b2, dim]: the whole batch, z2 [b2 conf, dim]) float32"""
    gen = torch.Generator().manual_seed(7000 + 13 * CASES.index(case) + len(kind))
    B, C, D = case.b2, case.conf, case.dim

    def randn(*shape):
        return torch.randn(*shape, generator=gen)

    if kind == 'collapsed':
        common = randn(D)
        z1, z2 = common + 0.05 * randn(B, D), common + 0.05 * randn(B * C, D)
    elif kind == 'aligned':
        z1 = randn(B, D)
        factor = 1.0 + 0.2 * torch.rand(B * C, 1, generator=gen)
        z2 = factor * z1.repeat_interleave(C, 0) + 0.03 * randn(B * C, D)
    else:
        z1, z2 = randn(B, D), randn(B * C, D)
    if kind == 'zero_rows':
        z1[case.pos_offset + case.b1 // 2] = 0.0           # a local row of z1 ...
        z2[case.pos_offset * C] = 0.0                      # ... and the positive column of another local row
    if kind == 'unnormalised':
        z1, z2 = z1 * 0.15, z2 * 0.15
    return z1.float().contiguous(), z2.float().contiguous()


def zero_rows_of(case):
    """(local row of z1, row of z2) that the zero_rows kind clears"""
    return case.b1 // 2, case.pos_offset * case.conf


@functools.lru_cache(maxsize=None)
def inputs(case_id, kind, upstream=1.0):
    """Everything a (case, kind) needs, built once; nothing in it may be modified.
    z1 (the local rows), z2, z1_full; tau, eps, norm, loss_scale = 1 / b2; given = (sim, n1, n2): an fp32 similarity matrix and
    fp32 norms made on the CPU, the inputs of the row kernels alone; ref_rows: the reference from `given`; ref: from z1, z2;
    full: the reference of the whole batch from z1_full, z2 (the shard cases; otherwise `ref` itself)."""
    case = CASE_BY_ID[case_id]
    z1_full, z2 = make_embeddings(case, kind)
    norm = kind != 'unnormalised'
    tau = case.tau if norm else 0.5
    eps = (1e-8 if case.conf == 1 else 0.0) if norm else 0.0
    scale = 1.0 / case.b2
    z1 = z1_full[case.pos_offset:case.pos_offset + case.b1].contiguous()
    I = SimpleNamespace(case=case, kind=kind, z1=z1, z2=z2, z1_full=z1_full, tau=tau, eps=eps, norm=norm, loss_scale=scale,
                        upstream=upstream, b1=case.b1, b2=case.b2, conf=case.conf, dim=case.dim, pos_offset=case.pos_offset,
                        ncol=case.b2 * case.conf)
    if norm:
        n1 = torch.from_numpy(np.sqrt((_np64(z1) ** 2).sum(1)).astype(f32))
        n2 = torch.from_numpy(np.sqrt((_np64(z2) ** 2).sum(1)).astype(f32))
    else:
        n1, n2 = torch.ones(case.b1), torch.ones(I.ncol)
    I.given = ((z1 @ z2.T).contiguous(), n1, n2)
    I.ref_rows = reference(*I.given, case.conf, case.pos_offset, tau, eps, scale, upstream)
    I.ref = reference_from_z(z1, z2, case.conf, case.pos_offset, tau, eps, scale, upstream, norm)
    I.full = I.ref if case.shards is None else reference_from_z(z1_full, z2, case.conf, 0, tau, eps, scale, upstream, norm)
    return I


def input_conditions(I):
    """The conditions on the inputs under which no element is ambiguous (asserted by both test files): the difference
    rowsum - pos keeps correct digits in every row, both in the row kernels' reference and from the embeddings; every bound is
    finite; the positives of the aligned kind have cosines of 0.99 or more; and no output is exactly zero except the norm-path
    coefficients of the cleared rows of zero_rows."""
    for r in (I.ref_rows, I.ref, I.full):
        assert np.all(r.den > r.e_den) and np.all(r.row_pos > r.e_row_pos) and np.all(r.r_q < 1), 'a row has den <= e_den'
        for name in ('e_row_sum', 'e_row_pos', 'e_row_loss', 'e_dsim', 'e_ca', 'e_cb'):
            assert np.all(np.isfinite(getattr(r, name))), name
        assert np.all(r.dsim != 0)
    assert np.all(np.isfinite(I.ref.e_dz1)) and np.all(np.isfinite(I.ref.e_dz2))
    z1r, z2r = zero_rows_of(I.case)
    ca0, cb0 = I.ref.ca == 0, I.ref.cb == 0
    if I.kind == 'zero_rows':
        assert ca0.sum() == 1 and ca0[z1r] and cb0.sum() == 1 and cb0[z2r]
        assert I.ref.e_ca[z1r] == 0 and I.ref.e_cb[z2r] == 0
    else:
        assert not ca0.any() and not cb0.any()
    if I.kind == 'aligned':
        s = I.ref.sim / (I.ref.n1[:, None] * I.ref.n2[None, :])
        assert s[I.ref.mask].min() >= 0.99
