"""The derived bounds of tests/grouped_reference.py are neither too tight nor too loose (no GPU, no HIP library):

* an fp32 emulation of every case tests/test_gpu_grouped.py runs stays inside them - torch's CPU fp32 product, the same product
  formed from operands pre-split into three bf16 parts with the three dropped part products removed (csrc/gemm.hip:456-464), the
  bf16 mode's product of rounded operands, and the statistics in the kernel's own order (gemm.hip:611-648: four 16-row quarters
  summed sequentially, then ((a + b) + c) + d),
* and each defect a rewrite of these kernels can have, injected into the emulation, is flagged on every case where it can occur.
The emulated buffers go through the same verdict functions as the GPU outputs.
"""
import numpy as np
import pytest
import torch

import grouped_reference as R

f32 = np.float32
IDS = lambda c: '-'.join(str(v) for v in c)      # noqa: E731


# ---- the emulation ---------------------------------------------------------------------------------------------------------------
def split3(x):
    """x = hi + mid + lo exactly, every part the RNE bf16 of what the parts in front of it leave (gemm.hip: split_pair)"""
    hi = x.bfloat16().float()
    r1 = x - hi
    mid = r1.bfloat16().float()
    lo = (r1 - mid).bfloat16().float()
    return hi, mid, lo


def product32(a, w, mode, drop_low=False):
    """a [m, K] w [K, N] in fp32: 'fp32' torch's own order; 'split' the six part products of order <= 2, small ones first, each
    exact in fp32; 'bf16' the product of the rounded operands"""
    if mode == 'fp32':
        return a @ w
    if mode == 'bf16':
        return a.bfloat16().float() @ w.bfloat16().float()
    ah, am, al = split3(a)
    bh, bm, bl = split3(w)
    terms = [(ah, bl), (al, bh), (am, bm), (ah, bm), (am, bh), (ah, bh)]
    if drop_low:
        terms = terms[2:]
    acc = torch.zeros(a.shape[0], w.shape[1])
    for x, y in terms:
        acc = acc + x @ y
    return acc


def act32(x, act):
    if act is None:
        return x
    return torch.where(x > 0, x, torch.zeros_like(x) if act == 'relu' else x * float(f32(0.01)))


def emulate_grouped(inp, accumulate, mode, act=None, addend=None, defect=None):
    """the buffer [n, N + PAD] a grouped launch leaves.  addend: None (in place: the buffer's own content when accumulating) or
    (buffer, column offset, pitch) of fused_addend() -> (C, before)"""
    gr, K, N = inp.gr, inp.K, inp.N
    C = torch.full((gr.n, N + R.PAD), R.POISON)
    if accumulate and addend is None:
        C[:, :N] = inp.c0
    before = C.clone() if (accumulate and addend is None) else None
    A = inp.A
    kk = K - 1 if defect == 'drop_k' else K

    def c_in(rows):
        if not accumulate:
            return 0.0
        if addend is None:
            return inp.c0[rows]
        buf, off, pitch = addend
        if defect == 'cin_pitch':
            flat = buf.flatten()
            return flat[(off + torch.as_tensor(rows, dtype=torch.long)[:, None] * N + torch.arange(N)[None, :])]
        return buf[rows, off:off + N]

    for gi, (_, start, count) in enumerate(gr.groups):
        for t0 in range(start, start + count, 64):
            r = gr.rows[t0:min(t0 + 64, start + count)].astype(np.int64)
            wi = gi
            if defect == 'next_weight' and t0 + 64 >= start + count and gi + 1 < gr.n_groups:
                wi = gi + 1
            w = inp.B[wi].T if inp.trans_b else inp.B[wi]
            C[r, :N] = act32(product32(A[r, :kk], w[:kk], mode, defect == 'drop_low') + c_in(r), act)
    if defect == 'pad_row0' and (gr.rows < 0).any():        # a padding row's zero product, stored through row index max(-1, 0)
        C[0, :N] = act32(torch.zeros(1, N) + c_in(np.array([0])), act)[0]
    if defect == 'zero_unlisted':
        C[torch.from_numpy(~gr.listed), :N] = 0.0
    return C, before


def emulate_tile_stats(stored, rows, defect=None, groups=None):
    """[T, 3, N] float32 in the order of gemm.hip:611-648"""
    x_all = stored.numpy().astype(f32)
    T, N = rows.shape[0] // 64, x_all.shape[1]
    out = np.zeros((T, 3, N), dtype=f32)
    for t in range(T):
        r = rows[t * 64:(t + 1) * 64]
        valid = r >= 0
        x = np.where(valid[:, None], x_all[np.maximum(r, 0)], f32(0))
        v = valid.astype(f32)
        if defect == 'count_pad':
            v = np.ones(64, dtype=f32)
        qs, qc = [], []
        for part in range(4):
            s1, cnt = np.zeros(N, dtype=f32), f32(0)
            for k in range(16):
                s1 = s1 + x[part * 16 + k]
                cnt = cnt + v[part * 16 + k]
            qs.append(s1)
            qc.append(cnt)
        tot = ((qs[0] + qs[1]) + qs[2]) + qs[3]
        n_rows = ((qc[0] + qc[1]) + qc[2]) + qc[3]
        mean = tot / n_rows if n_rows > 0 else np.zeros(N, dtype=f32)
        if defect == 'm2_group_mean':
            start, count = next((s, c) for _, s, c in groups if s <= t * 64 < s + max(c, 1))
            mean = x_all[rows[start:start + count]].astype(np.float64).mean(0).astype(f32)
        qm = []
        for part in range(4):
            m2 = np.zeros(N, dtype=f32)
            for k in range(16):
                if valid[part * 16 + k]:
                    d = x[part * 16 + k] - mean
                    m2 = m2 + d * d
            qm.append(m2)
        out[t, 0], out[t, 1], out[t, 2] = tot, ((qm[0] + qm[1]) + qm[2]) + qm[3], n_rows
    assert out.dtype == f32
    return out


def emulate_batched(inp, trans_b, mode, accumulate):
    gr, T, Fo, KA = inp.gr, inp.T, inp.Fo, inp.KA
    width = inp.Mq if trans_b else inp.AW
    C = torch.full((gr.n, width + R.PAD), R.POISON)
    if accumulate:
        C[:, :width] = inp.lin0
    before = C.clone() if accumulate else None
    for gi, (_, start, count) in enumerate(gr.groups):
        r = gr.rows[start:start + count].astype(np.int64)
        for t in range(T):
            w = inp.WD[gi, t * Fo:(t + 1) * Fo, t * KA:(t + 1) * KA]
            if trans_b:
                C[r, t * Fo:(t + 1) * Fo] = product32(inp.agg[r, t * KA:(t + 1) * KA], w.T.contiguous(), mode) + inp.lin0[r, t * Fo:(t + 1) * Fo]
            else:
                C[r, t * KA:(t + 1) * KA] = product32(inp.gl[r, t * Fo:(t + 1) * Fo], w.contiguous(), mode)
    return C, before


def emulate_wgrad(inp, accumulate, seg_rows=0, mode='fp32', defect=None, zero_group=None):
    """[G, M, N + PAD]: every group's A[rows]^T B[rows], in segments of seg_rows rows added one after the other"""
    gr, M, N = inp.gr, inp.M, inp.N
    C = torch.full((gr.n_groups, M, N + R.PAD), R.POISON)
    if accumulate:
        C[:, :, :N] = inp.c0
    lists = [gr.rows[s:s + c].astype(np.int64) for _, s, c in gr.groups]
    if zero_group is not None:
        lists[zero_group] = lists[zero_group][:0]
    if defect == 'row_to_neighbour':
        lists[1] = np.concatenate([lists[0][-1:], lists[1]])
        lists[0] = lists[0][:-1]
    for gi, r in enumerate(lists):
        if defect == 'stale_zero_group' and gi == zero_group:
            continue
        acc = inp.c0[gi].clone() if accumulate else torch.zeros(M, N)
        step = seg_rows or max(len(r), 1)
        for k in range(0, len(r), step):
            rr = r[k:k + step]
            acc = acc + product32(inp.dY[rr].T.contiguous(), inp.a[rr].contiguous(), mode)
        C[gi, :, :N] = acc
    return C


def emulate_combine_fwd(inp):
    W, S, A = inp.W.numpy(), inp.S, inp.A
    out = np.zeros((inp.G, inp.f_out, A), dtype=f32)
    for gi in range(inp.G):
        for s in range(S):
            out[gi] = out[gi] + inp.coef[gi, s] * W[:, s * A:(s + 1) * A]
    return out


def emulate_combine_bwd(inp):
    d, S, A = inp.dWD.numpy(), inp.S, inp.A
    out = np.zeros((inp.f_out, S * A), dtype=f32)
    for gi in range(inp.G):
        for s in range(S):
            out[:, s * A:(s + 1) * A] = out[:, s * A:(s + 1) * A] + inp.coef[gi, s] * d[gi]
    return out


# ---- the layouts are what the cases rely on ------------------------------------------------------------------------------------
def test_the_layouts():
    e0, e1 = R.grouping('edges', False), R.grouping('edges', True)
    assert e0.n == 457 and e0.m_padded == 704 and e1.m_padded == 768
    assert e0.tiles.tolist() == [0, 1, 2, 3, 3, 4, 4, 5, 5, 5, 6] and e1.tiles.tolist() == [0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 6, 7]
    assert [c for _, _, c in e0.groups] == [1, 63, 64, 65, 128, 129, 2] and (~e0.listed).sum() == 5 and e1.listed.all()
    valid = (e0.rows.reshape(-1, 64) >= 0).sum(1).tolist()
    assert valid == [1, 63, 64, 64, 1, 64, 64, 64, 64, 1, 2]
    one = R.grouping('one_group', False)
    assert one.n == 70 and one.n_groups == 1 and one.m_padded == 128
    mx = R.grouping('max_groups', False)
    assert mx.n_groups == 32 and {c for _, _, c in mx.groups} == {1, 2, 3} and mx.tiles.tolist() == list(range(32))
    lg = R.grouping('long', True)
    assert lg.n == 6200 and [c for _, _, c in lg.groups] == [3100, 3100]
    assert -(-3100 // 64) * 2 == 98 and -(-3100 // 128) * 2 == 50 and -(-3100 // 96) * 2 == 66       # the segment counts the cases name
    for name in ('edges', 'one_group', 'max_groups', 'long'):      # shuffled ids: row 0 is not special
        for z in (False, True):
            gr = R.grouping(name, z)
            assert sorted(gr.rows[gr.rows >= 0].tolist()) == np.nonzero(gr.listed)[0].tolist()


# ---- valid results stay inside the bounds ----------------------------------------------------------------------------------------
def _assert_product(v, what, fp32_mode=True):
    print(f'{what}: worst err / bound {v.ratio:.4f} at {v.index}, rms {v.rms:.3e}')
    assert v.ratio <= 1.0, (what, v.ratio, v.index)
    assert v.pad_ok and v.unlisted_ok, what
    if fp32_mode:
        assert v.rms < R.RMS_FP32, (what, v.rms)


@pytest.mark.parametrize('case', R.PRODUCT_CASES, ids=IDS)
@pytest.mark.parametrize('mode', ['fp32', 'split'])
def test_emulated_products_stay_inside_the_bound(case, mode):
    name, K, N = case
    for zero in (False, True):
        for trans_b, accumulate in ((1, 0), (1, 1), (0, 0)):
            inp = R.product_inputs(name, zero, K, N, trans_b)
            ref, mag = R.product_reference(name, zero, K, N, trans_b, accumulate)
            C, before = emulate_grouped(inp, accumulate, mode)
            _assert_product(R.verdict(C, ref, mag, inp.gr, K, before), f'{case} {mode} zero={zero} tb={trans_b} acc={accumulate}')


@pytest.mark.parametrize('case', R.BF16_CASES, ids=IDS)
def test_emulated_bf16_products_stay_inside_the_bound_of_the_rounded_operands(case):
    name, K, N = case
    for trans_b in (1, 0):
        inp = R.product_inputs(name, True, K, N, trans_b)
        ref, mag = R.product_reference(name, True, K, N, trans_b, 0, bf16=True)
        C, _ = emulate_grouped(inp, 0, 'bf16')
        _assert_product(R.verdict(C, ref, mag, inp.gr, K), f'{case} bf16 tb={trans_b}', fp32_mode=False)
        if K >= 40:      # and the rounding is not absorbed: against the unrounded product the same output is far outside
            ref, mag = R.product_reference(name, True, K, N, trans_b, 0)
            assert R.verdict(C, ref, mag, inp.gr, K).ratio > 10.0


def _fused(case, form, act, mode, defect=None, bf16=False):
    name, K, N = case
    inp = R.product_inputs(name, True, K, N, 1)
    buf, off, pitch = R.fused_addend(form, inp.c0, N)
    ref, mag = R.product_reference(name, True, K, N, 1, 1, bf16, act)
    C, before = emulate_grouped(inp, 1, mode, act, None if buf is None else (buf, off, pitch), defect)
    return inp, C, R.verdict(C, ref, mag, inp.gr, K, before)


@pytest.mark.parametrize('case', R.FUSED_CASES, ids=IDS)
@pytest.mark.parametrize('form', R.FUSED_FORMS)
def test_emulated_fused_product_and_statistics_stay_inside_the_bounds(case, form):
    worst_sum = worst_m2 = 0.0
    for act in R.FUSED_ACTS:
        for mode in ('fp32', 'split'):
            inp, C, v = _fused(case, form, act, mode)
            _assert_product(v, f'{case} {form} {act} {mode}')
            stored = C[:, :inp.N]
            s = R.stats_verdict(emulate_tile_stats(stored, inp.gr.rows), stored, inp.gr.rows)
            assert s.count_ok and s.single_ok and s.sum_ratio <= 1.0 and s.m2_ratio <= 1.0, (act, mode, vars(s))
            worst_sum, worst_m2 = max(worst_sum, s.sum_ratio), max(worst_m2, s.m2_ratio)
    print(f'{case} {form}: statistics worst err / bound: sum {worst_sum:.3f} M2 {worst_m2:.3f}')
    if case[0] == 'edges':
        assert s.n_single == 3      # the group of one row, the second tile of the 65-group and the third of the 129-group


@pytest.mark.parametrize('tower', R.TOWERS, ids=IDS)
@pytest.mark.parametrize('mode', ['fp32', 'split'])
def test_emulated_batched_products_stay_inside_the_bound(tower, mode):
    for zero in (False, True):
        inp = R.tower_inputs('edges', zero, *tower)
        for trans_b, accumulate, K in ((1, 1, inp.KA), (0, 0, inp.Fo)):
            ref, mag = R.ref_batched(inp, trans_b, inp.lin0 if accumulate else None)
            C, before = emulate_batched(inp, trans_b, mode, accumulate)
            _assert_product(R.verdict(C, ref, mag, inp.gr, K, before), f'{tower} {mode} zero={zero} tb={trans_b}')


@pytest.mark.parametrize('case', R.WGRAD_CASES, ids=IDS)
def test_emulated_weight_gradients_stay_inside_the_bound_of_each_group(case):
    name, M, N = case
    inp = R.wgrad_inputs(name, M, N)
    for accumulate in (0, 1):
        for seg in R.WGRAD_SEG_ROWS[name]:
            for mode, bf16 in (('fp32', False), ('bf16', True)):
                C = emulate_wgrad(inp, accumulate, seg, mode)
                assert torch.all(C[:, :, N:] == R.POISON)
                for gi, (ref, mag, count) in enumerate(R.wgrad_reference(name, M, N, accumulate, bf16)):
                    ratio, idx = R.check(C[gi, :, :N], ref, mag, count)
                    assert ratio <= 1.0, (case, accumulate, seg, mode, gi, count, ratio, idx)
                    assert bf16 or R.rms_rel(C[gi, :, :N], ref) < R.RMS_FP32


@pytest.mark.parametrize('case', R.COMBINE_CASES, ids=IDS)
def test_emulated_combined_weights_stay_inside_the_bound(case):
    inp = R.combine_inputs(*case)
    ref, mag = R.ref_combine_fwd(inp.W, inp.coef, inp.A)
    rf, _ = R.worst(emulate_combine_fwd(inp), ref, (inp.S + 1) * R.U * mag)
    ref, mag = R.ref_combine_bwd(inp.dWD, inp.coef)
    rb, _ = R.worst(emulate_combine_bwd(inp), ref, (inp.S + 1) * R.U * mag)
    print(f'{case}: combined weights worst err / bound: forward {rf:.3f} backward {rb:.3f}')
    assert rf <= 1.0 and rb <= 1.0


# ---- defects leave the bounds ------------------------------------------------------------------------------------------------------
def _product_defect_cases(defect):
    """(case, include_zero, trans_b, accumulate) where the defect can occur"""
    for case in R.PRODUCT_CASES:
        name = case[0]
        for zero in (False, True):
            for trans_b, accumulate in ((1, 0), (1, 1), (0, 0)):
                if defect == 'next_weight' and name == 'one_group':
                    continue                                   # there is no next group
                if defect == 'pad_row0' and accumulate:
                    continue                                   # (in place the addend of row 0 is rewritten by itself)
                if defect == 'zero_unlisted' and (zero or name != 'edges'):
                    continue                                   # every node is in a group
                yield case, zero, trans_b, accumulate


@pytest.mark.parametrize('defect', ['drop_k', 'next_weight', 'pad_row0', 'zero_unlisted'])
def test_a_defect_of_the_grouped_product_is_flagged_on_every_case(defect):
    """the last K element dropped; the last tile of a group on the next group's weight; a padding row written to row 0; the rows
    in no group overwritten with zeros"""
    n_cases, frac = 0, []
    for case, zero, trans_b, accumulate in _product_defect_cases(defect):
        name, K, N = case
        inp = R.product_inputs(name, zero, K, N, trans_b)
        gr = inp.gr
        ref, mag = R.product_reference(name, zero, K, N, trans_b, accumulate)
        for mode in ('fp32', 'split'):
            C, before = emulate_grouped(inp, accumulate, mode, defect=defect)
            v = R.verdict(C, ref, mag, gr, K, before)
            what = (defect, case, zero, trans_b, accumulate, mode)
            if defect == 'drop_k':      # at least one element of every affected row (the D = 0 group's weight is zero)
                flagged = R.flagged_rows(C[:, :N], ref, mag, K)
                affected = gr.listed & ~((gr.group_of == 0) & (gr.groups[0][0] == 0))
                assert flagged[affected].all(), what
                err = np.abs(C[:, :N].double().numpy() - ref)[affected]
                frac.append(float((err > (K + 6) * R.U * mag[affected]).mean()))
            elif defect == 'next_weight':
                rows = np.concatenate([R.last_tile_rows(gr, gi) for gi in range(gr.n_groups - 1)])
                assert R.flagged_rows(C[:, :N], ref, mag, K)[rows].all(), what
            elif defect == 'pad_row0':
                assert v.ratio > 1.0 or not v.unlisted_ok, what
            else:
                assert not v.unlisted_ok, what
            n_cases += 1
    assert n_cases > 0
    if frac:
        print(f'{defect}: flagged {min(frac):.0%} .. {max(frac):.0%} of the elements of the affected rows, {n_cases} cases')


@pytest.mark.parametrize('case', R.FUSED_CASES, ids=IDS)
def test_defects_of_the_fused_form_are_flagged(case):
    """c_in read at pitch N instead of ldcin; a padding row counted; M2 about the group mean instead of the tile mean"""
    for form in ('separate', 'wide'):
        for act in R.FUSED_ACTS:
            _, _, v = _fused(case, form, act, 'split', defect='cin_pitch')
            assert v.ratio > 1.0, (case, form, act)
    inp, C, v = _fused(case, 'wide', 'relu', 'split')
    assert v.ratio <= 1.0
    stored, gr = C[:, :inp.N], inp.gr
    assert (gr.rows < 0).any()
    assert not R.stats_verdict(emulate_tile_stats(stored, gr.rows, 'count_pad'), stored, gr.rows).count_ok
    if any(c > 64 for _, _, c in gr.groups):      # a group of more than one tile: its tiles have means of their own
        s = R.stats_verdict(emulate_tile_stats(stored, gr.rows, 'm2_group_mean', gr.groups), stored, gr.rows)
        assert s.m2_ratio > 1.0 or not s.single_ok, case
    else:
        assert case[0] == 'max_groups'


@pytest.mark.parametrize('case', R.WGRAD_CASES, ids=IDS)
def test_defects_of_the_weight_gradient_are_flagged(case):
    """one row of a group given to the neighbouring group; a zero-count group left stale"""
    name, M, N = case
    inp = R.wgrad_inputs(name, M, N)
    refs = R.wgrad_reference(name, M, N, 0)
    C = emulate_wgrad(inp, 0, defect='row_to_neighbour')
    for gi in (0, 1):
        ref, mag, count = refs[gi]
        assert R.check(C[gi, :, :N], ref, mag, count)[0] > 1.0, (case, gi)
    zg = inp.gr.n_groups - 1
    good = emulate_wgrad(inp, 0, zero_group=zg)
    assert torch.all(good[zg, :, :N] == 0)
    stale = emulate_wgrad(inp, 0, defect='stale_zero_group', zero_group=zg)
    assert not torch.all(stale[zg, :, :N] == 0)


@pytest.mark.parametrize('case', [c for c in R.PRODUCT_CASES if c[0] == 'edges'], ids=IDS)
def test_a_lost_low_part_of_the_split_trips_the_rms_figure(case):
    """the elementwise worst-case bound does not see it (at K = 800), the 1e-6 rms figure of fp32 mode does"""
    name, K, N = case
    inp = R.product_inputs(name, False, K, N, 1)
    ref, mag = R.product_reference(name, False, K, N, 1, 0)
    good = R.verdict(emulate_grouped(inp, 0, 'split')[0], ref, mag, inp.gr, K)
    bad = R.verdict(emulate_grouped(inp, 0, 'split', defect='drop_low')[0], ref, mag, inp.gr, K)
    print(f'{case}: rms {good.rms:.3e} -> {bad.rms:.3e} without the low parts; err / bound {good.ratio:.3f} -> {bad.ratio:.3f}')
    assert good.rms < R.RMS_FP32 <= bad.rms
