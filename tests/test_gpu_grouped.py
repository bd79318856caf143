"""-m gpu: the degree-grouped posttrans products at their edges, through the C ABI, against the fp64 references and the DERIVED
bounds of tests/grouped_reference.py (tests/test_grouped_bounds_cpu.py shows that the bounds hold for a correct fp32 evaluation and
that the defects a rewrite of these kernels can have leave them).

Every output is pre-filled with the poison 7.0 at row pitch N + 8: the pad columns must still hold it, the rows in no group must
still hold it (accumulate = 0) or be bit-unchanged (accumulate = 1).  Every index handed to a kernel is in range.

Measured on the MI355X, the worst err / bound over all cases of a test and the worst rms relative error against fp64 (the figure
fp32 mode is held to is 1e-6); the bounds are derived and do not depend on these numbers:
    grouped forward, fp32 mode           0.137    rms 4.3e-7        grouped forward / data gradient, bf16 mode   0.066    rms 1.6e-7
    grouped data gradient, fp32 mode     0.115    rms 4.3e-7        fused product, bf16 mode                     0.0016   rms 1.2e-7
    fused product, fp32 mode             0.106    rms 3.0e-7        tile statistics, bf16 mode    sum 0.49   M2 0.38
    tile statistics, fp32 mode    sum 0.58   M2 0.44                weight gradients, bf16 mode                  0.085    rms 5.7e-8
    batched (towers), fp32 mode          0.132    rms 9.3e-8        combined weights    forward 0.53   backward 0.91
    weight gradients, fp32 mode: through the scratch 0.270, rms 4.6e-7;  through atomics 0.270, rms 6.2e-7
(the worst product ratios belong to K <= 20, where the bound is 14 .. 26 u mag; at K = 800 they are near 0.001.  The 0.91 of the combined
weights is the backward at one scaler and 32 groups: 31 additions against a bound of two roundings - the sequential fp32 sum of the
CPU emulation gives the same figure to four digits.)

Which path a case takes, read from gemm_impl / rowseg_impl / i3d_gemm_f32_fused_src with the case's sizes:
    (800, 200), (8, 8), (80, 20): 64x32 tiles, Cfg11 (narrow_pays);  (800, 256), (200, 800), (20, 36), (48, 64): 64x64, Cfg9;
    (18, 7): K % 4 != 0, so Cfg11 in its non-vector instantiation, forward and data-gradient layout;
    bf16 mode: (40, 36) Cfg13, (8, 8) and (800, 200) Cfg14, the fused (800, 200) Cfg14;  the towers: Cfg11 with n_batch 3 and 5;
    weight gradients without the scratch: fp32 atomics on a zero fill; with it: slices and slab_reduce_kernel, except
    `long` at seg_rows 96 (66 slices >= 4 ZL, 128 items): slab_reduce_small_kernel;  `long` at seg_rows 64: 98 segments > MAX_SEGS,
    one doubling to 128 rows, 50 slices (so that case alone does not reach the small reduction: 96 was added for it).
"""
import contextlib
import importlib

import numpy as np
import pytest
import torch

import grouped_reference as R

pytestmark = pytest.mark.gpu

ops = None
lib_mod = None
L = None
DEV = None
WORST = {}                                # test -> the worst figures it saw (printed when the module is done)
IDS = lambda c: '-'.join(str(v) for v in c)      # noqa: E731


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    global ops, lib_mod, L, DEV
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    ops = importlib.import_module('3dinfomax_amd.ops')
    lib_mod = importlib.import_module('3dinfomax_amd._lib')
    L = lib_mod.load()
    DEV = torch.device('cuda:0')
    yield
    for key in sorted(WORST):
        print(f'\nMEASURED {key}: ' + ' '.join(f'{k}={v:.3e}' for k, v in sorted(WORST[key].items())), end='')


def g(t):
    return t.to(DEV)


def note(test, **figures):
    w = WORST.setdefault(test, {})
    for k, v in figures.items():
        w[k] = max(w.get(k, 0.0), float(v))


@contextlib.contextmanager
def precision(name):
    prev = ops.set_matmul_precision(name)
    try:
        yield
    finally:
        ops.set_matmul_precision(prev)


def index_tensors(gr):
    assert gr.rows.min() >= -1 and gr.rows.max() < gr.n and gr.tiles.min() >= 0 and gr.tiles.max() < gr.n_groups
    assert gr.m_padded % 64 == 0 and gr.tiles.shape[0] == gr.m_padded // 64
    return g(torch.from_numpy(gr.rows)), g(torch.from_numpy(gr.tiles))


def poisoned(rows, width, content=None):
    """[rows, width + PAD] of poison; content goes into the first `width` columns"""
    C = torch.full((rows, width + R.PAD), R.POISON, device=DEV)
    if content is not None:
        C[:, :width] = g(content)
    return C


def assert_product(v, what, test, fp32_mode=True):
    print(f'{what}: worst err / bound {v.ratio:.4f} at {v.index}, rms {v.rms:.3e}')
    note(test, ratio=v.ratio, rms=v.rms)
    assert v.pad_ok, f'{what}: a pad column lost its poison'
    assert v.unlisted_ok, f'{what}: a row in no group was written'
    assert v.ratio <= 1.0, f'{what}: err / bound {v.ratio} at (row, column) {v.index}'
    if fp32_mode:
        assert v.rms < R.RMS_FP32, f'{what}: rms relative error {v.rms}'


def run_grouped(inp, accumulate):
    gr, K, N = inp.gr, inp.K, inp.N
    rows, tiles = index_tensors(gr)
    A, B = g(inp.A), g(inp.B)
    C = poisoned(gr.n, N, inp.c0 if accumulate else None)
    before = C.clone() if accumulate else None
    lib_mod.check(L.i3d_gemm_f32_grouped(inp.trans_b, gr.m_padded, N, K, A.data_ptr(), K, gr.n, rows.data_ptr(), tiles.data_ptr(),
                                         B.data_ptr(), K if inp.trans_b else N, N * K, C.data_ptr(), N + R.PAD, accumulate,
                                         ops._stream()), 'i3d_gemm_f32_grouped')
    return C, before


# ---- 1, 2: i3d_gemm_f32_grouped ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.PRODUCT_CASES, ids=IDS)
@pytest.mark.parametrize('include_zero', [False, True])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_grouped_forward(case, include_zero, accumulate):
    """C[r] (+)= A[r] B_g(r)^T: (800, 200) on 64x32 tiles (Cfg11), (800, 256) on 64x64 (Cfg9), K shorter than a K-tile, a K tail,
    ragged column tiles, the unaligned non-vector kernel at (18, 7); groups of 1, 2, 63, 64, 65 rows, 32 groups"""
    name, K, N = case
    inp = R.product_inputs(name, include_zero, K, N, 1)
    ref, mag = R.product_reference(name, include_zero, K, N, 1, accumulate)
    C, before = run_grouped(inp, accumulate)
    assert_product(R.verdict(C, ref, mag, inp.gr, K, before), f'forward {case} zero={include_zero} acc={accumulate}', 'grouped forward fp32')


@pytest.mark.parametrize('case', R.PRODUCT_CASES, ids=IDS)
@pytest.mark.parametrize('include_zero', [False, True])
def test_grouped_data_gradient(case, include_zero):
    """C[r] = A[r] B_g(r) (trans_b = 0), the same checks"""
    name, K, N = case
    inp = R.product_inputs(name, include_zero, K, N, 0)
    ref, mag = R.product_reference(name, include_zero, K, N, 0, 0)
    C, before = run_grouped(inp, 0)
    assert_product(R.verdict(C, ref, mag, inp.gr, K, before), f'data gradient {case} zero={include_zero}', 'grouped data gradient fp32')


@pytest.mark.parametrize('case', R.BF16_CASES, ids=IDS)
@pytest.mark.parametrize('trans_b', [1, 0])
def test_grouped_products_in_bf16_mode(case, trans_b):
    """K-tile 32 (Cfg13 / Cfg14): the same bound against the fp64 product of the bf16-rounded operands - not a wider one"""
    name, K, N = case
    inp = R.product_inputs(name, True, K, N, trans_b)
    ref, mag = R.product_reference(name, True, K, N, trans_b, 0, bf16=True)
    with precision('bf16'):
        C, before = run_grouped(inp, 0)
    assert_product(R.verdict(C, ref, mag, inp.gr, K, before), f'bf16 {case} tb={trans_b}', 'grouped products bf16', fp32_mode=False)
    if K >= 40:      # (the mode did switch: against the unrounded product the output is far outside)
        ref, mag = R.product_reference(name, True, K, N, trans_b, 0)
        assert R.verdict(C, ref, mag, inp.gr, K, before).ratio > 10.0


# ---- 3: i3d_gemm_f32_fused_src, grouped ---------------------------------------------------------------------------------------------
def finalize_check(partial, tiles, stored):
    """ops.bn_finalize_partials on the per-tile partials, held to the tolerances of check_stats (tests/test_gpu_fused_bn.py)"""
    feat, momentum = stored.shape[1], 0.93
    rnd = lambda seed: torch.randn(feat, generator=torch.Generator().manual_seed(seed))      # noqa: E731
    gamma, beta, rm, rv = 1 + 0.2 * rnd(7), 0.2 * rnd(8), rnd(90), rnd(91).abs() + 0.5
    rm_d, rv_d = g(rm.clone()), g(rv.clone())
    nbt = torch.tensor(4, dtype=torch.int64, device=DEV)
    mean, invstd, aff = ops.bn_finalize_partials(partial, tiles, feat, 1e-5, momentum, g(gamma), g(beta), rm_d, rv_d, nbt)
    x = stored.double()
    m_ref, var = x.mean(0), x.var(0, unbiased=False)
    is_ref, unb = 1.0 / torch.sqrt(var + 1e-5), x.var(0, unbiased=True)
    rel = lambda a, b: ((a.double() - b).abs().max() / b.abs().max()).item()      # noqa: E731  (helpers.rel_err)
    assert ((mean.cpu().double() - m_ref).abs() / (1 / is_ref + m_ref.abs() * 1e-6)).max().item() < 2e-6
    assert rel(invstd.cpu(), is_ref) < 1e-5
    assert rel(rm_d.cpu(), (1 - momentum) * rm.double() + momentum * m_ref) < 1e-5
    assert rel(rv_d.cpu(), (1 - momentum) * rv.double() + momentum * unb) < 1e-5
    assert int(nbt.item()) == 5
    assert torch.equal(aff[0], mean) and torch.equal(aff[2].cpu(), beta)
    assert rel(aff[1].cpu(), gamma.double() * is_ref) < 1e-5


def run_fused(case, form, act, bf16=False):
    name, K, N = case
    inp = R.product_inputs(name, True, K, N, 1)
    gr = inp.gr
    rows, tiles = index_tensors(gr)
    A, W = g(inp.A), g(inp.B)
    buf, off, pitch = R.fused_addend(form, inp.c0, N)
    C = poisoned(gr.n, N, inp.c0 if buf is None else None)
    before = C.clone() if buf is None else None
    buf_d = None if buf is None else g(buf)
    T = gr.m_padded // 64
    partial = torch.full((T, 3, N), R.POISON, device=DEV)
    c_in = 0 if buf is None else buf_d.data_ptr() + 4 * off
    assert c_in % 16 == 0 and pitch % 4 == 0 and (buf is None or off + N <= pitch)
    lib_mod.check(L.i3d_gemm_f32_fused_src(gr.m_padded, N, K, A.data_ptr(), K, gr.n, W.data_ptr(), K, C.data_ptr(), N + R.PAD,
                                           c_in or None, pitch, None, 1, None, lib_mod.ACT[act], partial.data_ptr(), rows.data_ptr(),
                                           tiles.data_ptr(), N * K, ops._stream()), 'i3d_gemm_f32_fused_src')
    if buf is not None:
        assert torch.equal(buf_d.cpu(), buf), 'the addend was written'
    ref, mag = R.product_reference(name, True, K, N, 1, 1, bf16, act)
    return inp, C, partial, R.verdict(C, ref, mag, gr, K, before)


@pytest.mark.parametrize('case', R.FUSED_CASES, ids=IDS)
@pytest.mark.parametrize('form', R.FUSED_FORMS)
@pytest.mark.parametrize('act', R.FUSED_ACTS)
def test_fused_grouped_product_and_tile_statistics(case, form, act):
    """the product path of the native model (composite.hip:538): lin (+)= agg W_D^T with the addend in place, from a separate c_in,
    from c_in as a column block of a wider matrix; the activation; the statistics of the STORED values, tile by tile"""
    inp, C, partial, v = run_fused(case, form, act)
    what = f'fused {case} {form} {act}'
    assert_product(v, what, 'fused product fp32')
    stored = C[:, :inp.N].cpu()
    s = R.stats_verdict(partial.cpu(), stored, inp.gr.rows)
    print(f'{what}: statistics worst err / bound: sum {s.sum_ratio:.4f} at {s.sum_index}, M2 {s.m2_ratio:.4f} at {s.m2_index}')
    note('fused tile statistics', sum_ratio=s.sum_ratio, m2_ratio=s.m2_ratio)
    assert s.count_ok, f'{what}: a tile count is not the number of its valid rows'
    assert s.single_ok, f'{what}: a tile of one row: sum must be the stored value, M2 0.0'
    assert s.sum_ratio <= 1.0, f'{what}: tile sum err / bound {s.sum_ratio} at (tile, column) {s.sum_index}'
    assert s.m2_ratio <= 1.0, f'{what}: tile M2 err / bound {s.m2_ratio} at (tile, column) {s.m2_index}'
    if case[0] == 'edges':
        assert s.n_single == 3
    finalize_check(partial, inp.gr.m_padded // 64, stored)


def test_fused_grouped_product_in_bf16_mode():
    with precision('bf16'):
        inp, C, partial, v = run_fused(('edges', 800, 200), 'wide', 'relu', bf16=True)
    assert_product(v, 'fused bf16', 'fused product bf16', fp32_mode=False)
    s = R.stats_verdict(partial.cpu(), C[:, :inp.N].cpu(), inp.gr.rows)
    note('fused tile statistics bf16', sum_ratio=s.sum_ratio, m2_ratio=s.m2_ratio)
    assert s.count_ok and s.single_ok and s.sum_ratio <= 1.0 and s.m2_ratio <= 1.0, vars(s)


# ---- 4: i3d_gemm_f32_grouped_batched ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tower', R.TOWERS, ids=IDS)
@pytest.mark.parametrize('include_zero', [False, True])
def test_grouped_batched_products(tower, include_zero):
    """the diagonal blocks of W_D per tower with the strides of tower.hip:120 (forward, accumulate) and :208 (data gradient); the
    blocks off the diagonal hold 1e3: one read of them breaks the bound"""
    inp = R.tower_inputs('edges', include_zero, *tower)
    gr, T, Fo, KA, AW, Mq = inp.gr, inp.T, inp.Fo, inp.KA, inp.AW, inp.Mq
    rows, tiles = index_tensors(gr)
    agg, gl, WD = g(inp.agg), g(inp.gl), g(inp.WD)
    lin = poisoned(gr.n, Mq, inp.lin0)
    before = lin.clone()
    lib_mod.check(L.i3d_gemm_f32_grouped_batched(1, gr.m_padded, Fo, KA, agg.data_ptr(), AW, KA, gr.n, rows.data_ptr(), tiles.data_ptr(),
                                                 WD.data_ptr(), AW, Mq * AW, Fo * AW + KA, lin.data_ptr(), Mq + R.PAD, Fo, T, 1,
                                                 ops._stream()), 'i3d_gemm_f32_grouped_batched')
    ref, mag = R.ref_batched(inp, 1, inp.lin0)
    assert_product(R.verdict(lin, ref, mag, gr, KA, before), f'batched forward {tower} zero={include_zero}', 'batched fp32')
    g_agg = poisoned(gr.n, AW)
    lib_mod.check(L.i3d_gemm_f32_grouped_batched(0, gr.m_padded, KA, Fo, gl.data_ptr(), Mq, Fo, gr.n, rows.data_ptr(), tiles.data_ptr(),
                                                 WD.data_ptr(), AW, Mq * AW, Fo * AW + KA, g_agg.data_ptr(), AW + R.PAD, KA, T, 0,
                                                 ops._stream()), 'i3d_gemm_f32_grouped_batched')
    ref, mag = R.ref_batched(inp, 0)
    assert_product(R.verdict(g_agg, ref, mag, gr, Fo), f'batched data gradient {tower} zero={include_zero}', 'batched fp32')


# ---- 5: i3d_gemm_f32_rowsubset_multi ------------------------------------------------------------------------------------------------
def run_wgrad(inp, C, counts, accumulate, cfg, seg, use_ws):
    gr, M, N = inp.gr, inp.M, inp.N
    starts = [s for _, s, _ in gr.groups]
    assert all(0 <= s and s + c <= gr.m_padded for s, c in zip(starts, counts))
    assert all((gr.rows[s:s + c] >= 0).all() for s, c in zip(starts, counts))       # no padding row inside a range
    ws = ops._gemm_workspace(DEV) if use_ws else None
    lib_mod.check(L.i3d_gemm_f32_rowsubset_multi(M, N, gr.n_groups, lib_mod.int_array(starts), lib_mod.int_array(counts),
                                                 inp.dY_d.data_ptr(), M, inp.a_d.data_ptr(), N, inp.rows_d.data_ptr(), gr.n,
                                                 C.data_ptr(), M * (N + R.PAD), N + R.PAD, accumulate, cfg, seg,
                                                 ws.data_ptr() if use_ws else None, ops.GEMM_WORKSPACE_BYTES if use_ws else 0,
                                                 ops._stream()), 'i3d_gemm_f32_rowsubset_multi')
    return C


def wgrad_device_inputs(name, M, N):
    inp = R.wgrad_inputs(name, M, N)
    dev = type(inp)(**vars(inp))
    dev.dY_d, dev.a_d, dev.rows_d = g(inp.dY), g(inp.a), g(torch.from_numpy(inp.gr.rows))
    return dev


def check_wgrad(C, refs, N, what, test, skip=None, fp32_mode=True):
    out = C.cpu()
    assert torch.all(out[:, :, N:] == R.POISON), f'{what}: a pad column lost its poison'
    for gi, (ref, mag, count) in enumerate(refs):
        if gi == skip:
            continue
        ratio, idx = R.check(out[gi, :, :N], ref, mag, count)
        rms = R.rms_rel(out[gi, :, :N], ref)
        note(test, ratio=ratio, rms=rms)
        assert ratio <= 1.0, f'{what}: group {gi} of {count} rows: err / bound {ratio} at {idx}'
        if fp32_mode:
            assert rms < R.RMS_FP32, f'{what}: group {gi} of {count} rows: rms relative error {rms}'
    return out


@pytest.mark.parametrize('case', R.WGRAD_CASES, ids=IDS)
@pytest.mark.parametrize('use_ws', [True, False])
@pytest.mark.parametrize('cfg', R.WGRAD_CFGS)
def test_weight_gradient_of_every_group(case, use_ws, cfg):
    """dW_g of EVERY group against fp64 with the group's own reduction length (groups of 1 and 2 rows next to groups of 129 and
    3100), with the scratch (slices + fixed-order reduction; on `long` at seg_rows 96 the small reduction, at 64 the doubling of the
    segment length) and without (fp32 atomics on a zero fill); on top of a known matrix; a group of zero rows"""
    name, M, N = case
    inp = wgrad_device_inputs(name, M, N)
    gr = inp.gr
    counts = [c for _, _, c in gr.groups]
    zg = gr.n_groups - 1
    less = counts[:zg] + [0]
    for seg in R.WGRAD_SEG_ROWS[name]:
        what = f'wgrad {case} ws={use_ws} cfg={cfg} seg={seg}'
        test = 'weight gradient fp32 ' + ('scratch' if use_ws else 'atomics')
        first = check_wgrad(run_wgrad(inp, poisoned(gr.n_groups * M, N).view(gr.n_groups, M, -1), counts, 0, cfg, seg, use_ws),
                            R.wgrad_reference(name, M, N, 0), N, what, test)
        if use_ws:      # slices summed in a fixed order: the same bits every time
            again = run_wgrad(inp, poisoned(gr.n_groups * M, N).view(gr.n_groups, M, -1), counts, 0, cfg, seg, use_ws).cpu()
            assert torch.equal(first, again), f'{what}: two runs differ'
        # on top of a known matrix, the last group with no rows: bit-unchanged
        C = poisoned(gr.n_groups * M, N, inp.c0.reshape(-1, N)).view(gr.n_groups, M, -1)
        out = check_wgrad(run_wgrad(inp, C, less, 1, cfg, seg, use_ws), R.wgrad_reference(name, M, N, 1), N, what + ' acc', test, skip=zg)
        assert torch.equal(out[zg, :, :N], inp.c0[zg]), f'{what}: the group without rows changed under accumulate'
        # ... and all zeros without accumulate
        out = run_wgrad(inp, poisoned(gr.n_groups * M, N).view(gr.n_groups, M, -1), less, 0, cfg, seg, use_ws).cpu()
        assert torch.all(out[zg, :, :N] == 0), f'{what}: the group without rows is not zero'
        assert torch.all(out[:, :, N:] == R.POISON)


def test_weight_gradient_in_bf16_mode():
    name, M, N = 'edges', 36, 20
    inp = wgrad_device_inputs(name, M, N)
    gr = inp.gr
    with precision('bf16'):
        C = run_wgrad(inp, poisoned(gr.n_groups * M, N).view(gr.n_groups, M, -1), [c for _, _, c in gr.groups], 0, -1, 0, True)
    check_wgrad(C, R.wgrad_reference(name, M, N, 0, bf16=True), N, 'wgrad bf16', 'weight gradient bf16', fp32_mode=False)
    worst_unrounded = max(R.check(C[gi, :, :N].cpu(), ref, mag, count)[0] for gi, (ref, mag, count) in enumerate(R.wgrad_reference(name, M, N, 0)))
    assert worst_unrounded > 10.0      # (the mode did switch)


# ---- 6: combine_weights_fwd / _bwd ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.COMBINE_CASES, ids=IDS)
def test_combined_weights(case):
    """W_D = sum_s c_s W_s and dW_s = sum_g c_s(g) dW_D(g) with the weight a column block of a wider matrix: the columns outside
    the scaler blocks keep their poison; 33 groups are refused and nothing is launched"""
    inp = R.combine_inputs(*case)
    S, G, f_out, A = inp.S, inp.G, inp.f_out, inp.A
    f_in, lead, ldw = 8, 4, 4 + 8 + S * A + R.PAD        # the weight starts 4 columns into a wider matrix
    coef = ops._float_array([float(c) for c in inp.coef.reshape(-1)])
    wide = torch.full((f_out, ldw), R.POISON)
    wide[:, lead + f_in:lead + f_in + S * A] = inp.W
    wide_d = g(wide)
    WD = torch.full((G, f_out, A), R.POISON, device=DEV)
    lib_mod.check(L.i3d_pna_combine_weights_fwd(wide_d.data_ptr() + 4 * lead, ldw, f_in, f_out, A, G, S, coef, WD.data_ptr(), ops._stream()),
                  'i3d_pna_combine_weights_fwd')
    ref, mag = R.ref_combine_fwd(inp.W, inp.coef, A)
    rf, idx = R.worst(WD.cpu(), ref, (S + 1) * R.U * mag)
    assert rf <= 1.0, (case, 'forward', rf, idx)
    assert torch.equal(wide_d.cpu(), wide)
    dW = torch.full((f_out, ldw), R.POISON, device=DEV)
    dWD = g(inp.dWD)
    lib_mod.check(L.i3d_pna_combine_weights_bwd(dWD.data_ptr(), ldw, f_in, f_out, A, G, S, coef, dW.data_ptr() + 4 * lead, ops._stream()),
                  'i3d_pna_combine_weights_bwd')
    ref, mag = R.ref_combine_bwd(inp.dWD, inp.coef)
    out = dW.cpu()
    rb, idx = R.worst(out[:, lead + f_in:lead + f_in + S * A], ref, (S + 1) * R.U * mag)
    print(f'combined weights {case}: worst err / bound: forward {rf:.4f} backward {rb:.4f}')
    note('combined weights', forward_ratio=rf, backward_ratio=rb)
    assert rb <= 1.0, (case, 'backward', rb, idx)
    assert torch.all(out[:, :lead + f_in] == R.POISON) and torch.all(out[:, lead + f_in + S * A:] == R.POISON)


def test_combined_weights_refuse_33_groups():
    S, f_out, A, f_in = 3, 12, 20, 8
    coef = ops._float_array([1.0] * (33 * S))
    W = torch.full((f_out, f_in + S * A), 1.0, device=DEV)
    WD = torch.full((33, f_out, A), R.POISON, device=DEV)
    with pytest.raises(lib_mod.HipLibraryError):
        lib_mod.check(L.i3d_pna_combine_weights_fwd(W.data_ptr(), W.shape[1], f_in, f_out, A, 33, S, coef, WD.data_ptr(), ops._stream()),
                      'i3d_pna_combine_weights_fwd')
    dW = torch.full((f_out, f_in + S * A), R.POISON, device=DEV)
    with pytest.raises(lib_mod.HipLibraryError):
        lib_mod.check(L.i3d_pna_combine_weights_bwd(WD.data_ptr(), W.shape[1], f_in, f_out, A, 33, S, coef, dW.data_ptr(), ops._stream()),
                      'i3d_pna_combine_weights_bwd')
    torch.cuda.synchronize()
    assert torch.all(WD == R.POISON) and torch.all(dW == R.POISON)
