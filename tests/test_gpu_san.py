"""SAN on the MI355X: the attention kernels of csrc/san.hip against an fp64 torch composition (tests/san_reference.py), the model
against the reference's own outputs and gradients (tests/golden/gen_golden_san.py), the fused path against the composed one, the
absence of an edge-wide tensor, and a short training run.

Measured on the device, worst case of max |kernel - fp64| / max(4 x max |fp32 composition on the host - fp64|, 2^-20 x the tensor's
largest magnitude) per tensor (asserted <= 1, printed): out 0.25, s 0.13, dQ 0.30, dK 0.27, dV 0.26, dQ_2 0.52, dK_2 0.75, dTE 0.28,
dTE2 0.16; the model figures are in DESIGN.md, section SAN."""
import copy
import functools
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, grads_close, load, rel_err

import gen_golden_san as GS
import san_reference as R

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
san = importlib.import_module('3dinfomax_amd.san')
graph = importlib.import_module('3dinfomax_amd.graph')
DEV = torch.device('cuda:0')

# (H, heads, full_graph) -> (seed, scale of Q / K / the tables) of san_reference.make_case: 10-40 % of the scores saturate, none
# within 1e-3 of +-5 (tests/test_san_cpu.py::test_kernel_cases_saturate_as_stated checks it without a device)
CASE = {
    (64, 4, True): (1, 1.6), (64, 4, False): (1, 1.6),
    (24, 3, True): (1, 1.6), (24, 3, False): (1, 1.6),
    (8, 1, True): (1, 2.0), (8, 1, False): (1, 1.8),
    (200, 10, True): (1, 1.6), (200, 10, False): (1, 1.6),
}
# gamma does not enter without the full graph: one run there
RUNS = [(H, nh, True, gamma) for H, nh in R.SHAPES for gamma in (1e-6, 0.5)] + [(H, nh, False, 0.5) for H, nh in R.SHAPES]
BLOCKS = ('Q', 'K', 'V', 'Q2', 'K2')


@functools.lru_cache(maxsize=None)
def _case(H, nh, full_graph, gamma):
    """inputs, the fp64 reference and the fp32 composition's own error against it, computed once"""
    t, grad, idx, index, N = R.make_case(H, nh, full_graph, *CASE[(H, nh, full_graph)])
    ref = R.run(t, grad, idx, nh, gamma, full_graph, torch.float64)
    own = R.run(t, grad, idx, nh, gamma, full_graph, torch.float32)
    err32 = {k: float((own[k].double() - ref[k]).abs().max()) for k in ref}
    return t, grad, idx, index, N, ref, err32


def _device_run(t, grad, idx, index, nh, gamma, full_graph):
    names = BLOCKS if full_graph else BLOCKS[:3]
    Y = torch.cat([t[k] for k in names], 1).contiguous().to(DEV)
    te, te2 = t['TE'].to(DEV), (t['TE2'].to(DEV) if full_graph else None)
    codes = idx['code'].to(torch.int32).to(DEV)
    real = idx['real'].to(torch.uint8).to(DEV) if full_graph else None
    ix = index.to(DEV)
    order, ptr = ops.code_sorted_index(codes, R.NUM_CODES)
    out, s, z = ops.san_attn_fwd(Y, te, te2, codes, real, ix.in_ptr, ix.src_s, nh, gamma, full_graph)
    dY, dte, dte2 = ops.san_attn_bwd(grad.to(DEV), out, z, s, Y, te, te2, codes, real, ix, order, ptr, nh, gamma, full_graph)
    res = {'out': out, 's': s, 'dTE': dte}
    H = te.shape[1]
    for b, k in enumerate(names):
        res['d' + k] = dY[:, b * H:(b + 1) * H]
    if full_graph:
        res['dTE2'] = dte2
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize('H, nh, full_graph, gamma', RUNS)
def test_kernels_against_fp64(H, nh, full_graph, gamma):
    t, grad, idx, index, N, ref, err32 = _case(H, nh, full_graph, gamma)
    s = ref['s'].abs()
    share = float((s > 5).double().mean())
    assert 0.10 <= share <= 0.40 and float((s - 5).abs().min()) > 1e-3, share
    got = _device_run(t, grad, idx, index, nh, gamma, full_graph)
    assert set(got) == set(ref)
    worst = {}
    for k, r in ref.items():
        err = float((got[k].double() - r).abs().max())
        tol = max(4 * err32[k], 2.0 ** -20 * float(r.abs().max()))
        worst[k] = err / tol
        print(f'san kernel H={H} nh={nh} full={int(full_graph)} gamma={gamma:g} {k}: err {err:.3e} err32 {err32[k]:.3e} '
              f'err/tol {err / tol:.3f}')
    assert max(worst.values()) <= 1.0, worst
    # exact: the node without in-edges (complete batch: the one-atom molecule is node 0, it has no out-edges either), the absent code
    deg = np.diff(index.in_ptr.numpy())
    lone = [v for v in np.nonzero(deg == 0)[0] if not (idx['src'] == v).any()]
    assert lone
    for v in lone:
        for k in ('out',) + tuple('d' + b for b in (BLOCKS if full_graph else BLOCKS[:3])):
            assert torch.count_nonzero(got[k][v]) == 0, (k, v)
    for k in ('dTE', 'dTE2') if full_graph else ('dTE',):
        assert torch.count_nonzero(got[k][R.ABSENT_CODE]) == 0
    again = _device_run(t, grad, idx, index, nh, gamma, full_graph)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_shapes_outside_the_lane_map_are_not_taken_and_empty_batches_launch_nothing():
    assert not ops.san_attn_takes(130, 2, 60) and not ops.san_attn_takes(64, 4, 257) and ops.san_attn_takes(200, 10, 60)
    Y = torch.randn(4, 3 * 130, device=DEV)
    te = torch.randn(60, 130, device=DEV)
    ptr = torch.zeros(5, dtype=torch.int32, device=DEV)
    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    assert ops.san_attn_fwd(Y, te, None, none, None, ptr, none, 2, 0.5, False) is None
    Y, te = torch.randn(4, 3 * 64, device=DEV), torch.randn(60, 64, device=DEV)
    out, s, z = ops.san_attn_fwd(Y, te, None, none, None, ptr, none, 4, 0.5, False)          # E = 0
    assert torch.count_nonzero(out) == 0 and s.shape == (0, 4) and torch.count_nonzero(z) == 0
    out, s, z = ops.san_attn_fwd(Y[:0], te, None, none, None, ptr[:1], none, 4, 0.5, False)  # N = 0
    assert out.shape == (0, 64)


def test_edge_codes_and_flags_in_one_launch():
    mols = GS.GG.molecules(71)
    g = amd.batch([graph.san_graph(m) for m in mols]).to(DEV)
    idx = g.index()
    dims = list(amd.synth.BOND_FEATURE_DIMS)
    codes, real = ops.san_edge_codes(g.edata['feat'], g.edata['real'], idx.perm, dims)
    perm = idx.perm.long()
    want = (g.edata['feat'][perm] * torch.tensor([1, dims[0], dims[0] * dims[1]], device=DEV)).sum(1)
    assert codes.dtype == torch.int32 and real.dtype == torch.uint8
    assert torch.equal(codes.long(), want) and torch.equal(real.long(), g.edata['real'][perm])
    assert int(real.sum()) > 0 and len(set(codes.tolist())) > 3
    same, _ = ops.edge_codes(g.edata['feat'], idx.perm, dims, 64)
    assert torch.equal(codes, same)
    only, none = ops.san_edge_codes(g.edata['feat'], None, idx.perm, dims)
    assert none is None and torch.equal(only, codes)
    ec = san.edge_context(g, dims, True)
    assert torch.equal(ec.codes, codes) and torch.equal(ec.real, real) and ec._lazy == {}
    assert san.edge_context(g.local_copy(), dims, True) is ec


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _model_and_batch(cfg):
    import test_san_cpu as C
    z = load('san.npz')
    return z, C.model_of(z, cfg).to(DEV), C.batch_of(z, cfg, DEV), C


@pytest.mark.parametrize('cfg', sorted(GS.CONFIGS))
def test_model_matches_the_fixture(cfg):
    z, model, g, C = _model_and_batch(cfg)
    C.check_against_fixture(model, g, z, cfg, 'fused')
    assert all(layer.attention.path == 'fused' for layer in model.gnn.layers)


@pytest.mark.parametrize('cfg', ['a', 'b', 'c'])
def test_fused_equals_composed(cfg, monkeypatch):
    z, model, g, C = _model_and_batch(cfg)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(san, 'FUSED_ATTENTION', fused)
        m = copy.deepcopy(model)
        gg = g.local_copy()
        y = m(gg)
        C.loss_of(cfg, y, z).backward()
        assert all(layer.attention.path == ('fused' if fused else 'composed') for layer in m.gnn.layers)
        res[fused] = (y.detach().cpu(), gg.ndata['feat'].detach().cpu(),
                      {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None and p.numel()})
    scale = max(float(v.abs().max()) for v in res[False][2].values())        # (below 1e-4 of it: rounding noise on both sides)
    worst = max(rel_err(res[True][2][k], v) for k, v in res[False][2].items() if float(v.abs().max()) > 1e-4 * scale)
    print(f'san fused vs composed {cfg}: output {rel_err(res[True][0], res[False][0]):.2e}, node state '
          f'{rel_err(res[True][1], res[False][1]):.2e}, worst gradient tensor {worst:.2e}')
    assert rel_err(res[True][0], res[False][0]) < 1e-5 and rel_err(res[True][1], res[False][1]) < 1e-5
    assert set(res[True][2]) == set(res[False][2])
    grads_close(res[True][2], res[False][2], 1e-4, what=f'fused vs composed {cfg} ')


def test_no_edge_wide_tensor():
    """one layer's fused attention, forward + backward, at B = 64, n = 40, H = 64: the peak of allocated memory rises by less than
    one [E, H] fp32 tensor (E = 64 * 40 * 39) over the level before the call"""
    B, n, H, nh = 64, 40, 64, 4
    src, dst, N = R.complete_batch((n,) * B)
    E = src.shape[0]
    assert E == B * n * (n - 1)
    ix = graph.build_index(src, dst, N, [n] * B).to(DEV)
    gen = torch.Generator().manual_seed(4)
    codes = torch.randint(0, 60, (E,), generator=gen).to(torch.int32).to(DEV)
    real = (torch.rand(E, generator=gen) < 0.05).to(torch.uint8).to(DEV)
    order, ptr = ops.code_sorted_index(codes, 60)
    Y = (torch.randn(N, 5 * H, generator=gen) * 0.5).to(DEV)
    te, te2 = (torch.randn(60, H, generator=gen) * 0.5).to(DEV), (torch.randn(60, H, generator=gen) * 0.5).to(DEV)
    grad = torch.randn(N, H, generator=gen).to(DEV)

    def step():
        out, s, z = ops.san_attn_fwd(Y, te, te2, codes, real, ix.in_ptr, ix.src_s, nh, 0.5, True)
        return ops.san_attn_bwd(grad, out, z, s, Y, te, te2, codes, real, ix, order, ptr, nh, 0.5, True)

    step()                                   # the library and its per-stream scratch are in place
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dY, dte, dte2 = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f'san attention fwd + bwd: peak rise {rise / 2 ** 20:.2f} MiB, one [E, H] tensor {E * H * 4 / 2 ** 20:.2f} MiB')
    assert rise < E * H * 4
    assert torch.isfinite(dY).all() and torch.isfinite(dte).all() and torch.isfinite(dte2).all()


def test_training_lowers_the_loss_and_dropout_runs():
    z, model, g, C = _model_and_batch('a')
    opt = amd.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = C.loss_of('a', model(g.local_copy()), z)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(torch.isfinite(p).all() for p in model.parameters())
    torch.manual_seed(0)
    drop = amd.SAN(**dict(GS.CONFIGS['a'], dropout=0.01, in_feat_dropout=0.01)).to(DEV)
    drop.train()
    gg = g.local_copy()
    y = drop(gg)
    y.square().mean().backward()
    assert y.shape == (g.batch_size, 4) and torch.isfinite(y).all() and torch.isfinite(gg.ndata['feat']).all()
    assert all(torch.isfinite(p.grad).all() for p in drop.parameters() if p.grad is not None)
