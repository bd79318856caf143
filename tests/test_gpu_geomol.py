"""GeomolGNNWrapperOGBFeat on the MI355X: the step kernels of csrc/geomol.hip against fp64 torch on a hand-built graph, the module
against the reference's own outputs and gradients (tests/golden/gen_golden_geomol.py), the shared weights through the tape, the
fused step against the composed one, determinism, the checkpoint round trip and a short training run."""
import importlib
import types

import numpy as np
import pytest
import torch

from helpers import amd, grads_close, load, mols_from_npz, rel_err, sd_from_npz, synth

import gen_golden_geomol as GM

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
geomol = importlib.import_module('3dinfomax_amd.geomol')
layers = importlib.import_module('3dinfomax_amd.layers')
tape = importlib.import_module('3dinfomax_amd.tape')
graph_mod = importlib.import_module('3dinfomax_amd.graph')
DEV = torch.device('cuda:0')
EPS = 0.37
U24, U23, U52 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -52


def _synthetic_graph():
    """three graphs in one batch: a single node; 200 nodes with 3400 random directed edges; ten nodes with in-degrees 6, 4, 3, 2, 1,
    1, 0, 2, 3, 0 (two of them without out-edges as well as nodes without in-edges)"""
    rng = np.random.default_rng(12)
    big_src, big_dst = rng.integers(0, 200, 3400) + 1, rng.integers(0, 200, 3400) + 1
    dst = np.array([0] * 6 + [1] * 4 + [2] * 3 + [3] * 2 + [4] + [5] + [7, 7, 8, 8, 8])
    src = np.array([1, 2, 3, 4, 5, 7, 0, 2, 3, 8, 0, 1, 9, 0, 1, 0, 0, 8, 9, 7, 9, 9])
    order = rng.permutation(3400 + len(src))
    src = np.concatenate([big_src, src + 201])[order]
    dst = np.concatenate([big_dst, dst + 201])[order]
    idx = graph_mod.build_index(src, dst, 211, [1, 200, 10])
    indeg, outdeg = np.diff(idx.in_ptr.numpy()), np.diff(idx.out_ptr.numpy())
    assert indeg[201:].tolist() == [6, 4, 3, 2, 1, 1, 0, 2, 3, 0] and indeg[0] == 0 and outdeg[0] == 0 and outdeg[207] == 0
    return idx


def _eighths(shape, gen):
    return torch.randint(-16, 17, shape, generator=gen).float() / 8


class _Case:
    """inputs and the fp64 reference with its per-element sums of absolute values, computed once per H"""
    cache = {}

    def __init__(self, H):
        idx = _synthetic_graph()
        gen = torch.Generator().manual_seed(H)
        N, E = idx.num_nodes, idx.num_edges
        self.idx = idx.to(DEV)
        self.F, self.PQ = _eighths((E, H), gen), _eighths((N, 2 * H), gen)
        self.g = torch.randn(E, H, generator=gen)
        src, dst = idx.src_s.long(), idx.dst_s.long()
        F, PQ, g = self.F.double(), self.PQ.double(), self.g.double()
        pre = F + PQ[src, :H] + PQ[dst, H:]              # exact in fp32 as well: multiples of 1/8 below 8
        self.zero_share = float((pre == 0).double().mean())
        gate = (pre > 0).double()
        self.h = pre * gate
        self.dF = g * gate
        zeros = torch.zeros(N, H, dtype=torch.float64)
        self.dP, self.dP_abs = zeros.index_add(0, src, self.dF), zeros.index_add(0, src, self.dF.abs())
        self.dQ, self.dQ_abs = zeros.index_add(0, dst, self.dF), zeros.index_add(0, dst, self.dF.abs())
        self.indeg = (idx.in_ptr[1:] - idx.in_ptr[:-1]).double()
        self.outdeg = (idx.out_ptr[1:] - idx.out_ptr[:-1]).double()

    @classmethod
    def get(cls, H):
        if H not in cls.cache:
            cls.cache[H] = cls(H)
        return cls.cache[H]


def _run_edge_kernels(c):
    idx = c.idx
    h = ops.geomol_edge_fwd(c.F.to(DEV), c.PQ.to(DEV), idx.src_s, idx.dst_s)
    dF, dPQ = ops.geomol_edge_bwd(c.g.to(DEV), h, idx.in_ptr, idx.out_ptr, idx.out_epos)
    return h, dF, dPQ


@pytest.mark.parametrize('H', [300, 64, 50, 13])
def test_edge_kernels_match_fp64_within_derived_bounds(H):
    """h and dF: no rounding at all for these inputs (the pre-activation is exact, the gate a selection) - bit-equal.  dP / dQ: fp32
    sums in a fixed order, at most deg - 1 roundings of at most 2^-24 of the sum S of the absolute values of the element's terms,
    two spare: (deg + 1) 2^-24 S."""
    c = _Case.get(H)
    assert 0.01 < c.zero_share < 0.05                  # F + P + Q is exactly 0 on about 2.4 % of the elements: gate 0 there
    h, dF, dPQ = _run_edge_kernels(c)
    assert torch.equal(h.cpu().double(), c.h)
    assert torch.equal(dF.cpu().double(), c.dF)
    dP, dQ = dPQ[:, :H].cpu().double(), dPQ[:, H:].cpu().double()
    err_p, bound_p = (dP - c.dP).abs(), (c.outdeg[:, None] + 1) * U24 * c.dP_abs
    err_q, bound_q = (dQ - c.dQ).abs(), (c.indeg[:, None] + 1) * U24 * c.dQ_abs
    print(f'H={H}: dP worst err/bound {float((err_p / bound_p.clamp(min=1e-300)).max()):.3f}')
    print(f'H={H}: dQ worst err/bound {float((err_q / bound_q.clamp(min=1e-300)).max()):.3f}')
    assert (err_p <= bound_p).all() and (err_q <= bound_q).all()
    assert (c.outdeg == 0).sum() >= 2 and (c.indeg == 0).sum() >= 3
    assert torch.count_nonzero(dP[c.outdeg == 0]) == 0 and torch.count_nonzero(dQ[c.indeg == 0]) == 0     # exact zero rows
    assert torch.count_nonzero(dP) > 0 and torch.count_nonzero(dQ) > 0
    again = _run_edge_kernels(c)                       # fixed summation order: the same bits
    for a, b in zip((h, dF, dPQ), again):
        assert torch.equal(a, b)


def _run_residual(a, b, g, eps):
    out = ops.geomol_residual_fwd(a, b, eps)
    da, deps = ops.geomol_residual_bwd(g, a, eps)
    return out, da, deps


# 3422 rows: the edge count of the synthetic graph; 4099 x 300 and 20999 x 13: more workgroups than the backward keeps partials for
# (grid-stride), four floats and one float at a time
@pytest.mark.parametrize('rows, H', [(3422, 300), (3422, 64), (3422, 50), (3422, 13), (211, 50), (4099, 300), (20999, 13)])
def test_residual_kernels_match_fp64_within_derived_bounds(rows, H):
    """forward: the fp32 sum 1 + eps (taken as the kernel takes it), one product, one sum: 3 2^-24 (|(1 + eps) a| + |b|).  da: the
    product and the spare: 2 2^-24 |ref|.  deps: fp64 accumulation of exact products (n 2^-52 S) and one rounding to fp32 (2^-24
    |ref|, taken as 2^-23)."""
    gen = torch.Generator().manual_seed(rows + H)
    a, b, g = (torch.randn(rows, H, generator=gen) for _ in range(3))
    eps = torch.tensor([EPS], dtype=torch.float32, device=DEV)
    scale = float(np.float32(1) + np.float32(EPS))
    out, da, deps = _run_residual(a.to(DEV), b.to(DEV), g.to(DEV), eps)
    ref = scale * a.double() + b.double()
    err = (out.cpu().double() - ref).abs()
    bound = 3 * U24 * ((scale * a.double()).abs() + b.double().abs())
    print(f'rows={rows} H={H}: out worst err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}')
    assert (err <= bound).all()
    ref_da = scale * g.double()
    assert ((da.cpu().double() - ref_da).abs() <= 2 * U24 * ref_da.abs()).all()
    prod = g.double() * a.double()
    ref_eps = float(prod.sum())
    err_eps, bound_eps = abs(float(deps.cpu().double()) - ref_eps), U23 * abs(ref_eps) + rows * H * U52 * float(prod.abs().sum())
    print(f'rows={rows} H={H}: deps err {err_eps:.3e} bound {bound_eps:.3e}')
    assert err_eps <= bound_eps
    for x, y in zip((out, da, deps), _run_residual(a.to(DEV), b.to(DEV), g.to(DEV), eps)):
        assert torch.equal(x, y)


@pytest.mark.parametrize('H', [300, 50, 13])
@pytest.mark.parametrize('N', [1, 5])
def test_empty_edge_set_is_exact(H, N):
    gen = torch.Generator().manual_seed(H + N)
    PQ = torch.randn(N, 2 * H, generator=gen).to(DEV)
    a, b, g = (torch.randn(N, H, generator=gen).to(DEV) for _ in range(3))
    eps = torch.tensor([EPS], dtype=torch.float32, device=DEV)
    zeros = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
    none = torch.empty(0, dtype=torch.int32, device=DEV)
    no_rows = torch.empty(0, H, dtype=torch.float32, device=DEV)
    h = ops.geomol_edge_fwd(no_rows, PQ, none, none)
    assert h.shape == (0, H)
    dF, dPQ = ops.geomol_edge_bwd(no_rows, h, zeros, zeros, none)
    assert dF.shape == (0, H) and dPQ.shape == (N, 2 * H) and torch.count_nonzero(dPQ) == 0
    out, da, deps = _run_residual(a, b, g, eps)
    assert torch.equal(out, (1 + eps) * a + b)
    assert torch.equal(da, (1 + eps) * g)
    ref = (g.double() * a.double()).sum().item()
    assert abs(deps.item() - ref) <= U23 * abs(ref) + N * H * U52 * (g.double() * a.double()).abs().sum().item()
    out0, da0, deps0 = _run_residual(no_rows, no_rows, no_rows, eps)         # the edge residual of a batch without edges
    assert out0.shape == (0, H) and da0.shape == (0, H) and deps0.item() == 0.0


# ---- the module ---------------------------------------------------------------------------------------------------------------
def _graph(mols):
    return amd.batch([amd.bond_graph(m) for m in mols]).to(DEV)


def _model(z, cfg, **override):
    model = amd.GeomolGNNWrapperOGBFeat(**dict(GM.CONFIGS[cfg], **override))
    model.load_state_dict(sd_from_npz(z, f'{cfg}/sd'), strict=True)
    return model.to(DEV)


def _loss(cfg, y, z):
    return GM.loss_of(cfg, y, torch.from_numpy(z[f'{cfg}/target']).to(DEV))


def _param_grads(model):
    return {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}


def _step(z, cfg, train=True):
    """-> model, output, node representation, edge representation, loss, gradients of one forward + backward on the fixture's batch"""
    model = _model(z, cfg)
    model.train(train)
    feat = []
    hook = model.node_gnn.register_forward_hook(lambda mod, args, out: feat.append([t.detach().clone() for t in out]))
    y = model(_graph(mols_from_npz(z, f'{cfg}/mol')))
    hook.remove()
    loss = _loss(cfg, y, z)
    loss.backward()
    return model, y.detach(), feat[0][0], feat[0][1], loss.item(), _param_grads(model)


def _check_grads_against_fixture(z, cfg, got, keys=None):
    ref = sd_from_npz(z, f'{cfg}/grad')
    scale = max(float(v.abs().max()) for v in ref.values())
    for k, v in ref.items():
        if keys is not None and k not in keys:
            continue
        rtol = max(1e-3, 4 * float(z[f'{cfg}/ref_err/grad/{k}']))
        err = float((got[k].double() - v.double()).abs().max())
        print(f'{cfg}: grad {k}: err {err:.3e} max {float(v.abs().max()):.3e} rtol {rtol:.1e} scale {scale:.3e}')
    for k, v in ref.items():
        if keys is not None and k not in keys:
            continue
        rtol = max(1e-3, 4 * float(z[f'{cfg}/ref_err/grad/{k}']))
        # one tensor per call (its own rtol); the '_scale' entry keeps grads_close's absolute floor tied to the largest gradient of
        # the whole set, as in a call on the whole dict
        grads_close({k: got[k], '_scale': torch.tensor([scale])}, {k: v, '_scale': torch.tensor([scale])}, rtol, what=f'{cfg}: ')


@pytest.mark.parametrize('cfg', sorted(GM.CONFIGS))
def test_module_matches_reference_fixture(cfg):
    """Gradients: rtol = max(1e-3, 4 x the fp32 reference's own error against its fp64 run, per tensor) - two fp32 implementations
    each as far from fp64 as the reference is, times two for the different summation order."""
    z = load('geomol.npz')
    model, y, feat, efeat, loss, got = _step(z, cfg, cfg != 'd')
    assert y.shape == z[f'{cfg}/out'].shape
    print(f'{cfg}: rel_err out {rel_err(y.cpu(), z[f"{cfg}/out"]):.2e} feat {rel_err(feat.cpu(), z[f"{cfg}/feat"]):.2e} '
          f'efeat {rel_err(efeat.cpu(), z[f"{cfg}/efeat"]):.2e}; fixture ref_err out {float(z[f"{cfg}/ref_err/out"]):.2e}')
    assert rel_err(y.cpu(), z[f'{cfg}/out']) < 1e-4
    assert rel_err(feat.cpu(), z[f'{cfg}/feat']) < 1e-4
    assert rel_err(efeat.cpu(), z[f'{cfg}/efeat']) < 1e-4          # the caller's edge order
    assert abs(loss - float(z[f'{cfg}/loss'])) < 1e-4 * abs(float(z[f'{cfg}/loss']))
    assert set(got) == set(sd_from_npz(z, f'{cfg}/grad')) == {k for k, _ in model.named_parameters()}
    _check_grads_against_fixture(z, cfg, got)
    sd = model.state_dict()
    bufs = sd_from_npz(z, f'{cfg}/buf_after')
    assert bool(bufs) == GM.CONFIGS[cfg]['readout_batchnorm']
    for k, v in bufs.items():
        if 'running' in k:
            assert rel_err(sd[k].cpu(), v) < 1e-5, k
        else:
            assert int(sd[k]) == int(v), k


def test_shared_weights_collect_every_step_through_the_tape():
    """every parameter of `update` is used depth = 3 times.  Its gradient matches the fixture; and the same three steps taken by
    hand on a depth-1 model under plain torch autograd (no tape: autograd sums the contributions itself) give the tape's gradients,
    which a tape that overwrote a contribution instead of summing it would not."""
    z = load('geomol.npz')
    model, y3, _, _, _, got = _step(z, 'a')
    shared = {k for k in got if k.startswith('node_gnn.update.')}
    assert len(shared) == 24 and 'node_gnn.update.edge_eps' in shared and 'node_gnn.update.node_eps' in shared
    _check_grads_against_fixture(z, 'a', got, keys=shared)

    one = _model(z, 'a', depth=1).train()
    g = _graph(mols_from_npz(z, 'a/mol'))
    idx = g.index()
    assert tape.active() is None
    x, e = one.node_gnn(g, g.ndata['feat'], g.edata['feat'])                      # init + the first step
    assert x.grad_fn is not None and e.grad_fn is not None                      # plain autograd nodes
    e = geomol._GatherRowsFn.apply(e, idx.perm, idx.inv_perm)                    # back to the destination-sorted order
    for _ in range(2):
        x, e = one.node_gnn.update(x, idx, e)
    y = one.output(layers.ReadoutFn.apply(x, idx, ops.agg_codes(['mean'])))
    assert rel_err(y.detach().cpu(), y3.cpu()) < 1e-6
    _loss('a', y, z).backward()
    by_hand = _param_grads(one)
    assert set(by_hand) == set(got)
    for k in sorted(got):
        print(f'by hand vs tape: {k}: rel_err {rel_err(by_hand[k], got[k]):.2e}')
    for k in got:
        assert rel_err(by_hand[k], got[k]) < 1e-5, k


@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_fused_step_matches_composed(cfg, monkeypatch):
    """FUSED_STEP True against False.  The two paths compute the same fp32 terms; the order of the three-way add, of the sums inside a
    neighbourhood and the place of node_mlp_1's last Linear (N rows after the sum against E rows before it) differ, each within the
    per-element bounds of the kernel tests; propagated loosely through three steps: rel_err < 1e-5.  The gradient of
    node_mlp_1.layers.<last>.bias is the in-degree-weighted column sum on one side and a plain column sum on the other."""
    z = load('geomol.npz')
    _, y1, f1, e1, _, g1 = _step(z, cfg)
    monkeypatch.setattr(geomol, 'FUSED_STEP', False)
    _, y0, f0, e0, _, g0 = _step(z, cfg)
    print(f'{cfg}: fused vs composed rel_err out {rel_err(y1.cpu(), y0.cpu()):.2e} feat {rel_err(f1.cpu(), f0.cpu()):.2e} '
          f'efeat {rel_err(e1.cpu(), e0.cpu()):.2e}')
    assert rel_err(y1.cpu(), y0.cpu()) < 1e-5 and rel_err(f1.cpu(), f0.cpu()) < 1e-5 and rel_err(e1.cpu(), e0.cpu()) < 1e-5
    assert set(g1) == set(g0) and 'node_gnn.update.node_model.node_mlp_1.layers.4.bias' in g1
    grads_close(g1, g0, 1e-5, what=f'{cfg} fused vs composed: ')


def test_two_identical_steps_are_bit_identical():
    z = load('geomol.npz')
    m0, y0, f0, e0, _, g0 = _step(z, 'a')
    m1, y1, f1, e1, _, g1 = _step(z, 'a')
    assert torch.equal(y0, y1) and torch.equal(f0, f1) and torch.equal(e0, e1)
    assert set(g0) == set(g1) == {k for k, _ in m0.named_parameters()}
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for (k, v), w in zip(m0.state_dict().items(), m1.state_dict().values()):
        assert torch.equal(v, w), k


def test_checkpoint_round_trip_is_bit_identical_and_pyg_input_is_the_same_batch():
    z = load('geomol.npz')
    model, *_ = _step(z, 'a')                       # one training forward: running statistics moved
    model.eval()
    mols = mols_from_npz(z, 'a/mol')
    g = _graph(mols)
    sd = {k: v.cpu().clone() for k, v in model.state_dict().items()}
    assert list(sd) == list(sd_from_npz(z, 'a/sd'))
    fresh = amd.GeomolGNNWrapperOGBFeat(**GM.CONFIGS['a'])
    fresh.load_state_dict(sd, strict=True)
    fresh.to(DEV).eval()
    d = GM.data_of(mols)
    data = types.SimpleNamespace(z=d.z.to(DEV), edge_index=d.edge_index.to(DEV), edge_attr=d.edge_attr.to(DEV), batch=d.batch.to(DEV))
    with torch.no_grad():
        a, b, c = model(g), fresh(g), fresh(data)
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)


def test_thirty_adam_steps_lower_the_loss_and_move_every_parameter():
    mols = synth.make_dataset(64, seed=8)
    g = _graph(mols)
    torch.manual_seed(2)
    model = amd.GeomolGNNWrapperOGBFeat(hidden_dim=64, target_dim=3, depth=3, n_layers=2).to(DEV).train()
    target = torch.randn(64, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = amd.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.L1Loss()(model(g), target)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    # The Linear bias directly in front of the readout's training-mode BatchNorm has an analytically zero gradient (the BatchNorm
    # removes the shift): the fused Linear + BatchNorm backward writes exactly 0 for it, so Adam leaves it where it is.  Every
    # OTHER parameter must have moved - edge_eps and node_eps included.
    feeds_bn = {'output.fully_connected.0.linear.bias'}
    assert feeds_bn < set(before)
    for k, p in model.named_parameters():
        assert torch.isfinite(p).all(), k
        if k not in feeds_bn:
            assert not torch.equal(p.detach(), before[k]), k
    assert 'node_gnn.update.edge_eps' in before and 'node_gnn.update.node_eps' in before
