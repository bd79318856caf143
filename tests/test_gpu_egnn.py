"""EGNN on the MI355X: the gate-and-reduce kernels of csrc/egnn.hip against fp64 torch on a hand-built destination-sorted batch, the
widths the kernels leave to the composed chain, the fused step against the composed one, the module against the reference's own outputs
and gradients (tests/golden/gen_golden_egnn.py), determinism, the checkpoint round trip and a short training run."""
import importlib
import math

import numpy as np
import pytest
import torch

from helpers import amd, grads_close, load, mols_from_npz, rel_err, sd_from_npz

import gen_golden_egnn as GE

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
egnn = importlib.import_module('3dinfomax_amd.egnn')
graph_mod = importlib.import_module('3dinfomax_amd.graph')
DEV = torch.device('cuda:0')
U24 = 2.0 ** -24
DEGREES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 0, 203, 0]          # node 0 and the last node have no in-edges
K_SIGMOID = 6            # exp within 2 ulp (4 half-ulps), the addition 1 + e, the division
MAX_H = 512


def _index():
    rng = np.random.default_rng(5)
    dst = np.repeat(np.arange(len(DEGREES)), DEGREES)
    src = rng.integers(0, len(DEGREES), dst.shape[0])
    order = rng.permutation(dst.shape[0])
    idx = graph_mod.build_index(src[order], dst[order], len(DEGREES), [len(DEGREES)])
    indeg = np.diff(idx.in_ptr.numpy())
    assert indeg.tolist() == DEGREES and indeg[0] == 0 and indeg[-1] == 0
    assert {0, 1, 2, 3, 4, 5, 63, 64, 65} <= set(indeg.tolist()) and 190 <= indeg.max() <= 210
    return idx


def _dot_roundings(H, fused):
    """roundings a product of a dot over H passes through, one spare.  Kernel (csrc/egnn.hip): 4 R products per lane (R = 2 above 256
    columns) added in order, log2(G) xor-shuffle steps over the G lanes of a row (G the power of two with 4 G >= H, 8 <= G <= 64),
    the bias.  Composed (csrc/edge.hip, one lane per edge): H additions in order behind the product."""
    if not fused:
        return H + 2
    R = 2 if H > 256 else 1
    G = min(64, max(8, 1 << max(0, math.ceil(math.log2(H / 4)))))
    return 4 * R + int(math.log2(G)) + 1 + 1


class _Case:
    """inputs, the fp64 reference and the per-element error bounds, computed once per (H, mean)

    Counting (u = 2^-24, first order, one spare rounding in every count):
      z_j = <ws, m_j> + bs:  |dz_j| <= K u A_j, A_j = sum_c |ws_c m_jc| + |bs|, K = _dot_roundings(H).
      w_j = sigmoid(z_j):    sigma' <= 1/4 carries dz_j, the evaluation 1 / (1 + exp(-z)) adds K_SIGMOID relative roundings:
                             dw_j = (K A_j / 4 + K_SIGMOID w_j) u.
      u_vc = h_vc + s sum_j m_jc w_j (s = 1 or 1 / deg):  every product m_jc w_j carries |m_jc| dw_j and one rounding; a term then
                             passes at most deg additions inside the wave (ceil(deg / groups) in its lane group, 3 across the groups),
                             the division of the mean and the addition of h: deg + 5 roundings on |h_vc| + s sum_j |m_jc| w_j.
      g = gu_v s (one rounding), D_j = <g, m_j>: dD_j = (K + 1) u sum_c |g_c m_jc|.
      gg_j = D_j w_j (1 - w_j):  |d(w (1 - w))| <= |1 - 2 w| dw <= dw, three roundings:  dgg_j = dD_j w_j (1 - w_j) + |D_j| dw_j + 4 u |gg_j|.
      gm_jc = g_c w_j + gg_j ws_c:  |g_c| dw_j + |ws_c| dgg_j + 4 u (|g_c| w_j + |gg_j ws_c|).
      gws_c = sum_j gg_j m_jc, gbs = sum_j gg_j:  sum_j |m_jc| dgg_j (sum_j dgg_j) and n u sum_j |gg_j m_jc| (|gg_j|); a term passes
                             the additions of its node's wave and the column sum over the N partial rows: n = max deg + N + 5.  Composed:
                             one column sum over the E edges, n = E + 2."""
    cache = {}

    def __init__(self, H, mean, fused=True):
        idx = _index()
        gen = torch.Generator().manual_seed(1000 * int(mean) + H)
        N, E = idx.num_nodes, idx.num_edges
        self.H, self.mean, self.idx = H, mean, idx.to(DEV)
        self.m, self.h, self.gu = torch.randn(E, H, generator=gen), torch.randn(N, H, generator=gen), torch.randn(N, H, generator=gen)
        self.ws = torch.randn(1, H, generator=gen) * (1.5 / math.sqrt(H))
        self.bs = torch.tensor([0.3])
        m, h, gu, ws, bs = (t.double() for t in (self.m, self.h, self.gu, self.ws.view(-1), self.bs))
        dst = idx.dst_s.long()
        deg = torch.tensor(DEGREES, dtype=torch.float64)
        s = (1 / deg.clamp(min=1)) if mean else torch.ones(N, dtype=torch.float64)
        K = _dot_roundings(H, fused)
        zero = torch.zeros(N, H, dtype=torch.float64)
        # forward
        w = torch.sigmoid(m @ ws + bs)
        A = (m * ws).abs().sum(1) + bs.abs()
        dw = (K * A / 4 + K_SIGMOID * w) * U24
        self.w, self.dw = w, dw
        T = zero.index_add(0, dst, m * w[:, None])
        T_abs = zero.index_add(0, dst, m.abs() * w[:, None])
        self.u = h + s[:, None] * T
        self.u_bound = s[:, None] * zero.index_add(0, dst, m.abs() * (dw + U24 * w)[:, None]) \
            + (deg[:, None] + 5) * U24 * (h.abs() + s[:, None] * T_abs)
        # backward
        g = (gu * s[:, None])[dst]
        D = (g * m).sum(1)
        p = w * (1 - w)
        gg = D * p
        dgg = (K + 1) * U24 * (g * m).abs().sum(1) * p + D.abs() * dw + 4 * U24 * gg.abs()
        self.gm = g * w[:, None] + gg[:, None] * ws
        self.gm_bound = g.abs() * dw[:, None] + ws.abs() * dgg[:, None] + 4 * U24 * (g.abs() * w[:, None] + (gg[:, None] * ws).abs())
        n = (max(DEGREES) + N + 5) if fused else (E + 2)
        self.gws = (gg[:, None] * m).sum(0)
        self.gws_bound = (m.abs() * dgg[:, None]).sum(0) + n * U24 * (gg[:, None] * m).abs().sum(0)
        self.gbs = gg.sum()
        self.gbs_bound = dgg.sum() + n * U24 * gg.abs().sum()

    @classmethod
    def get(cls, H, mean, fused=True):
        key = (H, mean, fused)
        if key not in cls.cache:
            cls.cache[key] = cls(H, mean, fused)
        return cls.cache[key]


def _run_function(c):
    """GateReduceFn under torch autograd -> u, gm, gws, gbs, gh"""
    m, ws, bs, h = (t.to(DEV).requires_grad_(True) for t in (c.m, c.ws, c.bs, c.h))
    u = egnn.GateReduceFn.apply(m, ws, bs, h, c.idx, c.mean)
    u.backward(c.gu.to(DEV))
    return u.detach(), m.grad, ws.grad.view(-1), bs.grad, h.grad


def _check(c, u, gm, gws, gbs, what):
    worst = {}
    for name, got, ref, bound in (('u', u, c.u, c.u_bound), ('gm', gm, c.gm, c.gm_bound), ('gws', gws, c.gws, c.gws_bound),
                                  ('gbs', gbs.view(()), c.gbs, c.gbs_bound)):
        err = (got.cpu().double() - ref).abs()
        worst[name] = float((err / bound.clamp(min=1e-300)).max())
    print(f'{what} H={c.H} mean={c.mean}: worst err / bound ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= 1.0, (name, v)


@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('H', [4, 20, 64, 128, 132, 260, MAX_H])
def test_gate_reduce_kernels_match_fp64_within_derived_bounds(H, mean):
    """The bounds are the fp64 reference's per-element sums of absolute values times 2^-24 times the operation counts of the kernels,
    written out in _Case's docstring; 64, 260: the two lane layouts the issue's widths leave out (16 lanes per row; a second, partly
    empty group of four columns per lane)."""
    assert ops.gate_reduce_max_feat() == MAX_H
    c = _Case.get(H, mean)
    idx = c.idx
    m, ws, bs, h, gu = (t.to(DEV) for t in (c.m, c.ws, c.bs, c.h, c.gu))
    res = ops.gate_reduce_fwd(m, ws, bs, idx.in_ptr, h, mean)
    assert res is not None, 'the kernel must take this width'
    u, w = res
    err_w = (w.cpu().double() - c.w).abs()
    print(f'H={H} mean={mean}: w worst err / bound {float((err_w / c.dw).max()):.3f}')
    assert (err_w <= c.dw).all()
    gm, gws, gbs = ops.gate_reduce_bwd(gu, m, w, ws, idx.in_ptr, mean)
    _check(c, u, gm, gws, gbs, 'kernels')
    empty = [v for v, d in enumerate(DEGREES) if d == 0]
    assert torch.equal(u[empty].cpu(), c.h[empty])          # no in-edges: u = h, bit for bit
    # the same bits on a second call, and through the autograd Function (whose dL/dh is dL/du itself)
    u2, w2 = ops.gate_reduce_fwd(m, ws, bs, idx.in_ptr, h, mean)
    again = ops.gate_reduce_bwd(gu, m, w2, ws, idx.in_ptr, mean)
    assert torch.equal(u, u2) and torch.equal(w, w2) and all(torch.equal(a, b) for a, b in zip((gm, gws, gbs), again))
    fu, fgm, fgws, fgbs, fgh = _run_function(c)
    assert torch.equal(fu, u) and torch.equal(fgm, gm) and torch.equal(fgws, gws) and torch.equal(fgbs, gbs)
    assert torch.equal(fgh.cpu(), c.gu)


@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('H', [6, MAX_H + 4])
def test_uncovered_widths_take_the_composed_chain(H, mean):
    """H % 4 != 0 and H above the kernels' bound: I3D_NOT_TAKEN, and GateReduceFn runs soft_edge -> segment_sum -> add.  The same
    bounds with the composed kernels' counts: a dot product added in order by one lane (H + 2), one column sum over the edges."""
    c = _Case.get(H, mean, fused=False)
    m, ws, bs, h = (t.to(DEV) for t in (c.m, c.ws, c.bs, c.h))
    assert ops.gate_reduce_fwd(m, ws, bs, c.idx.in_ptr, h, mean) is None
    assert ops.gate_reduce_bwd(c.gu.to(DEV), m, torch.zeros(m.shape[0], device=DEV), ws, c.idx.in_ptr, mean) is None
    u, gm, gws, gbs, gh = _run_function(c)
    _check(c, u, gm, gws, gbs, 'composed')
    assert torch.equal(gh.cpu(), c.gu)


def _graph(z, cfg):
    g = amd.batch([amd.complete_graph(m, coordinates=True) for m in mols_from_npz(z, f'{cfg}/mol')])
    g.ndata['feat'] = torch.from_numpy(z[f'{cfg}/feat_in'].copy())
    return g.to(DEV)


def _model(z, cfg):
    model = amd.EGNN(**GE.CONFIGS[cfg])
    model.load_state_dict(sd_from_npz(z, f'{cfg}/sd'), strict=True)
    return model.to(DEV)


def _step(z, cfg, train=True):
    """-> model, output, final node features, loss, gradients of one forward + backward on the fixture's batch"""
    model = _model(z, cfg)
    model.train(train)
    g = _graph(z, cfg)
    y = model(g)
    loss = (y ** 2).mean()
    loss.backward()
    return model, y.detach(), g.ndata['feat'].detach(), loss.item(), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}


@pytest.mark.parametrize('cfg', sorted(GE.CONFIGS))
def test_module_matches_reference_fixture(cfg):
    """Gradients: rtol = max(1e-3, 4 x the fp32 reference's own error against its fp64 run, per tensor) - two fp32 implementations
    each as far from fp64 as the reference is, times two for the different summation order."""
    z = load('egnn.npz')
    model, y, feat, loss, got = _step(z, cfg, cfg != 'd')
    assert y.shape == z[f'{cfg}/out'].shape
    print(f'{cfg}: out rel_err {rel_err(y.cpu(), z[f"{cfg}/out"]):.2e} feat rel_err {rel_err(feat.cpu(), z[f"{cfg}/feat"]):.2e} '
          f'loss {loss:.8f} ref {float(z[f"{cfg}/loss"]):.8f}')
    ref = sd_from_npz(z, f'{cfg}/grad')
    assert set(got) == set(ref)
    scale = max(float(v.abs().max()) for v in ref.values())
    for k, v in ref.items():
        rtol = max(1e-3, 4 * float(z[f'{cfg}/ref_err/grad/{k}']))
        err = float((got[k].double() - v.double()).abs().max())
        print(f'{cfg}: grad {k}: err {err:.3e} max {float(v.abs().max()):.3e} rtol {rtol:.1e} scale {scale:.3e}')
    assert rel_err(y.cpu(), z[f'{cfg}/out']) < 1e-4
    assert rel_err(feat.cpu(), z[f'{cfg}/feat']) < 1e-4
    assert abs(loss - float(z[f'{cfg}/loss'])) < 1e-4 * abs(float(z[f'{cfg}/loss']))
    for k, v in ref.items():
        rtol = max(1e-3, 4 * float(z[f'{cfg}/ref_err/grad/{k}']))
        # one tensor per call (its own rtol); the '_scale' entry keeps grads_close's absolute floor tied to the largest gradient of
        # the whole set, as in a call on the whole dict
        grads_close({k: got[k], '_scale': torch.tensor([scale])}, {k: v, '_scale': torch.tensor([scale])}, rtol, what=f'{cfg}: ')
    sd = model.state_dict()
    for k, v in sd_from_npz(z, f'{cfg}/buf_after').items():
        if 'running' in k:
            assert rel_err(sd[k].cpu(), v) < 1e-5, k
        else:
            assert int(sd[k]) == int(v), k


def test_fused_gate_reduce_matches_composed(monkeypatch):
    """fused_gate_reduce True against False, same weights.  Both compute the same fp32 terms; the order of the dot product over H
    and of the sum inside a neighbourhood differs: the project's figures for GIN's fused-vs-composed check."""
    z = load('egnn.npz')
    _, y1, f1, l1, g1 = _step(z, 'a')
    monkeypatch.setattr(egnn.EGCLayer, 'fused_gate_reduce', False)
    _, y0, f0, l0, g0 = _step(z, 'a')
    print(f'fused vs composed: out {rel_err(y1.cpu(), y0.cpu()):.2e} feat {rel_err(f1.cpu(), f0.cpu()):.2e}')
    assert rel_err(y1.cpu(), y0.cpu()) < 1e-5 and rel_err(f1.cpu(), f0.cpu()) < 1e-5
    assert set(g1) == set(g0)
    grads_close(g1, g0, 1e-5, what='a fused vs composed: ')


def test_two_identical_steps_are_bit_identical():
    z = load('egnn.npz')
    m0, y0, f0, _, g0 = _step(z, 'a')
    m1, y1, f1, _, g1 = _step(z, 'a')
    assert torch.equal(y0, y1) and torch.equal(f0, f1)
    assert set(g0) == set(g1) == {k for k, _ in m0.named_parameters()}
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for (k, v), w in zip(m0.state_dict().items(), m1.state_dict().values()):
        assert torch.equal(v, w), k


def test_checkpoint_round_trip_is_bit_identical():
    z = load('egnn.npz')
    model, *_ = _step(z, 'a')                       # one training forward: running statistics moved
    model.eval()
    sd = {k: v.cpu().clone() for k, v in model.state_dict().items()}
    assert list(sd) == list(sd_from_npz(z, 'a/sd'))
    fresh = amd.EGNN(**GE.CONFIGS['a'])
    fresh.load_state_dict(sd, strict=True)
    fresh.to(DEV).eval()
    with torch.no_grad():
        a, b = model(_graph(z, 'a')), fresh(_graph(z, 'a'))
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_thirty_adam_steps_lower_the_loss():
    z = load('egnn.npz')
    model = _model(z, 'a').train()
    g = _graph(z, 'a')
    target = torch.randn(7, 8, generator=torch.Generator().manual_seed(9)).to(DEV)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = amd.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = ((model(g.local_copy()) - target) ** 2).mean()          # the forward overwrites ndata['feat']
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    for l in range(3):      # the gate's parameters get a gradient through the fused step
        for k in (f'mp_layers.{l}.soft_edge_network.weight', f'mp_layers.{l}.soft_edge_network.bias'):
            assert not torch.equal(dict(model.named_parameters())[k].detach(), before[k]), k
