"""OGBGNN (GIN + virtual node) on the MI355X: the message kernels of csrc/gin.hip against fp64 torch on a hand-built graph, the
fused message step against the composed one, the module against the reference's own outputs and gradients
(tests/golden/gen_golden_gin.py), determinism, the checkpoint round trip and a short training run."""
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, grads_close, load, mols_from_npz, rel_err, sd_from_npz, synth

import gen_golden_gin as GG

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
gin = importlib.import_module('3dinfomax_amd.gin')
graph_mod = importlib.import_module('3dinfomax_amd.graph')
DEV = torch.device('cuda:0')
V = 60
ABSENT, HEAVY = 41, 7
EPS = 0.37
U24, U23, U52 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -52


def _synthetic_graph():
    """three graphs in one batch: a single node; 200 nodes with 3400 random directed edges, 3100 of them of code HEAVY (more than any
    reduction chunk), the rest spread over every code but ABSENT; ten nodes with in-degrees 6, 4, 3, 2, 1, 1, 0, 2, 3, 0"""
    rng = np.random.default_rng(12)
    big_src, big_dst = rng.integers(0, 200, 3400) + 1, rng.integers(0, 200, 3400) + 1
    others = [c for c in range(V) if c not in (ABSENT, HEAVY)]
    big_code = np.full(3400, HEAVY)
    big_code[rng.permutation(3400)[:300]] = [others[i % len(others)] for i in range(300)]
    dst = np.array([0] * 6 + [1] * 4 + [2] * 3 + [3] * 2 + [4] + [5] + [7, 7, 8, 8, 8])
    src = np.array([1, 2, 3, 4, 5, 7, 0, 2, 3, 8, 0, 1, 9, 0, 1, 0, 0, 8, 9, 7, 9, 9])
    small_code = rng.choice(others, size=len(src))
    order = rng.permutation(3400 + len(src))
    src = np.concatenate([big_src, src + 201])[order]
    dst = np.concatenate([big_dst, dst + 201])[order]
    code = np.concatenate([big_code, small_code])[order]
    idx = graph_mod.build_index(src, dst, 211, [1, 200, 10])
    codes_s = torch.from_numpy(code[idx.perm.numpy()].astype(np.int32))
    indeg = np.diff(idx.in_ptr.numpy())
    assert {0, 1, 2, 3, 4, 6} <= set(indeg.tolist()) and indeg[0] == 0
    counts = np.bincount(code, minlength=V)
    assert counts[ABSENT] == 0 and counts[HEAVY] >= 3000 and (np.delete(counts, ABSENT) > 0).all()
    return idx, codes_s


def _eighths(shape, gen):
    return torch.randint(-16, 17, shape, generator=gen).float() / 8


class _Case:
    """inputs and the fp64 reference with its per-element sums of absolute values, computed once per (H, vn)"""
    cache = {}

    def __init__(self, H, with_vn):
        idx, codes_s = _synthetic_graph()
        gen = torch.Generator().manual_seed(H + int(with_vn))
        N, B = idx.num_nodes, idx.num_graphs
        self.idx, self.codes = idx.to(DEV), codes_s.to(DEV)
        self.x, self.T = _eighths((N, H), gen), _eighths((V, H), gen)
        self.vn = _eighths((B, H), gen) if with_vn else None
        node_graph = torch.repeat_interleave(torch.arange(B), torch.tensor([1, 200, 10]))
        self.h = self.x - self.vn[node_graph] if with_vn else self.x          # exact: multiples of 1/8 below 4
        self.g = torch.randn(N, H, generator=gen)
        src, dst, code = idx.src_s.long(), idx.dst_s.long(), codes_s.long()
        x, T, g = self.x.double(), self.T.double(), self.g.double()
        scale = float(np.float32(1) + np.float32(EPS))         # the kernel's 1 + eps is an fp32 sum: one of the counted roundings
        pre = x[src] + T[code]                          # exact in fp32 as well: multiples of 1/8 below 4
        self.zero_share = float((pre == 0).double().mean())
        gate = (pre > 0).double()
        msg = pre * gate
        self.z = (scale * x).index_add(0, dst, msg)
        self.z_abs = (scale * x).abs().index_add(0, dst, msg.abs())
        back = g[dst] * gate
        self.dx = (scale * g).index_add(0, src, back)
        self.dx_abs = (scale * g).abs().index_add(0, src, back.abs())
        self.dT = torch.zeros(V, H, dtype=torch.float64).index_add(0, code, back)
        self.dT_abs = torch.zeros(V, H, dtype=torch.float64).index_add(0, code, back.abs())
        self.n_code = torch.bincount(code, minlength=V).double()
        self.deps, self.deps_abs = (g * x).sum(), (g * x).abs().sum()
        self.indeg = (idx.in_ptr[1:] - idx.in_ptr[:-1]).double()
        self.outdeg = (idx.out_ptr[1:] - idx.out_ptr[:-1]).double()

    @classmethod
    def get(cls, H, with_vn):
        key = (H, with_vn)
        if key not in cls.cache:
            cls.cache[key] = cls(H, with_vn)
        return cls.cache[key]


def _run_kernels(c):
    idx = c.idx
    eps = torch.tensor([EPS], dtype=torch.float32, device=DEV)
    order, ptr = ops.code_sorted_index(c.codes, V)
    x, z = ops.gin_conv_fwd(c.h.to(DEV), c.vn.to(DEV) if c.vn is not None else None, idx.graph_ptr, idx.num_graphs, c.T.to(DEV),
                            c.codes, idx.in_ptr, idx.src_s, eps)
    dx, dT, deps = ops.gin_conv_bwd(c.g.to(DEV), x, c.T.to(DEV), c.codes, idx.src_s, idx.dst_s, idx.out_ptr, idx.out_epos, order, ptr,
                                    eps)
    return x, z, dx, dT, deps


@pytest.mark.parametrize('with_vn', [True, False], ids=['vn', 'plain'])
@pytest.mark.parametrize('H', [300, 64, 13])
def test_message_kernels_match_fp64_within_derived_bounds(H, with_vn):
    """z and dx: fp32 sums in a fixed order - at most indeg + 2 (outdeg + 2) roundings, each at most 2^-24 of the sum S of the
    absolute values of the element's terms, one spare: (deg + 3) 2^-24 S.  dT and deps: fp64 accumulation (n 2^-52 S) and one
    rounding to fp32 (2^-24 |ref|, taken as 2^-23)."""
    c = _Case.get(H, with_vn)
    assert 0.01 < c.zero_share < 0.06                  # x[src] + T[code] is exactly 0 on about 1 / 33 of the elements: gate 0 there
    x, z, dx, dT, deps = _run_kernels(c)
    assert torch.equal(x.cpu(), c.x)                   # h + vn is exact for these values
    err_z = (z.cpu().double() - c.z).abs()
    bound_z = (c.indeg[:, None] + 3) * U24 * c.z_abs
    print(f'H={H} vn={with_vn}: z worst err/bound {float((err_z / bound_z.clamp(min=1e-300)).max()):.3f}')
    assert (err_z <= bound_z).all()
    err_dx = (dx.cpu().double() - c.dx).abs()
    bound_dx = (c.outdeg[:, None] + 3) * U24 * c.dx_abs
    print(f'H={H} vn={with_vn}: dx worst err/bound {float((err_dx / bound_dx.clamp(min=1e-300)).max()):.3f}')
    assert (err_dx <= bound_dx).all()
    err_dT = (dT.cpu().double() - c.dT).abs()
    bound_dT = U23 * c.dT.abs() + c.n_code[:, None] * U52 * c.dT_abs
    print(f'H={H} vn={with_vn}: dT worst err/bound {float((err_dT / bound_dT.clamp(min=1e-300)).max()):.3f}')
    assert (err_dT <= bound_dT).all()
    assert torch.count_nonzero(dT[ABSENT]) == 0        # a code without edges: exactly zero
    assert torch.count_nonzero(dT[HEAVY]) > 0
    err_eps = abs(float(deps.cpu().double()) - float(c.deps))
    bound_eps = U23 * abs(float(c.deps)) + c.x.numel() * U52 * float(c.deps_abs)
    print(f'H={H} vn={with_vn}: deps err {err_eps:.3e} bound {bound_eps:.3e}')
    assert err_eps <= bound_eps
    again = _run_kernels(c)                            # fixed summation order: the same bits
    for a, b in zip((x, z, dx, dT, deps), again):
        assert torch.equal(a, b)


@pytest.mark.parametrize('H', [300, 13])
@pytest.mark.parametrize('N', [1, 5])
def test_empty_edge_set_is_exact(H, N):
    gen = torch.Generator().manual_seed(H + N)
    x, T, g = torch.randn(N, H, generator=gen).to(DEV), torch.randn(V, H, generator=gen).to(DEV), torch.randn(N, H, generator=gen).to(DEV)
    eps = torch.tensor([EPS], dtype=torch.float32, device=DEV)
    zeros = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    order, ptr = ops.code_sorted_index(empty, V)
    same, z = ops.gin_conv_fwd(x, None, None, 0, T, empty, zeros, empty, eps)
    assert same is x
    assert torch.equal(z, (1 + eps) * x)
    dx, dT, deps = ops.gin_conv_bwd(g, x, T, empty, empty, empty, zeros, empty, order, ptr, eps)
    assert torch.equal(dx, (1 + eps) * g)
    assert torch.count_nonzero(dT) == 0
    ref = (g.double() * x.double()).sum().item()
    assert abs(deps.item() - ref) <= U23 * abs(ref) + N * H * U52 * (g.double() * x.double()).abs().sum().item()


def _graph(mols):
    return amd.batch([amd.bond_graph(m) for m in mols]).to(DEV)


def _model(z, cfg):
    model = amd.OGBGNN(**GG.CONFIGS[cfg])
    model.load_state_dict(sd_from_npz(z, f'{cfg}/sd'), strict=True)
    return model.to(DEV)


def _loss(cfg, y, z):
    if cfg in ('a', 'd'):
        return (y ** 2).mean()
    return torch.nn.L1Loss()(y, torch.from_numpy(z[f'{cfg}/target']).to(DEV))


def _param_grads(model):
    return {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}


def _step(z, cfg, train=True):
    """-> model, output, node representation, loss, gradients of one forward + backward on the fixture's batch"""
    model = _model(z, cfg)
    model.train(train)
    feat = []
    hook = model.node_gnn.register_forward_hook(lambda mod, args, out: feat.append(out.detach().clone()))
    y = model(_graph(mols_from_npz(z, f'{cfg}/mol')))
    hook.remove()
    loss = _loss(cfg, y, z)
    loss.backward()
    return model, y.detach(), feat[0], loss.item(), _param_grads(model)


@pytest.mark.parametrize('cfg', sorted(GG.CONFIGS))
def test_module_matches_reference_fixture(cfg):
    """Gradients: rtol = max(1e-3, 4 x the fp32 reference's own error against its fp64 run, per tensor) - two fp32 implementations
    each as far from fp64 as the reference is, times two for the different summation order."""
    z = load('ogbgnn.npz')
    train = cfg != 'd'
    model, y, feat, loss, got = _step(z, cfg, train)
    assert y.shape == z[f'{cfg}/out'].shape
    print(f'{cfg}: out rel_err {rel_err(y.cpu(), z[f"{cfg}/out"]):.2e} feat rel_err {rel_err(feat.cpu(), z[f"{cfg}/feat"]):.2e}')
    assert rel_err(y.cpu(), z[f'{cfg}/out']) < 1e-4
    assert rel_err(feat.cpu(), z[f'{cfg}/feat']) < 1e-4
    assert abs(loss - float(z[f'{cfg}/loss'])) < 1e-4 * abs(float(z[f'{cfg}/loss']))
    ref = sd_from_npz(z, f'{cfg}/grad')
    assert set(got) == set(ref)            # JK 'sum' (b): the last layer's parameters have no gradient on either side
    scale = max(float(v.abs().max()) for v in ref.values())
    for k, v in ref.items():
        rtol = max(1e-3, 4 * float(z[f'{cfg}/ref_err/grad/{k}']))
        err = float((got[k].double() - v.double()).abs().max())
        print(f'{cfg}: grad {k}: err {err:.3e} max {float(v.abs().max()):.3e} rtol {rtol:.1e} scale {scale:.3e}')
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


@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_fused_message_step_matches_composed(cfg, monkeypatch):
    """FUSED_CONV True against False.  The two paths compute the same fp32 terms; only the order of the sum inside a neighbourhood
    (and of the table's gradient over a code's edges, fp64 on the fused side) differs, so the per-element bounds of the kernel test
    apply at every layer; propagated loosely through three layers: rel_err < 1e-5."""
    z = load('ogbgnn.npz')
    _, y1, f1, l1, g1 = _step(z, cfg)
    monkeypatch.setattr(gin, 'FUSED_CONV', False)
    _, y0, f0, l0, g0 = _step(z, cfg)
    assert rel_err(y1.cpu(), y0.cpu()) < 1e-5 and rel_err(f1.cpu(), f0.cpu()) < 1e-5
    assert set(g1) == set(g0)
    grads_close(g1, g0, 1e-5, what=f'{cfg} fused vs composed: ')


def test_two_identical_steps_are_bit_identical():
    z = load('ogbgnn.npz')
    m0, y0, f0, _, g0 = _step(z, 'a')
    m1, y1, f1, _, g1 = _step(z, 'a')
    assert torch.equal(y0, y1) and torch.equal(f0, f1)
    assert set(g0) == set(g1) == {k for k, _ in m0.named_parameters()}
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for (k, v), w in zip(m0.state_dict().items(), m1.state_dict().values()):
        assert torch.equal(v, w), k


def test_checkpoint_round_trip_is_bit_identical():
    z = load('ogbgnn.npz')
    model, *_ = _step(z, 'a')                       # one training forward: running statistics moved
    model.eval()
    g = _graph(mols_from_npz(z, 'a/mol'))
    sd = {k: v.cpu().clone() for k, v in model.state_dict().items()}
    assert list(sd) == list(sd_from_npz(z, 'a/sd'))
    fresh = amd.OGBGNN(**GG.CONFIGS['a'])
    fresh.load_state_dict(sd, strict=True)
    fresh.to(DEV).eval()
    with torch.no_grad():
        a, b = model(g), fresh(g)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_thirty_adam_steps_lower_the_loss_and_move_every_parameter():
    mols = synth.make_dataset(64, seed=8)
    g = _graph(mols)
    torch.manual_seed(2)
    model = amd.OGBGNN(target_dim=3, hidden_dim=64, num_layers=3, virtual_node=True).to(DEV).train()
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
    # A Linear bias directly in front of a training-mode BatchNorm has an analytically zero gradient (the BatchNorm removes the
    # shift): the fused Linear + BatchNorm backward writes exactly 0 for it, so Adam leaves it where it is.  Every OTHER parameter
    # must have moved - eps and virtualnode_embedding included.
    feeds_bn = {f'node_gnn.convs.{l}.mlp.{i}.bias' for l in range(3) for i in (0, 3)}
    feeds_bn |= {f'node_gnn.mlp_virtualnode_list.{l}.{i}.bias' for l in range(2) for i in (0, 3)}
    assert feeds_bn < set(before)
    for k, p in model.named_parameters():
        assert torch.isfinite(p).all(), k
        if k not in feeds_bn:
            assert not torch.equal(p.detach(), before[k]), k
    assert 'node_gnn.virtualnode_embedding.weight' in before and 'node_gnn.convs.0.eps' in before
