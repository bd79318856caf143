"""DistancePredictor on the MI355X: the kernels of csrc/distance.hip against fp64 torch, the module against the reference's own
outputs and gradients (tests/golden/gen_golden_distance.py), the blessed size against a torch-eager composition with the same
weights, determinism, eval mode and a short training run."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import amd, close, grads_close, load, mols_from_npz, rel_err, sd_from_npz, synth

import gen_golden_distance as GD

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
dataset_mod = importlib.import_module('3dinfomax_amd.dataset')
DEV = torch.device('cuda:0')
SIZES = [1, 2, 3, 18, 29, 64, 65, 130, 200]
BLESSED_PNA = dict(hidden_dim=200, mid_batch_norm=True, last_batch_norm=True, batch_norm_momentum=0.1, dropout=0.0, propagation_depth=7,
                   aggregators=['mean', 'max', 'min', 'std'], scalers=['identity', 'amplification', 'attenuation'],
                   readout_aggregators=['min', 'max', 'mean', 'sum'], pretrans_layers=2, posttrans_layers=1, residual=True)
BLESSED = dict(target_dim=1, projection_dim=0, distance_net=True, projection_layers=1, transformer_layer=True, nhead=2,
               dim_feedforward=200)


def _graph_ptr(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)


def _mha_ref(qkv, sizes, nhead):
    """fp64 softmax(q k^T / sqrt(dh)) v per molecule and head"""
    H = qkv.shape[1] // 3
    dh = H // nhead
    out, o = [], 0
    for n in sizes:
        q, k, v = (qkv[o:o + n, j * H:(j + 1) * H].reshape(n, nhead, dh).transpose(0, 1) for j in range(3))
        a = torch.softmax(q @ k.transpose(1, 2) / dh ** 0.5, dim=-1) @ v
        out.append(a.transpose(0, 1).reshape(n, H))
        o += n
    return torch.cat(out)


@pytest.mark.parametrize('dh', [100, 50, 13, 8])
def test_attention_matches_fp64(dh):
    nhead = 2
    H = nhead * dh
    g = torch.Generator().manual_seed(dh)
    N = sum(SIZES)
    qkv = torch.randn(N, 3 * H, generator=g, dtype=torch.float64) * 1.5
    gout = torch.randn(N, H, generator=g, dtype=torch.float64)
    ptr = _graph_ptr(SIZES)
    q32 = qkv.float().to(DEV)
    out, lse = ops.mha_fwd(q32, ptr, len(SIZES), nhead, 1.0 / dh ** 0.5)
    dq = ops.mha_bwd(q32, out, gout.float().to(DEV), lse, ptr, len(SIZES), nhead, 1.0 / dh ** 0.5)
    x = q32.double().cpu().requires_grad_(True)
    ref = _mha_ref(x, SIZES, nhead)
    (ref * gout).sum().backward()
    assert rel_err(out.cpu(), ref.detach()) < 2e-5
    assert rel_err(dq.cpu(), x.grad) < 5e-5
    o = 0
    for n in SIZES:          # every molecule on its own (a small one next to big ones is not drowned by the global max)
        assert rel_err(out[o:o + n].cpu(), ref.detach()[o:o + n]) < 2e-5, n
        assert rel_err(dq[o:o + n].cpu(), x.grad[o:o + n]) < 5e-5, n
        o += n
    assert torch.isfinite(lse).all()


@pytest.mark.parametrize('feat', [200, 13])
def test_layernorm_residual_matches_fp64(feat):
    g = torch.Generator().manual_seed(feat)
    rows = 1000
    x, r = (torch.randn(rows, feat, generator=g) * 2 + 0.5 for _ in range(2))
    gamma, beta = 1 + 0.3 * torch.randn(feat, generator=g), 0.2 * torch.randn(feat, generator=g)
    gy = torch.randn(rows, feat, generator=g)
    y, mean, rstd = ops.ln_res_fwd(x.to(DEV), r.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-5)
    gz, gg, gb = ops.ln_res_bwd(gy.to(DEV), x.to(DEV), r.to(DEV), gamma.to(DEV), mean, rstd)
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = F.layer_norm(xd + r.double(), (feat,), gd, bd, 1e-5)
    (ref * gy.double()).sum().backward()
    assert rel_err(y.cpu(), ref.detach()) < 1e-5
    assert rel_err(gz.cpu(), xd.grad) < 1e-5
    assert rel_err(gg.cpu(), gd.grad) < 1e-5
    assert rel_err(gb.cpu(), bd.grad) < 1e-5


def _pair_batch(sizes, seed):
    mols = [synth.Molecule(n, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((n, 9), np.int64), np.zeros((0, 3), np.int64),
                           np.random.default_rng(seed + n).normal(size=(n, 3)).astype(np.float32)) for n in sizes]
    g = amd.batch([amd.complete_graph(m) for m in mols])
    src, dst = g.edges()
    return g.index().to(DEV), src, dst


@pytest.mark.parametrize('T', [1, 3])
def test_pair_sum_head_matches_fp64_and_is_symmetric(T):
    sizes = [1, 2, 18, 65]
    pidx, src, dst = _pair_batch(sizes, 1)
    N = sum(sizes)
    g = torch.Generator().manual_seed(T)
    u, b = torch.randn(N, T, generator=g) * 3, torch.randn(T, generator=g)
    gout = torch.randn(src.shape[0], T, generator=g)
    out = ops.pair_sum_fwd(u.to(DEV), b.to(DEV), pidx)
    du = ops.pair_sum_bwd(gout.to(DEV), u.to(DEV), b.to(DEV), pidx)
    ud = u.double().requires_grad_(True)
    ref = F.softplus(ud[src] + ud[dst] + 2 * b.double())
    (ref * gout.double()).sum().backward()
    assert rel_err(out.cpu(), ref.detach()) < 1e-6
    assert rel_err(du.cpu(), ud.grad) < 1e-5
    # d_ij == d_ji exactly: the pair (j, i) of pair (i, j)
    key = {(int(s), int(d)): p for p, (s, d) in enumerate(zip(src.tolist(), dst.tolist()))}
    rev = torch.tensor([key[(int(d), int(s))] for s, d in zip(src.tolist(), dst.tolist())])
    oc = out.cpu()
    assert torch.equal(oc, oc[rev])


def test_pair_norm_matches_fp64_and_is_zero_at_coincident_points():
    sizes = [3, 18, 130]
    pidx, src, dst = _pair_batch(sizes, 2)
    N = sum(sizes)
    g = torch.Generator().manual_seed(5)
    p = torch.randn(N, 3, generator=g)
    p[1] = p[0]                              # distance 0 between nodes 0 and 1
    gout = torch.randn(src.shape[0], 1, generator=g)
    out = ops.pair_norm_fwd(p.to(DEV), pidx)
    dpp = ops.pair_norm_bwd(gout.to(DEV), p.to(DEV), out, pidx)
    pd = p.double().requires_grad_(True)
    ref = torch.norm(pd[src] - pd[dst], dim=-1).unsqueeze(-1)
    (ref * gout.double()).sum().backward()
    assert rel_err(out.cpu(), ref.detach()) < 1e-6
    assert rel_err(dpp.cpu(), pd.grad) < 1e-5
    assert torch.isfinite(dpp).all()


def _items(mols):
    items = []
    for m in mols:
        s, d = synth.complete_graph_edges(m.n_atoms)
        items.append((amd.bond_graph(m), torch.stack([torch.from_numpy(s), torch.from_numpy(d)]),
                      torch.from_numpy(synth.pairwise_distances(m.coords, s, d))))
    return items


def _batch(mols):
    (g, pidx, mask), dist = amd.pairwise_distance_collate(_items(mols))
    return g.to(DEV), pidx.to(DEV), mask.to(DEV), dist.to(DEV)


def _param_grads(model):
    return {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('cfg', sorted(GD.CONFIGS))
def test_module_matches_reference_fixture(cfg):
    """outputs and node state at 1e-4; the pair head's rewrite (u = (W_a + W_b) h, then u_i + u_j + 2b) changes only the order of
    fp32 sums; gradients of the whole model under L1Loss with the bound of the PNA fixtures"""
    z = load('distance_predictor.npz')
    mols = mols_from_npz(z, f'{cfg}/mol')
    model = amd.DistancePredictor(pna_args=dict(GD.PNA_ARGS), **GD.CONFIGS[cfg])
    model.load_state_dict(sd_from_npz(z, f'{cfg}/sd'), strict=True)
    model.to(DEV).train()
    g, pidx, mask, dist = _batch(mols)
    y = model(g, pidx, mask)
    assert y.shape == (pidx.shape[1], 1)
    assert rel_err(y.detach().cpu(), z[f'{cfg}/out']) < 1e-4
    assert rel_err(g.ndata['feat'].detach().cpu(), z[f'{cfg}/feat']) < 1e-4
    loss = torch.nn.L1Loss()(y, dist)
    assert abs(loss.item() - float(z[f'{cfg}/loss'])) < 1e-4 * abs(float(z[f'{cfg}/loss']))
    loss.backward()
    ref = sd_from_npz(z, f'{cfg}/grad')
    got = _param_grads(model)
    assert set(got) == set(ref)
    grads_close(got, ref, 5e-4, what=f'{cfg}: ')
    sd = model.state_dict()
    for k, v in sd_from_npz(z, f'{cfg}/buf_after').items():
        if 'running' in k:
            assert close(sd[k], v, 1e-4, 1e-6), k
        else:
            assert int(sd[k]) == int(v), k


def test_device_assembled_batch_equals_collate():
    mols = synth.make_dataset(7, seed=4) + synth.make_dataset(1, seed=5, kind='qmugs')
    ds = dataset_mod.FlatMolDataset(mols)
    [g2, pidx, mask], dist = ds.assemble_distance(np.arange(len(mols)), DEV)
    g, pidx_c, mask_c, dist_c = _batch(mols)
    assert torch.equal(pidx.cpu(), pidx_c.cpu()) and torch.equal(mask.cpu(), mask_c.cpu())
    assert rel_err(dist.cpu(), dist_c.cpu()) < 1e-6
    torch.manual_seed(0)
    model = amd.DistancePredictor(pna_args=dict(GD.PNA_ARGS), **GD.CONFIGS['a']).to(DEV).train()
    with torch.no_grad():
        a = model(g2, pidx, mask)
        b = model(g, pidx_c, mask_c)
    assert torch.equal(a, b)


def _blessed(seed=0):
    torch.manual_seed(seed)
    return amd.DistancePredictor(pna_args=dict(BLESSED_PNA), **BLESSED).to(DEV)


def _eager(model, g, pidx, mask):
    """torch-eager composition of the reference's transformer and head on our PNAGNN output: padded batch, key padding mask,
    nn.TransformerEncoderLayer.forward, the two distance_net calls on the [P, 2H] concatenations"""
    gg = g.local_copy()
    model.node_gnn(gg)
    h = gg.ndata['feat']
    B, M = mask.shape
    H = h.shape[1]
    keep = ~mask.reshape(-1)
    pad = torch.zeros(B * M, H, device=h.device)
    pad[keep] = h
    t = model.transformer_layer(pad.view(B, M, H), src_key_padding_mask=mask)
    h = t.reshape(B * M, H)[keep]
    lin = model.distance_net.fully_connected[0].linear
    hs, hd = h[pidx[0]], h[pidx[1]]
    return F.softplus(F.linear(torch.cat([hs, hd], 1), lin.weight, lin.bias) + F.linear(torch.cat([hd, hs], 1), lin.weight, lin.bias))


@pytest.mark.parametrize('kind, n', [('qm9', 100), ('qmugs', 12)])
def test_blessed_size_matches_torch_eager(kind, n):
    mols = synth.make_dataset(n, seed=11, kind=kind)
    model = _blessed().train()
    g, pidx, mask, dist = _batch(mols)
    loss = torch.nn.L1Loss()(model(g.local_copy(), pidx, mask), dist)
    loss.backward()
    ours = {k: p.grad.clone() for k, p in model.named_parameters() if k.startswith(('transformer_layer', 'distance_net'))}
    model.zero_grad()
    ref = torch.nn.L1Loss()(_eager(model, g, pidx, mask), dist)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    for k, v in ours.items():
        assert rel_err(v.cpu(), dict(model.named_parameters())[k].grad.cpu()) < 2e-3, k
    # eval mode (running statistics, no gradient): same composition
    model.eval()
    with torch.no_grad():
        a = model(g.local_copy(), pidx, mask)
        b = _eager(model, g, pidx, mask)
    assert rel_err(a.cpu(), b.cpu()) < 1e-4


def test_two_identical_steps_are_bit_identical():
    mols = synth.make_dataset(30, seed=3) + synth.make_dataset(2, seed=3, kind='qmugs')
    g, pidx, mask, dist = _batch(mols)
    results = []
    for _ in range(2):
        model = _blessed(seed=1).train()
        y = model(g.local_copy(), pidx, mask)
        torch.nn.L1Loss()(y, dist).backward()
        results.append((y.detach().clone(), _param_grads(model), {k: v.clone() for k, v in model.state_dict().items()}))
    (y0, g0, s0), (y1, g1, s1) = results
    assert torch.equal(y0, y1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


@pytest.mark.parametrize('cfg', sorted(GD.CONFIGS))
def test_eval_mode_matches_with_and_without_grad(cfg):
    z = load('distance_predictor.npz')
    mols = mols_from_npz(z, f'{cfg}/mol')
    model = amd.DistancePredictor(pna_args=dict(GD.PNA_ARGS), **GD.CONFIGS[cfg])
    model.load_state_dict(sd_from_npz(z, f'{cfg}/sd'), strict=True)
    model.to(DEV).eval()
    g, pidx, mask, _ = _batch(mols)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        a = model(g.local_copy(), pidx, mask)
    b = model(g.local_copy(), pidx, mask)
    assert torch.isfinite(a).all()
    assert rel_err(a.cpu(), b.detach().cpu()) < 1e-6
    for k, v in model.state_dict().items():          # eval mode leaves the running statistics alone
        assert torch.equal(v, before[k]), k


def test_thirty_adam_steps_lower_the_l1_loss():
    mols = synth.make_dataset(64, seed=8)
    g, pidx, mask, dist = _batch(mols)
    model = _blessed(seed=2).train()
    opt = amd.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.L1Loss()(model(g.local_copy(), pidx, mask), dist)
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < 0.9 * np.mean(losses[:3]), losses
