"""Net3DAE + NTXentAE on the MI355X: the fused pair head and the MSE kernels of csrc/pairmlp.hip against fp64 torch, the module against
the reference's own outputs and gradients (tests/golden/gen_golden_net3dae.py), the fused head against the composed path, eval mode,
determinism, a short training run, the device-assembled batch and the absence of host synchronisation."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import amd, close, grads_close, load, mols_from_npz, rel_err, sd_from_npz, synth

import gen_golden_net3dae as GA

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
graph_mod = importlib.import_module('3dinfomax_amd.graph')
layers = importlib.import_module('3dinfomax_amd.layers')
pair_head = importlib.import_module('3dinfomax_amd.pair_head')
net3d_ae = importlib.import_module('3dinfomax_amd.net3d_ae')
dataset_mod = importlib.import_module('3dinfomax_amd.dataset')
DEV = torch.device('cuda:0')
MOMENTUM, EPS = 0.1, 1e-5


def _pairs(kind, seed):
    """(src, dst, sizes): the complete graphs of molecules of 1, 2, 18 and 65 atoms, or ('asymmetric') a random 60 % of those ordered
    pairs - (i, j) without (j, i), nodes without in- or out-pairs"""
    sizes = [1, 2, 18, 65]
    src, dst, off = [], [], 0
    for n in sizes:
        s, d = synth.complete_graph_edges(n)
        src.append(s + off)
        dst.append(d + off)
        off += n
    src, dst = np.concatenate(src), np.concatenate(dst)
    if kind == 'asymmetric':
        keep = np.random.default_rng(seed).random(src.shape[0]) < 0.6
        src, dst = src[keep], dst[keep]
    return src, dst, sizes


def _head_inputs(H, D, N, P, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    return dict(h=r(N, H), W1=r(D, 2 * H) / (2 * H) ** 0.5, b1=0.3 * r(D), gamma=1 + 0.3 * r(D), beta=0.2 * r(D), W2=r(1, D) / D ** 0.5,
                b2=0.2 * r(1), rm=0.1 * r(D), rv=1 + 0.2 * torch.rand(D, generator=g), gout=r(P, 1))


def _head_reference(t, src, dst, dtype, training):
    """the reference formula (models/net3d_VAE.py:107-119, base_layers.py FCLayer: Linear -> activation -> BatchNorm) in torch on the CPU:
    -> {out, grads, running statistics after both calls}"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(k in ('h', 'W1', 'b1', 'gamma', 'beta', 'W2', 'b2')) for k, v in t.items()}
    rm, rv = p['rm'], p['rv']
    src, dst = torch.as_tensor(src), torch.as_tensor(dst)

    def net(x):
        x = F.relu(F.linear(x, p['W1'], p['b1']))
        x = F.batch_norm(x, rm, rv, p['gamma'], p['beta'], training, MOMENTUM, EPS)
        return F.linear(x, p['W2'], p['b2'])
    hs, hd = p['h'][src], p['h'][dst]
    y = F.softplus(net(torch.cat([hs, hd], 1)) + net(torch.cat([hd, hs], 1)))
    (y * p['gout']).sum().backward()
    out = {'out': y.detach(), 'rm': rm.detach(), 'rv': rv.detach()}
    out.update({'d' + k: p[k].grad for k in ('h', 'W1', 'b1', 'gamma', 'beta', 'W2', 'b2')})
    return out


def _head_ours(t, pidx, training):
    p = {k: v.detach().to(DEV).clone().requires_grad_(k in ('h', 'W1', 'b1', 'gamma', 'beta', 'W2', 'b2')) for k, v in t.items()}
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    bn = layers.BNSpec(p['rm'], p['rv'], nbt, MOMENTUM, EPS, training)
    y = pair_head._PairMLPHeadFn.apply(p['h'], p['W1'], p['b1'], p['gamma'], p['beta'], p['W2'], p['b2'], pidx, bn)
    (y * p['gout']).sum().backward()
    out = {'out': y.detach().cpu(), 'rm': p['rm'].detach().cpu(), 'rv': p['rv'].detach().cpu(), 'nbt': int(nbt)}
    out.update({'d' + k: p[k].grad.cpu() for k in ('h', 'W1', 'b1', 'gamma', 'beta', 'W2', 'b2')})
    return out


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('kind', ['complete', 'asymmetric'])
@pytest.mark.parametrize('H, D', [(16, 3), (70, 70), (200, 64)])
def test_fused_pair_head_matches_fp64(H, D, kind, training):
    """Every output of the fused head against the reference formula in fp64, both orders with their own statistics.  The bound is
    four times the error of the SAME formula in torch fp32 against fp64 on the same inputs (the factor: the kernel's sums are blocked
    differently from torch's), per quantity and case; the figures are printed before the assertions.

    Measured on an MI355X (relative error against fp64, max norm; torch fp32 / kernel), training mode, complete pair graphs:
        (H, D)      out            dh             dW1            db1            dgamma         dbeta          dW2            db2            running_var
        (16, 3)     4.5e-7/1.2e-7  7.5e-7/9.6e-8  1.5e-6/1.8e-7  3.8e-6/3.3e-7  1.2e-6/1.4e-7  1.7e-7/3.4e-8  3.2e-6/2.2e-7  3.4e-7/6.7e-8  1.5e-7/7.8e-8
        (70, 70)    4.3e-7/1.6e-7  4.1e-7/2.9e-7  4.8e-7/2.0e-7  1.3e-6/2.5e-7  4.1e-7/2.3e-7  8.2e-7/9.9e-8  9.9e-7/1.2e-7  3.3e-8/5.2e-8  1.9e-7/1.7e-7
        (200, 64)   4.8e-7/3.2e-7  6.6e-7/2.7e-7  6.4e-7/2.6e-7  2.2e-6/8.7e-7  9.9e-7/5.4e-7  7.4e-7/1.7e-7  1.4e-6/4.0e-7  5.5e-7/2.0e-7  1.3e-7/1.6e-7
    The asymmetric lists and eval mode give figures of the same size.  Over all 12 cases the largest kernel error relative to torch
    fp32's (the quantity bounded by 4) is 2.35: dgamma, (16, 3), asymmetric, eval, torch fp32 4.876e-8, kernel 1.148e-7.  In eval
    mode the running statistics are bit-equal."""
    src, dst, sizes = _pairs(kind, seed=H + D)
    N, P = sum(sizes), src.shape[0]
    t = _head_inputs(H, D, N, P, seed=3 * H + D)
    pidx = graph_mod.build_index(src, dst, N, np.asarray(sizes)).to(DEV)
    ref64 = _head_reference(t, src, dst, torch.float64, training)
    ref32 = _head_reference(t, src, dst, torch.float32, training)
    ours = _head_ours(t, pidx, training)
    assert ours['out'].shape == (P, 1)
    assert ours['nbt'] == (2 if training else 0)
    failures = []
    for k in ('out', 'dh', 'dW1', 'db1', 'dgamma', 'dbeta', 'dW2', 'db2', 'rm', 'rv'):
        e32, e = rel_err(ref32[k], ref64[k]), rel_err(ours[k], ref64[k])
        print(f'pair head H={H} D={D} {kind} training={training} {k}: torch fp32 {e32:.3e} kernel {e:.3e}')
        if not e <= 4 * e32:
            failures.append((k, e32, e))
    if not training:
        assert torch.equal(ours['rm'], t['rm']) and torch.equal(ours['rv'], t['rv'])
    assert not failures, failures


def test_fused_pair_head_without_pairs_and_single_pair():
    H, D, sizes = 16, 3, [1, 1, 1]
    t = _head_inputs(H, D, 3, 0, seed=1)
    empty = np.zeros(0, np.int64)
    pidx = graph_mod.build_index(empty, empty, 3, np.asarray(sizes)).to(DEV)
    for training in (True, False):
        o = _head_ours(t, pidx, training)
        assert o['out'].shape == (0, 1) and o['nbt'] == 0
        assert torch.equal(o['rm'], t['rm']) and torch.equal(o['rv'], t['rv'])
        for k in ('dh', 'dW1', 'db1', 'dgamma', 'dbeta', 'dW2', 'db2'):
            assert torch.count_nonzero(o[k]) == 0, k
    one = graph_mod.build_index(np.array([0]), np.array([1]), 3, np.asarray(sizes)).to(DEV)
    t1 = _head_inputs(H, D, 3, 1, seed=1)
    with pytest.raises(ValueError, match='more than one pair'):          # torch's BatchNorm refuses a single row in training mode too
        _head_ours(t1, one, True)
    o = _head_ours(t1, one, False)
    ref = _head_reference(t1, [0], [1], torch.float64, False)
    assert rel_err(o['out'], ref['out']) < 1e-5 and rel_err(o['dh'], ref['dh']) < 1e-5


@pytest.mark.parametrize('n', [1, 1252, 300001])
def test_mse_kernels_match_fp64(n):
    """same rule as the pair head: four times torch fp32's own error against fp64 (the kernels form differences, squares and sums in
    fp64 and round once, so their error is the rounding of the result).  Measured on an MI355X (torch fp32 / kernel), loss then
    gradient: n=1 1.4e-7/2.4e-8, 6.9e-8/4.3e-8; n=1252 8.3e-8/4.8e-9, 1.1e-7/3.4e-8; n=300001 7.9e-8/2.9e-10, 1.2e-7/3.1e-8"""
    g = torch.Generator().manual_seed(n)
    a, b = 3 * torch.rand(n, 1, generator=g), 3 * torch.rand(n, 1, generator=g)
    gs = torch.tensor(0.37)

    def ref(dtype):
        x = a.to(dtype).clone().requires_grad_(True)          # a copy: .to() of the same dtype returns a itself
        loss = 0.5 * F.mse_loss(b.to(dtype), x)
        (loss * gs.to(dtype)).backward()
        return loss.detach(), x.grad
    l64, g64 = ref(torch.float64)
    l32, g32 = ref(torch.float32)
    loss_fn = importlib.import_module('3dinfomax_amd.losses')._MSEFn
    x = a.to(DEV).requires_grad_(True)
    loss = loss_fn.apply(b.to(DEV), x, 0.5)
    (loss * gs.to(DEV)).backward()
    e32, e = rel_err(l32, l64), rel_err(loss.detach().cpu(), l64)
    ge32, ge = rel_err(g32, g64), rel_err(x.grad.cpu(), g64)
    print(f'mse n={n}: loss torch fp32 {e32:.3e} kernel {e:.3e}; grad torch fp32 {ge32:.3e} kernel {ge:.3e}')
    assert e <= 4 * e32 or e == 0.0
    assert ge <= 4 * ge32 or ge == 0.0


# ---- the module ------------------------------------------------------------------------------------------------------------------
def _items(mols):
    items = []
    for m in mols:
        s, d = synth.complete_graph_edges(m.n_atoms)
        dist = torch.from_numpy(synth.pairwise_distances(m.coords, s, d))
        items.append((amd.bond_graph(m), amd.complete_graph(m), torch.stack([torch.from_numpy(s), torch.from_numpy(d)]), dist))
    return items


def _batch(mols):
    (g2,), (g3, pidx), dist = amd.contrastive_vae_collate(_items(mols))
    return g3.to(DEV), pidx.to(DEV), dist.to(DEV)


def _model(z, cfg, train=True):
    model = amd.Net3DAE(**GA.CONFIGS[cfg])
    model.load_state_dict(sd_from_npz(z, f'{cfg}/sd'), strict=True)
    model.to(DEV)
    return model.train() if train else model.eval()


def _param_grads(model):
    return {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}


def _step(model, g3, pidx, dist, z1):
    """forward, both loss terms, backward of their sum -> (latent, pred, feat, contrastive, recon)"""
    g = g3.local_copy()
    latent, pred = model(g, pidx)
    contrastive, recon = amd.NTXentAE(**GA.LOSS)(z1, latent, dist, pred)
    (contrastive + recon).backward()
    return latent.detach(), pred.detach(), g.ndata['feat'].detach(), contrastive.detach(), recon.detach()


@pytest.mark.parametrize('cfg', sorted(GA.CONFIGS))
def test_module_matches_reference_fixture(cfg):
    """latent, distances and node state at 1e-4 relative, both loss terms at 1e-4, every parameter gradient of the summed loss with
    helpers.grads_close at 5e-4, the buffers after the step: the bounds of tests/test_gpu_distance_predictor.py"""
    z = load('net3dae.npz')
    mols = mols_from_npz(z, f'{cfg}/mol')
    model = _model(z, cfg)
    g3, pidx, dist = _batch(mols)
    z1 = torch.from_numpy(z[f'{cfg}/z1']).to(DEV)
    latent, pred, feat, contrastive, recon = _step(model, g3, pidx, dist, z1)
    assert latent.shape == tuple(z[f'{cfg}/latent'].shape) and pred.shape == (pidx.shape[1], 1)
    for name, got, key in (('latent', latent, 'latent'), ('distances', pred, 'pred'), ('feat', feat, 'feat')):
        e = rel_err(got.cpu(), z[f'{cfg}/{key}'])
        print(f'{cfg} {name}: rel err {e:.3e}')
        assert e < 1e-4, name
    for name, got in (('contrastive', contrastive), ('recon', recon)):
        ref = float(z[f'{cfg}/{name}'])
        print(f'{cfg} {name}: {got.item():.7f} reference {ref:.7f}')
        assert abs(got.item() - ref) < 1e-4 * abs(ref), name
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


def _run_both(z, cfg, train, monkeypatch):
    mols = mols_from_npz(z, f'{cfg}/mol')
    g3, pidx, dist = _batch(mols)
    z1 = torch.from_numpy(z[f'{cfg}/z1']).to(DEV)
    runs = []
    for fused in (True, False):
        monkeypatch.setattr(net3d_ae, 'FUSED_PAIR_HEAD', fused)
        model = _model(z, cfg, train)
        assert (model.fused_head_refusal() is None) == fused
        runs.append(_step(model, g3, pidx, dist, z1) + (_param_grads(model), {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    return runs


@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('cfg', ['a', 'b'])
def test_fused_head_matches_composed_path(cfg, train, monkeypatch):
    z = load('net3dae.npz')
    fused, composed = _run_both(z, cfg, train, monkeypatch)
    for name, a, b in zip(('latent', 'distances', 'feat'), fused[:3], composed[:3]):
        assert rel_err(a.cpu(), b.cpu()) < 1e-4, name
    for name, a, b in zip(('contrastive', 'recon'), fused[3:5], composed[3:5]):
        assert abs(a.item() - b.item()) < 1e-4 * abs(b.item()), name
    assert set(fused[5]) == set(composed[5])
    grads_close(fused[5], composed[5], 5e-4, what=f'{cfg} fused vs composed: ')
    for k, v in composed[6].items():
        if 'running' in k:
            assert close(fused[6][k], v, 1e-4, 1e-6), k
        elif 'num_batches_tracked' in k:
            assert int(fused[6][k]) == int(v), k
    if not train:
        z0 = sd_from_npz(z, f'{cfg}/sd')
        for k, v in fused[6].items():          # eval mode leaves the running statistics alone
            assert torch.equal(v, z0[k]), k


def test_two_identical_steps_are_bit_identical():
    z = load('net3dae.npz')
    mols = synth.make_dataset(30, seed=3) + mols_from_npz(z, 'a/mol')
    g3, pidx, dist = _batch(mols)
    z1 = torch.randn(len(mols), 48, generator=torch.Generator().manual_seed(1)).to(DEV)
    results = []
    for _ in range(2):
        model = _model(z, 'a')
        out = _step(model, g3, pidx, dist, z1)
        results.append((out, _param_grads(model), {k: v.clone() for k, v in model.state_dict().items()}))
    (o0, g0, s0), (o1, g1, s1) = results
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


def _train(z, fused, steps, monkeypatch):
    monkeypatch.setattr(net3d_ae, 'FUSED_PAIR_HEAD', fused)
    mols = synth.make_dataset(48, seed=8)
    g3, pidx, dist = _batch(mols)
    z1 = torch.randn(len(mols), 48, generator=torch.Generator().manual_seed(2)).to(DEV)
    model = _model(z, 'a')
    loss_fn = amd.NTXentAE(**GA.LOSS)
    opt = amd.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        latent, pred = model(g3.local_copy(), pidx)
        contrastive, recon = loss_fn(z1, latent, dist, pred)
        loss = contrastive + recon
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
        opt.step()
        losses.append(loss.item())
    return losses


def test_thirty_adam_steps_lower_the_loss_and_track_the_composed_path(monkeypatch):
    z = load('net3dae.npz')
    fused = _train(z, True, 30, monkeypatch)
    composed = _train(z, False, 30, monkeypatch)
    print('fused   ', ' '.join(f'{v:.5f}' for v in fused))
    print('composed', ' '.join(f'{v:.5f}' for v in composed))
    assert all(np.isfinite(fused))
    assert np.mean(fused[-5:]) < 0.9 * np.mean(fused[:3]), fused
    assert abs(fused[-1] - composed[-1]) < 1e-4 * abs(composed[-1]), (fused[-1], composed[-1])


def test_device_assembled_batch_equals_collate():
    mols = synth.make_dataset(7, seed=4) + synth.make_dataset(1, seed=5, kind='qmugs')
    ds = dataset_mod.FlatMolDataset(mols)
    [g2], [g3, pidx], dist = ds.assemble_ae(np.arange(len(mols)), DEV)
    g3c, pidx_c, dist_c = _batch(mols)
    assert torch.equal(pidx.cpu(), pidx_c.cpu())
    assert rel_err(dist.cpu(), dist_c.cpu()) < 1e-6
    assert g2.number_of_nodes() == g3.number_of_nodes() == g3c.number_of_nodes()
    assert pair_head.pair_index(pidx, g3) is g3.index()
    z = load('net3dae.npz')
    model = _model(z, 'a')
    with torch.no_grad():
        la, da = model(g3, pidx)
        lb, db = model(g3c, pidx_c)
    assert rel_err(la.cpu(), lb.cpu()) < 1e-5 and rel_err(da.cpu(), db.cpu()) < 1e-5
    assert dist.data_ptr() != g3.edata['d'].data_ptr()          # the model's overwrite of edata['d'] does not touch the targets
    assert rel_err(dist.cpu(), dist_c.cpu()) < 1e-6


def test_assemble_and_training_step_do_not_synchronise():
    mols = synth.make_dataset(64, seed=12)
    ds = dataset_mod.FlatMolDataset(mols)
    ids = np.arange(len(mols))
    z = load('net3dae.npz')
    model = _model(z, 'a')
    loss_fn = amd.NTXentAE(**GA.LOSS)
    z1 = torch.randn(len(mols), 48, generator=torch.Generator().manual_seed(2)).to(DEV)

    def step():
        [g2], [g3, pidx], dist = ds.assemble_ae(ids, DEV)
        latent, pred = model(g3, pidx)
        contrastive, recon = loss_fn(z1, latent, dist, pred)
        (contrastive + recon).backward()
        return contrastive, recon
    step()                                   # allocations, workspaces, the library's first load
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        contrastive, recon = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(contrastive) and torch.isfinite(recon)
    assert model.fused_head_refusal() is None


def test_ntxentae_refuses_a_world_of_two(monkeypatch):
    loss = amd.NTXentAE(**GA.LOSS)
    group = object()
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2 if g is group else 1)
    loss.attach_group(group)
    zz = torch.zeros(4, 8, device=DEV)
    with pytest.raises(NotImplementedError, match='NTXentAE'):
        loss(zz, zz, torch.zeros(5, 1, device=DEV), torch.zeros(5, 1, device=DEV))
