"""Fixture of the local-global pre-training mode (reference commons/losses.py: NTXentLocalGlobal; models/legacy/pna_local.py: PNALocal):
the unmodified reference classes on fixed random embeddings and on seeded synthetic molecules -> tests/golden/local_global.npz.

    python tests/golden/gen_golden_local_global.py          (imports the reference checkout, as gen_golden.py does)

Every case runs in fp32 and in fp64 (the same module / inputs converted); both are stored ('<quantity>' and '<quantity>64') with
ref_err/<quantity> = the fp32 run's own error against its fp64 run.

Loss cases (LOSS_CASES: nodes_per_graph, D, tau): zn [N, D], zg [B, D], loss, dzn, dzg.
  'b2'    [5, 9], D = 6, tau 0.1: the B = 2 minimum, D no multiple of 4; zn = relu(randn), the seed the first one whose zn holds an
          all-zero row (what PNALocal's final ReLU can produce): that row's gradient is of order 1 / (N tau 1e-10)
  'zero'  [1, 7, 64, 3, 1], D = 24, tau 0.5, row 3 set to zero
  'long'  [70, 70, 70, 1, 129], D = 256, tau 0.1: segments longer than a wave and than 128 rows, a one-node graph between them.
          Committed files stay below 1 MiB and this case's [340, 256] arrays are most of the file: its inputs are randn rounded to
          multiples of 1/32 (they compress to a third), and the fp32 run's dzn is not stored - ref_err/dzn is all the tests take from it
Measures of ref_err (the GPU tests use the same ones, row_rel_err / helpers-style max-norm):
  loss  max(|l32 - l64| / |l64|, 2^-24); ref_err/loss_raw is the first term alone.  The loss is ONE rounded fp32 number: its distance
        from the fp64 value is anywhere in [0, 2^-24] of it by chance (1e-9 for 'long'), and no fp32 result can be asked to be nearer
        than the format's rounding unit
  dzg   max |d32 - d64| / max |d64|
  dzn   row by row: max_i ( max_c |d32 - d64|_ic / max(max_c |d64|_ic, 1e-6 x the median over the rows of max_c |d64|_ic) ) - a zero row
        carries a gradient ten orders of magnitude above the others, and a whole-tensor max-norm would check that row alone

Model case 'model/': PNALocal at hidden_dim 16, propagation_depth 2, target_dim 8, readout_hidden_dim 10 with the aggregators, scalers,
BatchNorm flags and pre / posttrans depths of configs/old_configs/contrastive_local.yml on gen_golden_gin.molecules (five QM9-like
molecules, one above 64 atoms, one single atom), fixed random zg [7, 8], loss = NTXentLocalGlobal(tau=0.1)(model(g), zg,
g.batch_num_nodes()): state_dict, output and loss (fp32 and fp64), every parameter's gradient (fp32; the fp64 ones enter ref_err only), the buffers after the
step.  ref_err of a gradient as in
gen_golden_egnn.py.

The DGL stand-in of tests/golden/_stubs and the encoder stand-ins of gen_golden_gin.register_stand_ins cover what the two reference
modules touch.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_gin as GG  # noqa: E402

LOSS_CASES = {
    'b2': dict(nodes_per_graph=[5, 9], dim=6, tau=0.1),
    'zero': dict(nodes_per_graph=[1, 7, 64, 3, 1], dim=24, tau=0.5),
    'long': dict(nodes_per_graph=[70, 70, 70, 1, 129], dim=256, tau=0.1),
}
MODEL = dict(node_dim=None, edge_dim=None, hidden_dim=16, target_dim=8, propagation_depth=2, readout_hidden_dim=10,
             aggregators=['mean', 'max', 'min', 'std'], scalers=['identity', 'amplification', 'attenuation'], mid_batch_norm=True,
             last_batch_norm=True, readout_batchnorm=True, dropout=0.0, pretrans_layers=2, posttrans_layers=1, residual=True)
MODEL_SEED, MODEL_TAU = 81, 0.1


def loss_inputs(name):
    """zn [N, D], zg [B, D] of a loss case (fp32, fixed seeds)"""
    c = LOSS_CASES[name]
    n, b, d = sum(c['nodes_per_graph']), len(c['nodes_per_graph']), c['dim']
    if name == 'b2':
        for seed in range(1000, 2000):
            gen = torch.Generator().manual_seed(seed)
            zn = torch.relu(torch.randn(n, d, generator=gen))
            zg = torch.randn(b, d, generator=gen)
            if int((zn.abs().sum(1) == 0).sum()) == 1:
                return zn, zg
        raise RuntimeError('no seed with a zero row')
    gen = torch.Generator().manual_seed({'zero': 31, 'long': 32}[name])
    zn, zg = torch.randn(n, d, generator=gen), torch.randn(b, d, generator=gen)
    if name == 'zero':
        zn[3] = 0
    if name == 'long':
        zn, zg = torch.round(zn * 32) / 32, torch.round(zg * 32) / 32
    return zn, zg


def row_rel_err(a, b):
    """the dzn measure of the module docstring: a against the fp64 values b"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    rowmax = b.abs().amax(1)
    floor = 1e-6 * float(rowmax.median())
    return float(((a - b).abs().amax(1) / rowmax.clamp(min=floor)).max())


def run_loss(loss_fn, zn, zg, npg):
    zn, zg = zn.clone().requires_grad_(True), zg.clone().requires_grad_(True)
    loss = loss_fn(zn, zg, torch.tensor(npg))
    loss.backward()
    return loss.detach(), zn.grad, zg.grad


def run_model(model, bg, zg, loss_fn):
    y = model(bg)
    loss = loss_fn(y, zg, bg.batch_num_nodes())
    model.zero_grad()
    loss.backward()
    return y.detach(), bg.ndata['feat'].detach(), loss.detach()


def main():
    dgl = G.import_reference()[0]
    GG.register_stand_ins(dgl)
    from commons.losses import NTXentLocalGlobal
    from models.legacy.pna_local import PNALocal
    out = {}
    for name, c in LOSS_CASES.items():
        zn, zg = loss_inputs(name)
        fn = NTXentLocalGlobal(tau=c['tau'])
        l32, dn32, dg32 = run_loss(fn, zn, zg, c['nodes_per_graph'])
        l64, dn64, dg64 = run_loss(fn, zn.double(), zg.double(), c['nodes_per_graph'])
        assert torch.isfinite(l32) and torch.isfinite(dn32).all() and torch.isfinite(dg32).all()
        p = f'loss/{name}/'
        out[p + 'zn'], out[p + 'zg'] = zn.numpy(), zg.numpy()
        out[p + 'nodes_per_graph'] = np.array(c['nodes_per_graph'], dtype=np.int64)
        out[p + 'loss'], out[p + 'dzg'] = np.array(l32.item(), dtype=np.float32), dg32.numpy()
        if name != 'long':
            out[p + 'dzn'] = dn32.numpy()
        out[p + 'loss64'], out[p + 'dzn64'], out[p + 'dzg64'] = np.array(l64.item()), dn64.numpy(), dg64.numpy()
        out[p + 'ref_err/loss_raw'] = np.array(abs(l32.item() - l64.item()) / abs(l64.item()))
        out[p + 'ref_err/loss'] = np.maximum(out[p + 'ref_err/loss_raw'], 2.0 ** -24)
        out[p + 'ref_err/dzn'] = np.array(row_rel_err(dn32, dn64))
        out[p + 'ref_err/dzg'] = np.array(GG.rel_err(dg32, dg64))
        print(name, 'N', zn.shape[0], 'B', zg.shape[0], 'loss', l32.item(), l64.item(), 'zero rows', int((zn.abs().sum(1) == 0).sum()),
              'max |dzn|', float(dn64.abs().max()), 'ref_err loss', float(out[p + 'ref_err/loss']), 'dzn', float(out[p + 'ref_err/dzn']),
              'dzg', float(out[p + 'ref_err/dzg']))

    mols = GG.molecules(MODEL_SEED)
    torch.manual_seed(7)
    model = PNALocal(**MODEL)
    G.make_trained_like(model, 29)
    model.train()
    zg = torch.randn(len(mols), MODEL['target_dim'], generator=torch.Generator().manual_seed(MODEL_SEED + 1))
    fn = NTXentLocalGlobal(tau=MODEL_TAU)
    p = 'model/'
    out.update(G.mols_to_npz(mols, prefix=p + 'mol'))
    out[p + 'zg'] = zg.numpy()
    out.update(G.sd_np(model, p + 'sd'))
    ref64 = copy.deepcopy(model).double()
    y, nodes, loss = run_model(model, GG.graph_of(dgl, mols), zg, fn)
    assert torch.equal(y, nodes)
    out[p + 'out'], out[p + 'loss'] = y.numpy(), np.array(loss.item())
    out.update({f'{p}grad/{k}': q.grad.numpy().copy() for k, q in model.named_parameters()})
    out.update({f'{p}buf_after/{k}': v.numpy().copy() for k, v in model.named_buffers()})
    y64, _, loss64 = run_model(ref64, GG.graph_of(dgl, mols), zg.double(), fn)
    out[p + 'out64'], out[p + 'loss64'] = y64.numpy(), np.array(loss64.item())
    out[p + 'ref_err/out'] = np.array(GG.rel_err(y, y64))
    out[p + 'ref_err/loss'] = np.array(abs(loss.item() - loss64.item()) / abs(loss64.item()))
    g64 = dict(ref64.named_parameters())
    scale = max(float(q.grad.abs().max()) for q in g64.values())
    worst = 0.0
    for k, q in model.named_parameters():
        e = float((q.grad.double() - g64[k].grad).abs().max() / max(float(g64[k].grad.abs().max()), 1e-4 * scale))
        out[f'{p}ref_err/grad/{k}'] = np.array(e)
        worst = max(worst, e)
    print('model atoms', [m.n_atoms for m in mols], 'zero output rows', int((y.abs().sum(1) == 0).sum()), 'loss', loss.item(),
          loss64.item(), 'ref_err out', float(out[p + 'ref_err/out']), 'worst grad ref_err', worst)
    path = os.path.join(HERE, 'local_global.npz')
    np.savez_compressed(path, **out)
    print('wrote local_global.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(4)
    main()
