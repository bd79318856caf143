"""Fixtures of NTXentLikelihoodLoss (reference commons/losses.py:537-595), JSDMultiplePositivesLoss (:317-391) and the metrics
PositiveProb / NegativeProb (trainer/metrics.py:336-395): the unmodified reference classes on seeded inputs ->
tests/golden/gauss_pair.npz (likelihood loss and metrics), gauss_pair_jsd.npz (JSD loss), gauss_pair_e2e.npz (end to end).  Three files:
the fp64 gradients of the nine shapes alone pass the size a committed file may have.

    python tests/golden/gen_golden_gauss.py          (imports the reference checkout, as gen_golden.py does)

Loss level.  Inputs z1 [B, 2 D] (mean | log-variance), z2 [B C, D] (fp32) once per case ('in/<case>/z1', '.../z2', in both loss files);
per setting the reference's loss, dz1 and dz2 computed in fp32 ('loss32', 'dz1_32', 'dz2_32') and in fp64 on the same inputs ('loss64',
...), under 'lik/<case>/t0.1/', 'lik/<case>/t0.5/' (tau) and 'jsd/<case>/n0/', 'jsd/<case>/n1/' (norm off / on).  Cases (B, C, D), standard
normal entries, the log-variance half scaled by 0.5: (2, 2, 8), (2, 1, 8) (likelihood only), (5, 3, 24), (7, 5, 40), (3, 2, 7), (4, 9, 16),
(65, 3, 32), (6, 3, 256), (9, 2, 300).  Edge cases at (5, 3, 24):

  likelihood  'sharp': log-variance ~ N(-4, 0.5^2), z2 random.  'aligned2' / 'aligned4': z2 = the predicted mean + 0.3 sigma noise at
              log-variance ~ N(-2, 0.5^2) / N(-4, 0.5^2); at -4 and tau = 0.1 the reference's fp32 loss is -inf (its `row sum - positive`
              rounds to 0) while its fp64 loss is finite.  Not sharper: at -5 the fp64 loss is -inf as well.
  JSD         'jitter2' / 'jitter3': the conformers of a molecule are a base vector + 1e-2 / 1e-3 noise (1 / v2 large).

Metrics ('metrics/<case>/positive_prob', '.../negative_prob', in gauss_pair.npz): both metrics in fp64 on the inputs of every likelihood
case; the metrics read the SAME z2 array conformer major (row r: molecule r % B, conformer r // B).

End to end ('e2e/...'): 4 synthetic molecules x 2 conformers through the reference PNA (hidden 16, target_dim 2 * 8, depth 2) and Net3D
(hidden 8, target_dim 8) batched by the reference's conformer_collate, loss NTXentLikelihoodLoss(tau=0.1, conformer_variance_reg=0.05);
the loss, both embeddings and every parameter gradient, computed by the reference in fp64 from the fp32 weights and inputs stored beside
them.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_kl as GK  # noqa: E402

CASES = [(2, 2, 8), (2, 1, 8), (5, 3, 24), (7, 5, 40), (3, 2, 7), (4, 9, 16), (65, 3, 32), (6, 3, 256), (9, 2, 300)]
EDGE_SHAPE = (5, 3, 24)
LIK_EDGES = ('sharp', 'aligned2', 'aligned4')
JSD_EDGES = ('jitter2', 'jitter3')
TAUS = (0.1, 0.5)
LIK_CASES = [(c, None) for c in CASES] + [(EDGE_SHAPE, e) for e in LIK_EDGES]
JSD_CASES = [(c, None) for c in CASES if c[1] >= 2] + [(EDGE_SHAPE, e) for e in JSD_EDGES]
FILES = {'lik': 'gauss_pair.npz', 'jsd': 'gauss_pair_jsd.npz', 'e2e': 'gauss_pair_e2e.npz'}
E2E_MOLS, E2E_CONF, E2E_DIM = 4, 2, 8
E2E_TAU, E2E_CONF_REG = 0.1, 0.05
E2E_NOISE = 0.3          # coordinate noise of the synthetic conformers, as gen_golden_kl.py (main() asserts the yardstick holds)
PNA_KW = dict(G.PNA_YML, hidden_dim=16, target_dim=2 * E2E_DIM, propagation_depth=2, readout_hidden_dim=16)
NET3D_KW = dict(G.NET3D_YML, hidden_dim=8, hidden_edge_dim=8, readout_hidden_dim=8, target_dim=E2E_DIM)


def case_tag(shape, edge=None):
    B, C, D = shape
    return f'{B}x{C}x{D}' + (f'_{edge}' if edge else '')


def case_inputs(shape, edge=None):
    B, C, D = shape
    salt = 0 if edge is None else 1 + (LIK_EDGES + JSD_EDGES).index(edge)
    g = torch.Generator().manual_seed(3000 * B + 10 * C + D + 100000 * salt)
    z1 = torch.randn(B, 2 * D, generator=g)
    z1[:, D:] *= 0.5
    z2 = torch.randn(B * C, D, generator=g)
    if edge in LIK_EDGES:
        z1[:, D:] += -2.0 if edge == 'aligned2' else -4.0
    if edge in ('aligned2', 'aligned4'):
        sigma = torch.exp(z1[:, D:] / 2)
        z2 = (z1[:, None, :D] + 0.3 * sigma[:, None, :] * z2.reshape(B, C, D)).reshape(B * C, D)
    if edge in JSD_EDGES:
        base = torch.randn(B, 1, D, generator=g)
        z2 = (base + (1e-2 if edge == 'jitter2' else 1e-3) * z2.reshape(B, C, D)).reshape(B * C, D)
    return z1.contiguous(), z2.contiguous()


def run_loss(loss_fn, z1, z2, dtype):
    a = z1.to(dtype).clone().requires_grad_(True)
    b = z2.to(dtype).clone().requires_grad_(True)
    loss = loss_fn(a, b)
    loss.backward()
    return loss.detach().numpy().copy(), a.grad.numpy().copy(), b.grad.numpy().copy()


def errors32(r32, r64):
    """(loss, dz1, dz2) errors of fp32 results against fp64 ones: the loss relative to max(|loss|, 1), a gradient's max norm relative to
    its largest entry"""
    out = [abs(float(r32[0]) - float(r64[0])) / max(abs(float(r64[0])), 1.0)]
    for x, y in zip(r32[1:], r64[1:]):
        out.append(float(np.abs(x.astype(np.float64) - y).max() / max(np.abs(y).max(), 1e-30)))
    return out


def e2e_molecules():
    mols = G.synth.make_dataset(E2E_MOLS, seed=71)
    rng = np.random.default_rng(17)
    return mols, [G.synth.conformers(m, rng, E2E_CONF, E2E_NOISE) for m in mols]


def main():
    dgl, PNA, _, Net3D, _, _ = G.import_reference()
    sys.modules.setdefault('torch_geometric', types.ModuleType('torch_geometric'))    # custom_collate.py:6 (unused here)
    pkg = types.ModuleType('datasets')                                                 # bypass datasets/__init__.py
    pkg.__path__ = [os.path.join(G.REF, 'datasets')]
    sys.modules['datasets'] = pkg
    import commons.losses as ref_losses
    from datasets.custom_collate import conformer_collate
    M = GK.import_reference_metrics()

    def store(out, p, r32, r64):
        out.update({p + 'loss32': r32[0], p + 'dz1_32': r32[1], p + 'dz2_32': r32[2],
                    p + 'loss64': r64[0], p + 'dz1_64': r64[1], p + 'dz2_64': r64[2]})
        e = errors32(r32, r64)
        print(f'{p} loss {float(r64[0]):.6f} (fp32 {float(r32[0]):.6f}) fp32 against fp64: loss {e[0]:.2e} dz1 {e[1]:.2e} dz2 {e[2]:.2e}')

    lik, jsd = {}, {}
    for shape, edge in LIK_CASES:
        tag = case_tag(shape, edge)
        z1, z2 = case_inputs(shape, edge)
        lik[f'in/{tag}/z1'], lik[f'in/{tag}/z2'] = z1.numpy(), z2.numpy()
        for tau in TAUS:
            fn = ref_losses.NTXentLikelihoodLoss(tau=tau)
            store(lik, f'lik/{tag}/t{tau}/', run_loss(fn, z1, z2, torch.float32), run_loss(fn, z1, z2, torch.float64))
        p = f'metrics/{tag}/'
        lik[p + 'positive_prob'] = np.float64(M.PositiveProb()(z1.double(), z2.double()).item())
        lik[p + 'negative_prob'] = np.float64(M.NegativeProb()(z1.double(), z2.double()).item())
        print(p, float(lik[p + 'positive_prob']), float(lik[p + 'negative_prob']))
    for shape, edge in JSD_CASES:
        tag = case_tag(shape, edge)
        z1, z2 = case_inputs(shape, edge)
        jsd[f'in/{tag}/z1'], jsd[f'in/{tag}/z2'] = z1.numpy(), z2.numpy()
        for norm in (False, True):
            fn = ref_losses.JSDMultiplePositivesLoss(norm=norm)
            store(jsd, f'jsd/{tag}/n{int(norm)}/', run_loss(fn, z1, z2, torch.float32), run_loss(fn, z1, z2, torch.float64))

    mols, confs = e2e_molecules()
    e2e = dict(G.mols_to_npz(mols, prefix='e2e/mol'))
    e2e['e2e/conf_coords'] = np.concatenate([c for cs in confs for c in cs])          # molecule major, conformer minor

    def graph2d(m):
        g = dgl.graph((torch.from_numpy(m.src), torch.from_numpy(m.dst)), num_nodes=m.n_atoms)
        g.ndata['feat'] = torch.from_numpy(m.atom_feat)
        g.edata['feat'] = torch.from_numpy(m.bond_feat)
        return g

    def graph3d(m, xyz, dtype):
        s, d = G.synth.complete_graph_edges(m.n_atoms)
        g = dgl.graph((torch.from_numpy(s), torch.from_numpy(d)), num_nodes=m.n_atoms)
        g.edata['d'] = torch.from_numpy(G.synth.pairwise_distances(xyz, s, d)).to(dtype)
        return g

    def run_e2e(dtype):
        """the same fp32 weights and fp32 inputs, the reference computing in `dtype`"""
        torch.manual_seed(655)
        pna = PNA(avg_d=1.0, device='cpu', **PNA_KW)
        net = Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_KW)
        G.make_trained_like(pna, 31)
        G.make_trained_like(net, 37)
        sd = {**G.sd_np(pna, 'e2e/pna_sd'), **G.sd_np(net, 'e2e/net3d_sd')}
        pna.to(dtype).train(), net.to(dtype).train()
        items = [(graph2d(m), dgl.batch([graph3d(m, c, dtype) for c in cs])) for m, cs in zip(mols, confs)]
        (bg,), (bgc,) = conformer_collate(items)
        z1, z2 = pna(bg), net(bgc)
        loss = ref_losses.NTXentLikelihoodLoss(tau=E2E_TAU, conformer_variance_reg=E2E_CONF_REG)(z1, z2)
        loss.backward()
        res = {'e2e/loss': np.array(loss.item()), 'e2e/z1': z1.detach().numpy(), 'e2e/z2': z2.detach().numpy(),
               **G.grads_np(pna, 'e2e/pna_grad'), **G.grads_np(net, 'e2e/net3d_grad')}
        return sd, res

    sd, r64 = run_e2e(torch.float64)
    _, r32 = run_e2e(torch.float32)
    e2e.update(sd)
    e2e.update(r64)
    print(f'e2e loss {float(r64["e2e/loss"]):.7f} (fp32 {float(r32["e2e/loss"]):.7f}) log-variance: min '
          f'{r64["e2e/z1"][:, E2E_DIM:].min():.3f} max {r64["e2e/z1"][:, E2E_DIM:].max():.3f}')
    # the yardstick has to hold for the reference itself: its fp32 gradients against its fp64 ones under the rule of helpers.grads_close
    # (rtol 5e-4), at most a quarter of the bound
    for tag in ('e2e/pna_grad/', 'e2e/net3d_grad/'):
        keys = [k for k in r64 if k.startswith(tag)]
        scale = max(np.abs(r64[k]).max() for k in keys)
        worst = 0.0
        for k in keys:
            bmax = np.abs(r64[k]).max()
            bound = 5e-4 * bmax + (5e-5 if bmax < 1e-4 * scale else 5e-6) * scale
            worst = max(worst, np.abs(r32[k].astype(np.float64) - r64[k]).max() / bound)
        print(f'{tag} reference fp32 against fp64: worst error / bound of grads_close(5e-4) = {worst:.3f}')
        assert worst <= 0.25, (tag, worst)
    for key, out in (('lik', lik), ('jsd', jsd), ('e2e', e2e)):
        path = os.path.join(HERE, FILES[key])
        np.savez_compressed(path, **out)
        print('wrote', FILES[key], os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < 2 ** 20


if __name__ == '__main__':
    main()
