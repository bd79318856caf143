"""Fixture of the conformer-wise multi-positive losses (reference commons/losses.py NTXentMultiplePositivesSeparate2D :692-744 and
NTXentMMDSeparate2D :394-476): the unmodified reference classes on seeded inputs -> tests/golden/separate2d.npz.

    python tests/golden/gen_golden_separate2d.py          (imports the reference checkout, as gen_golden.py does)

Loss level, per loss ('sep', 'mmd') and case: z1 [B, C D], z2 [B C, D] (fp32), and the reference's loss, dz1 and dz2 computed in fp32
('loss32', 'dz1_32', 'dz2_32') and in fp64 on the same inputs ('loss64', ...).  tau = 0.1 as in both configs
(configs/contrastive_training_multiple_positives_separate2d.yml, ..._mmd_loss.yml), everything else at the constructor defaults.
Cases (B, C, D): (2, 1, 8), (5, 3, 24), (7, 5, 40), (3, 2, 7) with standard normal entries, and '5x3x24j': every conformer of both
views of a molecule is that molecule's base vector + 1e-2 noise (near-coincident points, exp(S / tau) at its largest).

End to end ('e2e/...'): 4 synthetic molecules x 2 conformers through the reference PNA (hidden 16, target_dim 2 * 8, depth 2) and
Net3D (hidden 8, target_dim 8) batched by the reference's conformer_collate; per loss the loss, both embeddings and every parameter
gradient.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

TAU = 0.1
CASES = [(2, 1, 8), (5, 3, 24), (7, 5, 40), (3, 2, 7)]
JITTER_CASE = (5, 3, 24)
LOSSES = {'sep': 'NTXentMultiplePositivesSeparate2D', 'mmd': 'NTXentMMDSeparate2D'}
E2E_MOLS, E2E_CONF, E2E_DIM = 4, 2, 8
PNA_KW = dict(G.PNA_YML, hidden_dim=16, target_dim=E2E_CONF * E2E_DIM, propagation_depth=2, readout_hidden_dim=16)
NET3D_KW = dict(G.NET3D_YML, hidden_dim=8, hidden_edge_dim=8, readout_hidden_dim=8, target_dim=E2E_DIM)


def case_tag(B, C, D, jitter=False):
    return f'{B}x{C}x{D}' + ('j' if jitter else '')


def case_inputs(B, C, D, jitter=False):
    g = torch.Generator().manual_seed(1000 * B + 10 * C + D + (7 if jitter else 0))
    if jitter:
        base = torch.randn(B, 1, D, generator=g)
        z1 = (base + 1e-2 * torch.randn(B, C, D, generator=g)).reshape(B, C * D)
        z2 = (base + 1e-2 * torch.randn(B, C, D, generator=g)).reshape(B * C, D)
    else:
        z1, z2 = torch.randn(B, C * D, generator=g), torch.randn(B * C, D, generator=g)
    return z1.contiguous(), z2.contiguous()


def run_loss(cls, z1, z2, dtype):
    a = z1.to(dtype).clone().requires_grad_(True)
    b = z2.to(dtype).clone().requires_grad_(True)
    loss = cls(tau=TAU)(a, b)
    loss.backward()
    return loss.detach().numpy().copy(), a.grad.numpy().copy(), b.grad.numpy().copy()


def e2e_molecules():
    mols = G.synth.make_dataset(E2E_MOLS, seed=61)
    rng = np.random.default_rng(9)
    return mols, [G.synth.conformers(m, rng, E2E_CONF) for m in mols]


def main():
    dgl, PNA, _, Net3D, _, _ = G.import_reference()
    sys.modules.setdefault('torch_geometric', types.ModuleType('torch_geometric'))    # custom_collate.py:6 (unused here)
    pkg = types.ModuleType('datasets')                                                 # bypass datasets/__init__.py
    pkg.__path__ = [os.path.join(G.REF, 'datasets')]
    sys.modules['datasets'] = pkg
    import commons.losses as ref_losses
    from datasets.custom_collate import conformer_collate

    out = {}
    for key, name in LOSSES.items():
        cls = getattr(ref_losses, name)
        for (B, C, D), jitter in [(c, False) for c in CASES] + [(JITTER_CASE, True)]:
            z1, z2 = case_inputs(B, C, D, jitter)
            p = f'{key}/{case_tag(B, C, D, jitter)}/'
            out[p + 'z1'], out[p + 'z2'] = z1.numpy(), z2.numpy()
            l32, a32, b32 = run_loss(cls, z1, z2, torch.float32)
            l64, a64, b64 = run_loss(cls, z1, z2, torch.float64)
            out.update({p + 'loss32': l32, p + 'dz1_32': a32, p + 'dz2_32': b32, p + 'loss64': l64, p + 'dz1_64': a64, p + 'dz2_64': b64})
            rel = lambda x, y: float(np.abs(x.astype(np.float64) - y).max() / max(np.abs(y).max(), 1e-30))
            print(f'{p} loss {float(l64):.6f} fp32 against fp64: loss {rel(l32, l64):.2e} dz1 {rel(a32, a64):.2e} dz2 {rel(b32, b64):.2e}')

    mols, confs = e2e_molecules()
    out.update(G.mols_to_npz(mols, prefix='e2e/mol'))
    out['e2e/conf_coords'] = np.concatenate([c for cs in confs for c in cs])          # molecule major, conformer minor

    def graph2d(m):
        g = dgl.graph((torch.from_numpy(m.src), torch.from_numpy(m.dst)), num_nodes=m.n_atoms)
        g.ndata['feat'] = torch.from_numpy(m.atom_feat)
        g.edata['feat'] = torch.from_numpy(m.bond_feat)
        return g

    def graph3d(m, xyz):
        s, d = G.synth.complete_graph_edges(m.n_atoms)
        g = dgl.graph((torch.from_numpy(s), torch.from_numpy(d)), num_nodes=m.n_atoms)
        g.edata['d'] = torch.from_numpy(G.synth.pairwise_distances(xyz, s, d))
        return g

    for key, name in LOSSES.items():
        torch.manual_seed(321)
        pna = PNA(avg_d=1.0, device='cpu', **PNA_KW)
        net = Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_KW)
        G.make_trained_like(pna, 17)
        G.make_trained_like(net, 19)
        pna.train(), net.train()
        if key == 'sep':
            out.update(G.sd_np(pna, 'e2e/pna_sd'))
            out.update(G.sd_np(net, 'e2e/net3d_sd'))
        items = [(graph2d(m), dgl.batch([graph3d(m, c) for c in cs])) for m, cs in zip(mols, confs)]
        (bg,), (bgc,) = conformer_collate(items)
        z1, z2 = pna(bg), net(bgc)
        loss = getattr(ref_losses, name)(tau=TAU)(z1, z2)
        loss.backward()
        p = f'e2e/{key}/'
        out[p + 'loss'], out[p + 'z1'], out[p + 'z2'] = np.array(loss.item()), z1.detach().numpy(), z2.detach().numpy()
        out.update(G.grads_np(pna, p + 'pna_grad'))
        out.update(G.grads_np(net, p + 'net3d_grad'))
        print(p, 'loss', loss.item(), 'z1', tuple(z1.shape), 'z2', tuple(z2.shape))
    path = os.path.join(HERE, 'separate2d.npz')
    np.savez_compressed(path, **out)
    print('wrote separate2d.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
