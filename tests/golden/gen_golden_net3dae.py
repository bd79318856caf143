"""Fixture of the 3D autoencoder pre-training (reference models/net3d_VAE.py Net3DAE, commons/losses.py NTXentAE,
datasets/custom_collate.py contrastive_vae_collate): the unmodified reference classes on seeded synthetic molecules, forward + both
loss terms + backward of their sum -> tests/golden/net3dae.npz.

    python tests/golden/gen_golden_net3dae.py          (imports the reference checkout, as gen_golden.py does)

Per configuration: the molecules, the collate output (pairwise_indices, distances), the state_dict and the ordered list of its keys,
the seeded 2D embedding z1, latent vector and predicted distances, both loss terms, ndata['feat'], every parameter's gradient of the
summed loss, the buffers after the step.

Three configurations: 'a' the shape of configs/contrastive_training_Net3DAE.yml (encoder only, distance_net of two layers); 'b' one
encoder and two decoder layers with the same head; 'c' Euclidean distances of a 3-wide node projection behind one encoder and one
decoder layer.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

COMMON = dict(node_dim=0, edge_dim=1, hidden_dim=16, readout_aggregators=['min', 'max', 'mean'], batch_norm=True,
              batch_norm_momentum=0.1, reduce_func='mean', dropout=0.0, fourier_encodings=4, activation='SiLU', update_net_layers=1,
              message_net_layers=1, use_node_features=False, node_wise_encoder_layers=0, node_wise_output_layers=0)
CONFIGS = {
    'a': dict(COMMON, encoder_depth=2, decoder_depth=0, distance_net=True, projection_dim=16, projection_layers=2),
    'b': dict(COMMON, encoder_depth=1, decoder_depth=2, distance_net=True, projection_dim=16, projection_layers=2),
    'c': dict(COMMON, encoder_depth=1, decoder_depth=1, distance_net=False, projection_dim=3, projection_layers=1),
}
LOSS = dict(norm=True, tau=0.1, reconstruction_reg=1)


def molecules(cfg):
    return G.synth.make_dataset(6, seed=41)


def items_of(mols, graph2d, graph3d):
    """(graph, graph3d, pairwise_indices [2, p], distances [p, 1]) per molecule: the pairs are the complete graph's edges"""
    items = []
    for m in mols:
        s, d = G.synth.complete_graph_edges(m.n_atoms)
        dist = torch.from_numpy(G.synth.pairwise_distances(m.coords, s, d))
        items.append((graph2d(m), graph3d(m, s, d, dist), torch.stack([torch.from_numpy(s), torch.from_numpy(d)]), dist.clone()))
    return items


def main():
    dgl = G.import_reference()[0]
    sys.modules.setdefault('torch_geometric', types.ModuleType('torch_geometric'))    # custom_collate.py:6 (unused here)
    pkg = types.ModuleType('datasets')                                                 # bypass datasets/__init__.py
    pkg.__path__ = [os.path.join(G.REF, 'datasets')]
    sys.modules['datasets'] = pkg
    from models.net3d_VAE import Net3DAE
    from commons.losses import NTXentAE
    from datasets.custom_collate import contrastive_vae_collate

    def graph2d(m):
        g = dgl.graph((torch.from_numpy(m.src), torch.from_numpy(m.dst)), num_nodes=m.n_atoms)
        g.ndata['feat'] = torch.from_numpy(m.atom_feat)
        g.edata['feat'] = torch.from_numpy(m.bond_feat)
        return g

    def graph3d(m, s, d, dist):
        g = dgl.graph((torch.from_numpy(s), torch.from_numpy(d)), num_nodes=m.n_atoms)
        g.ndata['feat'] = torch.from_numpy(m.atom_feat)
        g.edata['d'] = dist.clone()
        return g

    out = {}
    for cfg, kw in CONFIGS.items():
        mols = molecules(cfg)
        (bg,), (bg3, pidx), dist = contrastive_vae_collate(items_of(mols, graph2d, graph3d))
        torch.manual_seed(7)
        model = Net3DAE(**kw)
        G.make_trained_like(model, 17)
        model.train()
        latent_dim = kw['hidden_dim'] * len(kw['readout_aggregators'])
        z1 = torch.randn(len(mols), latent_dim, generator=torch.Generator().manual_seed(23))
        p = f'{cfg}/'
        out.update(G.mols_to_npz(mols, prefix=p + 'mol'))
        out.update(G.sd_np(model, p + 'sd'))
        out[p + 'sd_keys'] = np.array(list(model.state_dict().keys()))
        out[p + 'pidx'], out[p + 'dist'], out[p + 'z1'] = pidx.numpy(), dist.numpy(), z1.numpy()
        latent, pred = model(bg3, pidx)
        contrastive, recon = NTXentAE(**LOSS)(z1, latent, dist, pred)
        (contrastive + recon).backward()
        out[p + 'latent'], out[p + 'pred'], out[p + 'feat'] = latent.detach().numpy(), pred.detach().numpy(), bg3.ndata['feat'].detach().numpy()
        out[p + 'contrastive'], out[p + 'recon'] = np.array(contrastive.item()), np.array(recon.item())
        out.update({f'{p}grad/{k}': q.grad.numpy().copy() for k, q in model.named_parameters() if q.grad is not None})
        out.update({f'{p}buf_after/{k}': v.numpy().copy() for k, v in model.named_buffers()})
        print(cfg, 'atoms', [m.n_atoms for m in mols], 'pairs', pidx.shape[1], 'losses', contrastive.item(), recon.item())
    path = os.path.join(HERE, 'net3dae.npz')
    np.savez_compressed(path, **out)
    print('wrote net3dae.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
