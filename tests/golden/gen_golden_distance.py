"""Fixture of the distance-prediction baseline (reference models/distance_predictor.py, datasets/custom_collate.py:65-78): the
unmodified reference DistancePredictor and pairwise_distance_collate on seeded synthetic molecules, forward + L1 loss against the
true pair distances + backward -> tests/golden/distance_predictor.npz (collate output, state_dict, output, ndata['feat'], every
parameter's gradient, the buffers after the step).

    python tests/golden/gen_golden_distance.py          (imports the reference checkout, as gen_golden.py does)

Three configurations: 'a' the blessed head (distance_net of one Linear) behind a transformer layer, one QMugs-like molecule above
64 atoms in the batch; 'b' Euclidean distances of a 3-wide node projection, no transformer; 'c' distance_net of two layers
(BatchNorm) run on both pair orders, behind a transformer layer.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

PNA_ARGS = dict(hidden_dim=16, mid_batch_norm=True, last_batch_norm=True, batch_norm_momentum=0.1, dropout=0.0, propagation_depth=2,
                aggregators=['mean', 'max', 'min', 'std'], scalers=['identity', 'amplification', 'attenuation'],
                readout_aggregators=['min', 'max', 'mean', 'sum'], pretrans_layers=2, posttrans_layers=1, residual=True)
CONFIGS = {
    'a': dict(target_dim=1, projection_dim=0, distance_net=True, projection_layers=1, transformer_layer=True, nhead=2,
              dim_feedforward=32),
    'b': dict(target_dim=1, projection_dim=3, distance_net=False, projection_layers=1, transformer_layer=False, nhead=2,
              dim_feedforward=32),
    'c': dict(target_dim=1, projection_dim=3, distance_net=True, projection_layers=2, transformer_layer=True, nhead=2,
              dim_feedforward=32),
}


def molecules(cfg):
    mols = G.synth.make_dataset(5, seed=31)
    if cfg == 'a':
        rng = np.random.default_rng(7)
        big = [m for m in (G.synth.qmugs_like(rng) for _ in range(40)) if m.n_atoms > 64]
        mols = mols[:3] + big[:1] + mols[3:]
    return mols


def main():
    dgl = G.import_reference()[0]
    sys.modules.setdefault('torch_geometric', types.ModuleType('torch_geometric'))    # custom_collate.py:6 (unused here)
    pkg = types.ModuleType('datasets')                                                 # bypass datasets/__init__.py
    pkg.__path__ = [os.path.join(G.REF, 'datasets')]
    sys.modules['datasets'] = pkg
    from models.distance_predictor import DistancePredictor
    from datasets.custom_collate import pairwise_distance_collate
    out = {}
    for cfg, kw in CONFIGS.items():
        mols = molecules(cfg)
        items = []
        for m in mols:
            g = dgl.graph((torch.from_numpy(m.src), torch.from_numpy(m.dst)), num_nodes=m.n_atoms)
            g.ndata['feat'] = torch.from_numpy(m.atom_feat)
            g.edata['feat'] = torch.from_numpy(m.bond_feat)
            s, d = G.synth.complete_graph_edges(m.n_atoms)
            items.append((g, torch.stack([torch.from_numpy(s), torch.from_numpy(d)]),
                          torch.from_numpy(G.synth.pairwise_distances(m.coords, s, d))))
        (bg, pidx, mask), dist = pairwise_distance_collate(items)
        torch.manual_seed(5)
        model = DistancePredictor(pna_args=dict(PNA_ARGS), **kw)
        G.make_trained_like(model, 13)
        model.train()
        p = f'{cfg}/'
        out.update(G.mols_to_npz(mols, prefix=p + 'mol'))
        out.update(G.sd_np(model, p + 'sd'))
        out[p + 'pidx'], out[p + 'mask'], out[p + 'dist'] = pidx.numpy(), mask.numpy(), dist.numpy()
        y = model(bg, pidx, mask)
        loss = torch.nn.L1Loss()(y, dist)
        loss.backward()
        out[p + 'out'], out[p + 'feat'], out[p + 'loss'] = y.detach().numpy(), bg.ndata['feat'].detach().numpy(), np.array(loss.item())
        out.update({f'{p}grad/{k}': q.grad.numpy().copy() for k, q in model.named_parameters() if q.grad is not None})  # (an unused node_projection_net has none)
        out.update({f'{p}buf_after/{k}': v.numpy().copy() for k, v in model.named_buffers()})   # running statistics after the step
        print(cfg, 'atoms', [m.n_atoms for m in mols], 'pairs', pidx.shape[1], 'loss', loss.item())
    np.savez_compressed(os.path.join(HERE, 'distance_predictor.npz'), **out)
    print('wrote distance_predictor.npz', os.path.getsize(os.path.join(HERE, 'distance_predictor.npz')), 'bytes')


if __name__ == '__main__':
    main()
