"""Fixture of the GIN + virtual-node baseline (reference models/gin.py): the unmodified reference OGBGNN on seeded synthetic molecules,
forward + loss + backward -> tests/golden/ogbgnn.npz (molecules, state_dict, output, final node representation, loss, every
parameter's gradient, the buffers after the step, and the fp32 reference's own error against an fp64 run of itself).

    python tests/golden/gen_golden_gin.py          (imports the reference checkout, as gen_golden.py does)

Four configurations at hidden_dim 16, num_layers 3, on five QM9-like molecules plus one QMugs-like molecule above 64 atoms and one
single-atom molecule (no edges): 'a' virtual node, JK last, sum pooling, target_dim 8 (loss: mean of the outputs squared); 'b' no
virtual node, residual, mean pooling, JK sum; 'c' virtual node + residual, target_dim 1; 'd' as 'a' in eval mode after one
training step (SGD, lr 1e-4).

'b' at dropout 0 cannot be back-propagated by the reference as it stands: F.dropout(h, 0) returns its input, and GNN_node's in-place
`h += h_list[layer]` (models/gin.py:198) then overwrites the ReLU output its backward needs.  For 'b' alone F.dropout is wrapped to
return a copy (what it does for any p > 0): the same numbers, a gradient that exists.  models/gin.py itself is not touched.

ref_err of a gradient = max |fp32 - fp64| / max(max |fp64|, 1e-4 x the largest gradient of the set): analytically-zero gradients (a
bias in front of a BatchNorm) are rounding noise on both sides and would otherwise give a meaningless ratio.

The reference needs more of ogb and DGL than tests/golden/_stubs carries; the stand-ins for those parts are registered here, written
from the libraries' documented semantics:
  ogb.graphproppred.mol_encoder   AtomEncoder / BondEncoder: one xavier-initialised nn.Embedding per feature column, summed
  dgl.nn.pytorch                  SumPooling / AvgPooling: per-graph sum / mean of node rows; the other poolings by name only
  dgl.broadcast_nodes             a per-graph row repeated for every node of the graph
  dgl.function.copy_e             message = an edge feature
  DGLGraph.local_scope            frames restored on exit;  DGLGraph.batch_size = number of graphs
"""
import contextlib
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

BASE = dict(hidden_dim=16, num_layers=3, dropout=0.0, gnn_type='gin', batch_norm_momentum=0.1)
CONFIGS = {
    'a': dict(BASE, virtual_node=True, JK='last', graph_pooling='sum', target_dim=8, residual=False),
    'b': dict(BASE, virtual_node=False, JK='sum', graph_pooling='mean', target_dim=4, residual=True, batch_norm_momentum=0.3),
    'c': dict(BASE, virtual_node=True, JK='last', graph_pooling='sum', target_dim=1, residual=True, batch_norm_momentum=0.3),
    'd': dict(BASE, virtual_node=True, JK='last', graph_pooling='sum', target_dim=8, residual=False),
}
SEEDS = {'a': 61, 'b': 62, 'c': 63, 'd': 61}


def register_stand_ins(dgl):
    synth = G.synth

    class _Encoder(torch.nn.Module):
        def __init__(self, dims, emb_dim, name):
            super().__init__()
            lst = torch.nn.ModuleList()
            for d in dims:
                emb = torch.nn.Embedding(d, emb_dim)
                torch.nn.init.xavier_uniform_(emb.weight.data)
                lst.append(emb)
            setattr(self, name, lst)
            self._name = name

        def forward(self, x):
            out = 0
            for i, emb in enumerate(getattr(self, self._name)):
                out = out + emb(x[:, i])
            return out

    class AtomEncoder(_Encoder):
        def __init__(self, emb_dim):
            super().__init__(synth.ATOM_FEATURE_DIMS, emb_dim, 'atom_embedding_list')

    class BondEncoder(_Encoder):
        def __init__(self, emb_dim):
            super().__init__(synth.BOND_FEATURE_DIMS, emb_dim, 'bond_embedding_list')

    import ogb
    gp = types.ModuleType('ogb.graphproppred')
    me = types.ModuleType('ogb.graphproppred.mol_encoder')
    me.AtomEncoder, me.BondEncoder = AtomEncoder, BondEncoder
    gp.mol_encoder = me
    ogb.graphproppred = gp
    sys.modules['ogb.graphproppred'] = gp
    sys.modules['ogb.graphproppred.mol_encoder'] = me

    def _segments(g, feat):
        return torch.split(feat, g.batch_num_nodes().tolist())

    class SumPooling(torch.nn.Module):
        def forward(self, g, feat):
            return torch.stack([s.sum(0) for s in _segments(g, feat)])

    class AvgPooling(torch.nn.Module):
        def forward(self, g, feat):
            return torch.stack([s.mean(0) for s in _segments(g, feat)])

    nn_mod = types.ModuleType('dgl.nn')
    pt = types.ModuleType('dgl.nn.pytorch')
    pt.SumPooling, pt.AvgPooling = SumPooling, AvgPooling
    for name in ('MaxPooling', 'GlobalAttentionPooling', 'Set2Set'):
        setattr(pt, name, type(name, (torch.nn.Module,), {}))
    nn_mod.pytorch = pt
    dgl.nn = nn_mod
    sys.modules['dgl.nn'] = nn_mod
    sys.modules['dgl.nn.pytorch'] = pt

    dgl.broadcast_nodes = lambda g, t: torch.repeat_interleave(t, g.batch_num_nodes().to(t.device), dim=0)
    dgl.function.copy_e = lambda e, out: (lambda edges: {out: edges.data[e]})

    @contextlib.contextmanager
    def local_scope(self):
        nd, ed = dict(self.ndata), dict(self.edata)
        try:
            yield
        finally:
            self.ndata.clear(), self.ndata.update(nd)
            self.edata.clear(), self.edata.update(ed)

    dgl.DGLGraph.local_scope = local_scope
    dgl.DGLGraph.batch_size = property(lambda self: int(self.batch_num_nodes().shape[0]))


def molecules(seed):
    mols = G.synth.make_dataset(5, seed=seed)
    rng = np.random.default_rng(seed + 100)
    big = next(m for m in (G.synth.qmugs_like(rng) for _ in range(200)) if m.n_atoms > 64)
    m0 = mols[0]
    single = G.synth.Molecule(1, np.zeros(0, np.int64), np.zeros(0, np.int64), m0.atom_feat[:1].copy(),
                              np.zeros((0, 3), np.int64), m0.coords[:1].copy())
    return mols[:2] + [big] + mols[2:4] + [single] + mols[4:]


def make_trained_like(model, seed):
    """O(1) pre-BatchNorm scale, random BatchNorm affine, non-zero biases, distinct non-zero eps per layer, a non-zero virtual-node
    embedding (the reference's zero initialisation would hide both the eps and the virtual-node paths)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / np.sqrt(m.weight.shape[1]))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
            elif isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(1 + torch.randn(m.weight.shape, generator=g) * 0.2)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
        for l, conv in enumerate(model.node_gnn.convs):
            conv.eps.fill_((0.15 + 0.1 * l) * (-1) ** l)
        if hasattr(model.node_gnn, 'virtualnode_embedding'):
            w = model.node_gnn.virtualnode_embedding.weight
            w.copy_(torch.randn(w.shape, generator=g) * 0.5)


def graph_of(dgl, mols):
    gs = []
    for m in mols:
        g = dgl.graph((torch.from_numpy(m.src), torch.from_numpy(m.dst)), num_nodes=m.n_atoms)
        g.ndata['feat'] = torch.from_numpy(m.atom_feat)
        g.edata['feat'] = torch.from_numpy(m.bond_feat)
        gs.append(g)
    return dgl.batch(gs)


@contextlib.contextmanager
def dropout_returns_copy():
    F = torch.nn.functional
    orig = F.dropout
    F.dropout = lambda x, p=0.5, training=True, inplace=False: orig(x, p, training, inplace).clone()
    try:
        yield
    finally:
        F.dropout = orig


def run(model, bg, cfg, target):
    """-> output, node representation, loss (after backward)"""
    feat = []
    hook = model.node_gnn.register_forward_hook(lambda mod, args, out: feat.append(out.detach().clone()))
    with (dropout_returns_copy() if cfg == 'b' else contextlib.nullcontext()):
        y = model(bg)
    hook.remove()
    loss = (y ** 2).mean() if cfg in ('a', 'd') else torch.nn.L1Loss()(y, target.to(y.dtype))
    model.zero_grad()
    loss.backward()
    return y.detach(), feat[0], loss.detach()


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def main():
    dgl = G.import_reference()[0]
    register_stand_ins(dgl)
    from models.gin import OGBGNN
    out = {}
    for cfg, kw in CONFIGS.items():
        mols = molecules(SEEDS[cfg])
        torch.manual_seed(7)
        model = OGBGNN(**kw)
        make_trained_like(model, 17 + ord(cfg[0]) if cfg != 'd' else 17 + ord('a'))
        target = torch.randn(len(mols), kw['target_dim'], generator=torch.Generator().manual_seed(5))
        model.train()
        if cfg == 'd':      # one training step, then everything in eval mode
            opt = torch.optim.SGD(model.parameters(), lr=1e-4)
            run(model, graph_of(dgl, mols), cfg, target)
            opt.step()
            model.eval()
        p = f'{cfg}/'
        out.update(G.mols_to_npz(mols, prefix=p + 'mol'))
        out.update(G.sd_np(model, p + 'sd'))
        out[p + 'target'] = target.numpy()
        ref64 = copy.deepcopy(model).double()
        y, feat, loss = run(model, graph_of(dgl, mols), cfg, target)
        out[p + 'out'], out[p + 'feat'], out[p + 'loss'] = y.numpy(), feat.numpy(), np.array(loss.item())
        # JK 'sum' leaves the last layer's output out of the sum (models/gin.py:207): its parameters have no gradient
        out.update({f'{p}grad/{k}': q.grad.numpy().copy() for k, q in model.named_parameters() if q.grad is not None})
        out.update({f'{p}buf_after/{k}': v.numpy().copy() for k, v in model.named_buffers()})
        y64, feat64, _ = run(ref64, graph_of(dgl, mols), cfg, target)
        out[p + 'ref_err/out'] = np.array(rel_err(y, y64))
        out[p + 'ref_err/feat'] = np.array(rel_err(feat, feat64))
        g64 = dict(ref64.named_parameters())
        worst = 0.0
        scale = max(float(q.grad.abs().max()) for q in g64.values() if q.grad is not None)
        for k, q in model.named_parameters():
            if q.grad is None:
                continue
            e = float((q.grad.double() - g64[k].grad).abs().max() / max(float(g64[k].grad.abs().max()), 1e-4 * scale))
            out[f'{p}ref_err/grad/{k}'] = np.array(e)
            worst = max(worst, e)
        print(cfg, 'atoms', [m.n_atoms for m in mols], 'loss', loss.item(), 'ref_err out', float(out[p + 'ref_err/out']),
              'worst grad ref_err', worst)
    path = os.path.join(HERE, 'ogbgnn.npz')
    np.savez_compressed(path, **out)
    print('wrote ogbgnn.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
