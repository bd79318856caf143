"""Training-step time of the GIN + virtual-node baseline (configs/26.yml sizes: OGBGNN hidden 300, 5 layers, virtual node, L1 loss,
Adam) on one MI355X, and the message kernels of csrc/gin.hip on their own.

Two forms of the same step on the same device, batch and weights:
  hip    the package's OGBGNN (HIP kernels end to end)
  eager  a torch-eager composition of the same arithmetic with the same parameters: nn.Embedding sums, [E, H] bond embeddings,
         x[src] gather, relu, index_add, the nn.Sequential / nn.BatchNorm1d forwards of the module's own containers
The conv lines time i3d_gin_conv_fwd / i3d_gin_conv_bwd alone with HIP events around `--conv-iters` back-to-back calls (after a
warm-up), on the batch's graph at H = 300, with the bytes the algorithm has to move (x, z / g, dx rows once, the gathered rows
once per edge, the index arrays) over that time.  Prints one JSON line per measurement and writes them to --out.

    python tools/gin_bench.py --batches 32 512 --steps 50 --warmup 10 --out profiles/gin_bench.txt
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module('3dinfomax_amd')
ops = importlib.import_module('3dinfomax_amd.ops')
gin = importlib.import_module('3dinfomax_amd.gin')

MODEL = dict(target_dim=1, hidden_dim=300, num_layers=5, virtual_node=True)


def eager_forward(model, g):
    """reference models/gin.py composed from torch ops on the module's own parameter containers"""
    node = model.node_gnn
    src, dst = g.edges()
    bnn = g.batch_num_nodes()
    B, N = bnn.shape[0], g.number_of_nodes()
    batch_id = torch.repeat_interleave(torch.arange(B, device=src.device), bnn)
    atom, bond = g.ndata['feat'], g.edata['feat']
    h = sum(emb(atom[:, k]) for k, emb in enumerate(node.atom_encoder.atom_embedding_list))
    vn = node.virtualnode_embedding(torch.zeros(B, dtype=torch.long, device=src.device))
    L = node.num_layers
    for layer in range(L):
        conv = node.convs[layer]
        x = h + vn[batch_id]
        e = sum(emb(bond[:, k]) for k, emb in enumerate(conv.bond_encoder.bond_embedding_list))
        agg = torch.zeros_like(x).index_add(0, dst, F.relu(x[src] + e))
        h = node.batch_norms[layer](conv.mlp((1 + conv.eps) * x + agg))
        if layer < L - 1:
            h = F.relu(h)
            pooled = torch.zeros(B, x.shape[1], device=x.device).index_add(0, batch_id, x) + vn
            vn = node.mlp_virtualnode_list[layer](pooled)
    pooled = torch.zeros(B, h.shape[1], device=h.device).index_add(0, batch_id, h)
    return model.graph_pred_linear(pooled)


def run(form, B, steps, warmup, dev):
    mols = amd.synth.make_dataset(B, seed=B)
    g = amd.batch([amd.bond_graph(m) for m in mols]).to(dev)
    torch.manual_seed(0)
    model = amd.OGBGNN(**MODEL).to(dev).train()
    target = torch.randn(B, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    opt = amd.Adam(model.parameters(), lr=1e-3)
    loss_fn = torch.nn.L1Loss()

    def step():
        opt.zero_grad(set_to_none=True)
        y = model(g) if form == 'hip' else eager_forward(model, g)
        loss = loss_fn(y, target)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return dict(what='step', form=form, batch=B, atoms=int(g.number_of_nodes()), edges=int(g.number_of_edges()), steps=steps,
                warmup=warmup, ms_per_step=round(ms, 4), molecules_per_s=round(B / ms * 1e3, 1), last_loss=float(loss.item()),
                device=torch.cuda.get_device_name(dev))


def conv_alone(B, iters, warmup, dev, H=300):
    mols = amd.synth.make_dataset(B, seed=B)
    g = amd.batch([amd.bond_graph(m) for m in mols]).to(dev)
    ec = gin.edge_context(g, list(amd.synth.BOND_FEATURE_DIMS))
    idx = ec.index
    N, E, V = idx.num_nodes, idx.num_edges, ec.num_codes
    gen = torch.Generator().manual_seed(B)
    h, vn = torch.randn(N, H, generator=gen).to(dev), torch.randn(idx.num_graphs, H, generator=gen).to(dev)
    T, go = torch.randn(V, H, generator=gen).to(dev), torch.randn(N, H, generator=gen).to(dev)
    eps = torch.tensor([0.1], device=dev)

    def fwd():
        return ops.gin_conv_fwd(h, vn, idx.graph_ptr, idx.num_graphs, T, ec.codes, idx.in_ptr, idx.src_s, eps)

    x, _ = fwd()

    def bwd():
        return ops.gin_conv_bwd(go, x, T, ec.codes, idx.src_s, idx.dst_s, idx.out_ptr, idx.out_epos, ec.code_order, ec.code_ptr, eps)

    out = []
    # bytes the algorithm moves: node rows read and written once, one gathered node row and one table row per edge, the index arrays
    row = 4 * H
    need = {'fwd': (3 * N + 2 * E) * row + 4 * (2 * E + N), 'bwd': (3 * N + 2 * E) * row + (3 * E) * row + 4 * (6 * E + 2 * N)}
    for name, fn in (('fwd', fwd), ('bwd', bwd)):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        us = a.elapsed_time(b) * 1e3 / iters
        out.append(dict(what='conv_' + name, batch=B, atoms=N, edges=E, feat=H, iters=iters, us_per_call=round(us, 2),
                        algorithm_bytes=need[name], gbytes_per_s=round(need[name] / us / 1e3, 1),
                        note='back-to-back calls between two HIP events: includes the launch gaps and the output allocations',
                        device=torch.cuda.get_device_name(dev)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[32, 512])
    ap.add_argument('--forms', nargs='+', default=['hip', 'eager'], choices=['hip', 'eager'])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--conv-iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    lines = []
    for B in a.batches:
        for form in a.forms:          # both forms of one batch size back to back
            lines.append(run(form, B, a.steps, a.warmup, dev))
            print(json.dumps(lines[-1]), flush=True)
        for r in conv_alone(B, a.conv_iters, a.warmup, dev):
            lines.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
