"""Training-step time of the SAN baseline (configs/san_ogbg.yml: 10 layers, H 64, 4 heads, full graph, learned encoding of 3 layers)
on one MI355X, fused attention (csrc/san.hip) against the composed path (san.FUSED_ATTENTION = False: the reference's per-edge
tensors in torch ops, every other block the package's kernels), and the attention launches on their own.

One batch of --molecules drug-sized synthetic molecules (synth.qmugs_like) as complete graphs (graph.san_graph), the same weights
for both forms.  The two forms ALTERNATE inside one call: --rounds times (fused for --steps steps, composed for --steps steps),
each block after its own warm-up and closed by a device synchronise; the per-round times are printed so that the spread is
visible beside the difference.  The attention lines time ops.san_attn_fwd / ops.san_attn_bwd alone between two HIP events
around --attn-iters back-to-back calls, on the batch's graph, with the bytes the algorithm has to move (per edge and direction:
the gathered K, V and table rows, the index entries and the per-head floats; per node: the projections and the output) over
that time.  Prints one JSON line per measurement and writes them to --out.

    python tools/san_bench.py --out profiles/san_bench.txt
"""
import argparse
import copy
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module('3dinfomax_amd')
ops = importlib.import_module('3dinfomax_amd.ops')
san = importlib.import_module('3dinfomax_amd.san')

MODEL = dict(target_dim=1, in_feat_dropout=0.0, layer_norm=False, batch_norm=True, gamma=1e-6, full_graph=True, GT_hidden_dim=64,
             GT_n_heads=4, GT_out_dim=64, GT_layers=10, LPE_n_heads=4, LPE_layers=3, LPE_dim=16, dropout=0.01, batch_norm_momentum=0.1,
             readout_batchnorm=True, readout_hidden_dim=90, readout_layers=2, readout_aggregators=['min', 'max', 'mean', 'sum'],
             residual=True)


def make_batch(n_mol, dev):
    rng = np.random.default_rng(n_mol)
    mols = [amd.synth.qmugs_like(rng) for _ in range(n_mol)]
    return amd.batch([amd.san_graph(m) for m in mols]).to(dev)


def steps_of(model, opt, g, target, fused, steps, dev):
    san.FUSED_ATTENTION = fused
    loss_fn = torch.nn.L1Loss()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(model(g.local_copy()), target)
        loss.backward()
        opt.step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / steps, float(loss.item())


def attention_alone(g, iters, warmup, dev, H=64, nh=4, gamma=1e-6):
    ec = san.edge_context(g, list(amd.synth.BOND_FEATURE_DIMS), True)
    idx = ec.index
    N, E, V = idx.num_nodes, idx.num_edges, ec.comb.shape[0]
    gen = torch.Generator().manual_seed(E)
    Y = (torch.randn(N, 5 * H, generator=gen) * 0.5).to(dev)
    te, te2 = (torch.randn(V, H, generator=gen) * 0.5).to(dev), (torch.randn(V, H, generator=gen) * 0.5).to(dev)
    go = torch.randn(N, H, generator=gen).to(dev)

    def fwd():
        return ops.san_attn_fwd(Y, te, te2, ec.codes, ec.real, idx.in_ptr, idx.src_s, nh, gamma, True)

    out, s, z = fwd()

    def bwd():
        return ops.san_attn_bwd(go, out, z, s, Y, te, te2, ec.codes, ec.real, idx, ec.code_order, ec.code_ptr, nh, gamma, True)

    row = 4 * H
    need = {'fwd': 3 * E * row + E * (9 + 4 * nh) + N * (3 * row + 4 * nh),
            'bwd': (3 + 3 + 2) * E * row + E * (3 * 9 + 4 * 4 * nh + 12) + N * (10 * row + 4 * nh)}
    lines = []
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
        lines.append(dict(what='attention_' + name, atoms=N, edges=E, feat=H, heads=nh, iters=iters, us_per_call=round(us, 2),
                          algorithm_bytes=need[name], gbytes_per_s=round(need[name] / us / 1e3, 1),
                          note='back-to-back calls between two HIP events: includes the launch gaps and the output allocations; '
                               'the gathered rows mostly come from L2',
                          device=torch.cuda.get_device_name(dev)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--molecules', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--attn-iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    g = make_batch(a.molecules, dev)
    torch.manual_seed(0)
    models = {True: amd.SAN(**MODEL).to(dev).train()}
    models[False] = copy.deepcopy(models[True])
    opts = {f: amd.Adam(m.parameters(), lr=1e-4) for f, m in models.items()}
    target = torch.randn(a.molecules, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    lines = []
    for fused in (True, False):
        steps_of(models[fused], opts[fused], g, target, fused, a.warmup, dev)
    times = {True: [], False: []}
    for _ in range(a.rounds):
        for fused in (True, False):
            ms, loss = steps_of(models[fused], opts[fused], g, target, fused, a.steps, dev)
            times[fused].append(round(ms, 3))
            last = loss
            lines.append(dict(what='step', form='fused' if fused else 'composed', molecules=a.molecules, atoms=int(g.number_of_nodes()),
                              edges=int(g.number_of_edges()), steps=a.steps, ms_per_step=round(ms, 3), last_loss=last,
                              device=torch.cuda.get_device_name(dev)))
            print(json.dumps(lines[-1]), flush=True)
    san.FUSED_ATTENTION = True
    med = {f: float(np.median(t)) for f, t in times.items()}
    lines.append(dict(what='summary', fused_ms=times[True], composed_ms=times[False], fused_median_ms=med[True],
                      composed_median_ms=med[False], composed_over_fused=round(med[False] / med[True], 2)))
    print(json.dumps(lines[-1]), flush=True)
    for r in attention_alone(g, a.attn_iters, a.warmup, dev):
        lines.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
