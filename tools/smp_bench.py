"""Training-step time of SMP / SphereNet on one MI355X: the fused triplet step (csrc/smp.hip) against the composed torch chain
(smp.FUSED_TRIPLETS = False), and the geometry + bases stage and the triplet launches on their own.

Two models on QM9-sized synthetic molecules (synth.qm9_like): configs/sphere_net.yml (hidden 128, int_emb 64, basis_emb 8, 3
spherical, 6 radial, depth 4) at batch 32, and the 3D side of the contrastive config (num_spherical 7) at batch 500.  Forward + L1 loss
+ backward + Adam on one batch, the same weights for both forms.  The two forms ALTERNATE inside one call: --rounds times (fused for
--steps steps, composed for --steps steps), each block after its own warm-up and closed by a device synchronise; the per-round times
are printed so that the spread is visible beside the difference.  The stage lines time ops.smp_geometry + ops.smp_bases, and
ops.smp_triplets_fwd / ops.smp_triplets_bwd (against the composed chain's forward / backward on the same tensors), between two HIP
events around --iters back-to-back calls: launch gaps, allocations and (for the geometry) the two host reads included.  Prints one JSON
line per measurement and writes them to --out.

    python tools/smp_bench.py --out profiles/smp_bench.txt
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
smp = importlib.import_module('3dinfomax_amd.smp')
graph = importlib.import_module('3dinfomax_amd.graph')

BASE = dict(energy_and_force=False, cutoff=5.0, envelope_exponent=5, num_before_skip=1, num_after_skip=2, num_output_layers=3,
            hidden_channels=128, int_emb_size=64, basis_emb_size=8, out_emb_size=256, num_radial=6, propagation_depth=4)
CASES = {
    'sphere_net_b32': (dict(BASE, num_spherical=3, target_dim=1, output_init='GlorotOrthogonal'), 32),
    'spherical7_b500': (dict(BASE, num_spherical=7, target_dim=256), 500),
}


def make_batch(n_mol, dev):
    mols = amd.synth.make_dataset(n_mol, seed=n_mol)
    return graph.GeometricBatch.from_data_list(mols).to(dev)


def steps_of(model, opt, data, target, fused, steps, dev):
    smp.FUSED_TRIPLETS = fused
    loss_fn = torch.nn.L1Loss()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(model(data), target)
        loss.backward()
        opt.step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / steps, float(loss.item())


def timed(fn, iters, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e3 / iters


def stages(model, data, kw, iters, warmup, dev):
    pos = data.pos.float().contiguous()
    tb = model.emb.tables
    geo, _ = model.geometry(data)
    I, Bs = kw['int_emb_size'], kw['basis_emb_size']
    gen = torch.Generator().manual_seed(geo.T)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)          # noqa: E731
    x, s8, t8, w1, w2, g = r(geo.E, I), r(geo.T, Bs), r(geo.T, Bs), r(I, Bs), r(I, Bs), r(geo.E, I)
    leaves = [a.clone().requires_grad_() for a in (x, s8, t8, w1, w2)]

    def composed_fwd():
        return smp.triplets_composed(*leaves, geo)

    def composed_both():
        return torch.autograd.grad(composed_fwd(), leaves, g)

    fns = {
        'geometry': lambda: model.geometry(data),
        'bases': lambda: ops.smp_bases(pos, geo, tb.num_spherical, tb.num_radial, tb.cutoff, *tb.on(dev)),
        'triplets_fwd_fused': lambda: ops.smp_triplets_fwd(x, s8, t8, w1, w2, geo),
        'triplets_bwd_fused': lambda: ops.smp_triplets_bwd(g, x, s8, t8, w1, w2, geo),
        'triplets_fwd_composed': composed_fwd,
        'triplets_fwd_bwd_composed': composed_both,
    }
    for name, fn in fns.items():
        yield dict(what=name, atoms=geo.N, edges=geo.E, triplets=geo.T, int_emb=I, basis_emb=Bs, num_spherical=tb.num_spherical,
                   iters=iters, us_per_call=round(timed(fn, iters, warmup, dev), 2),
                   note='back-to-back calls between two HIP events: launch gaps, output allocations and host reads included')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for case, (kw, n_mol) in CASES.items():
        data = make_batch(n_mol, dev)
        torch.manual_seed(0)
        models = {True: amd.SMP(**kw).to(dev).train()}
        models[False] = copy.deepcopy(models[True])
        opts = {f: amd.Adam(m.parameters(), lr=1e-4) for f, m in models.items()}
        target = torch.randn(n_mol, kw['target_dim'], generator=torch.Generator().manual_seed(1)).to(dev)
        for fused in (True, False):
            steps_of(models[fused], opts[fused], data, target, fused, a.warmup, dev)
        times = {True: [], False: []}
        for _ in range(a.rounds):
            for fused in (True, False):
                ms, loss = steps_of(models[fused], opts[fused], data, target, fused, a.steps, dev)
                times[fused].append(round(ms, 3))
                emit(dict(what='step', case=case, form='fused' if fused else 'composed', molecules=n_mol, atoms=data.num_nodes,
                          steps=a.steps, ms_per_step=round(ms, 3), last_loss=loss, device=torch.cuda.get_device_name(dev)))
        smp.FUSED_TRIPLETS = True
        med = {f: float(np.median(t)) for f, t in times.items()}
        emit(dict(what='summary', case=case, fused_ms=times[True], composed_ms=times[False], fused_median_ms=med[True],
                  composed_median_ms=med[False], composed_over_fused=round(med[False] / med[True], 2)))
        for rec in stages(models[True], data, kw, a.iters, a.warmup, dev):
            emit(dict(rec, case=case))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
