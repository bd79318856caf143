"""Training-step time of the 3D autoencoder (configs/contrastive_training_Net3DAE.yml sizes: hidden 70, Fourier order 4, two encoder
layers, no decoder, distance_net of two layers with width 70, NTXentAE, Adam) on one MI355X, and the pair head's share of it.

Three forms of the pair head on the same device, batch and weights, in ONE process, their runs interleaved:
  fused     pair_head._PairMLPHeadFn (csrc/pairmlp.hip): nothing of size [P, 2H] or [P, D] is written
  composed  net3d_ae.FUSED_PAIR_HEAD = False: both [P, 2H] concatenations, the package MLP on each, softplus of the sum - kernels the
            package had before the fused head
  eager     the reference's two distance_net calls in torch eager on the node state of the package's trunk
Per (form, batch): `--runs` runs of `--steps` steps each (after `--warmup` steps per form), the median and the range of the
per-run step time, for the whole Net3DAE + NTXentAE forward + backward step (no optimiser: the trunk and the loss are the same in all
forms) and for the pair head alone (forward + backward from a fixed node state, HIP events).  One JSON line per (form, batch).
The eager form's whole step runs the trunk per block (no whole-model tape node, so that torch autograd can carry the eager head), the
other two run it under the whole-model node: compare `eager` with the others by `head_ms` only; its `step_ms` is marked `trunk:
per-block`.

    python tools/net3dae_bench.py --batches 50 500 --out profiles/net3dae_bench.jsonl
    rocprofv3 --kernel-trace --stats -d prof -o ae -- python tools/net3dae_bench.py --batches 500 --forms fused --runs 1 --steps 5 --warmup 2 --no-head
    python tools/net3dae_bench.py --kernel-stats prof/ae_results.db --trace-steps 7
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module('3dinfomax_amd')
dataset = importlib.import_module('3dinfomax_amd.dataset')
net3d_ae = importlib.import_module('3dinfomax_amd.net3d_ae')

MODEL = dict(node_dim=0, edge_dim=1, hidden_dim=70, readout_aggregators=['min', 'max', 'mean'], batch_norm=True, batch_norm_momentum=0.93,
             reduce_func='mean', dropout=0.0, fourier_encodings=4, update_net_layers=2, message_net_layers=2, encoder_depth=2,
             decoder_depth=0, node_wise_encoder_layers=0, node_wise_output_layers=0, distance_net=True, projection_dim=70,
             projection_layers=2)
LOSS = dict(tau=0.1, reconstruction_reg=1)


def eager_head(model, h, pidx):
    """reference models/net3d_VAE.py:107-119 with torch's own Linear / BatchNorm kernels"""
    f0, f1 = model.distance_net.fully_connected
    bn = f0.batch_norm

    def net(x):
        x = F.relu(F.linear(x, f0.linear.weight, f0.linear.bias))
        x = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, model.training, bn.momentum, bn.eps)
        return F.linear(x, f1.linear.weight, f1.linear.bias)
    hs, hd = h[pidx[0]], h[pidx[1]]
    return F.softplus(net(torch.cat([hs, hd], 1)) + net(torch.cat([hd, hs], 1)))


class Case:
    def __init__(self, B, dev, kind):
        mols = amd.synth.make_dataset(B, seed=B, kind=kind)
        ds = dataset.FlatMolDataset(mols)
        [_], [self.g3, self.pidx], self.dist = ds.assemble_ae(np.arange(B), dev)
        torch.manual_seed(0)
        self.model = amd.Net3DAE(**MODEL).to(dev).train()
        self.loss_fn = amd.NTXentAE(**LOSS)
        self.z1 = torch.randn(B, 70 * 3, generator=torch.Generator().manual_seed(1)).to(dev)
        self.B, self.atoms, self.pairs = B, int(self.g3.number_of_nodes()), int(self.pidx.shape[1])
        g = self.g3.local_copy()
        with torch.no_grad():
            self.model(g, self.pidx)
        self.h = g.ndata['feat'].detach().clone()          # a fixed node state for the head-only timing

    def head(self, form, h):
        if form == 'eager':
            return eager_head(self.model, h, self.pidx)
        net3d_ae.FUSED_PAIR_HEAD = form == 'fused'
        return self.model._pair_head(h, amd.pair_head.pair_index(self.pidx, self.g3))

    def step(self, form):
        self.model.zero_grad(set_to_none=True)
        g = self.g3.local_copy()
        if form == 'eager':
            # the trunk run per block with the head cut off, then the eager head on its node state
            latent, h = self.trunk(g)
            pred = eager_head(self.model, h, self.pidx)
        else:
            net3d_ae.FUSED_PAIR_HEAD = form == 'fused'
            latent, pred = self.model(g, self.pidx)
        contrastive, recon = self.loss_fn(self.z1, latent, self.dist, pred)
        (contrastive + recon).backward()
        return contrastive, recon

    def trunk(self, g):
        """latent vector and node state as autograd tensors: the model run per block (no whole-model node), head not called"""
        tape = importlib.import_module('3dinfomax_amd.tape')
        prev, tape.run_model = tape.run_model, lambda module, run: run()
        self.model.__dict__['_pair_head'] = lambda h, pidx: h          # shadows the method for this call
        try:
            latent, h = self.model(g, self.pidx)
        finally:
            tape.run_model = prev
            del self.model.__dict__['_pair_head']
        return latent, h

    def head_step(self, form):
        h = self.h.clone().requires_grad_(True)
        self.model.zero_grad(set_to_none=True)
        y = self.head(form, h)
        y.backward(self.dist)


def timed(fn, steps, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / steps


def kernel_stats(db, steps):
    """table of the kernels of a rocprofv3 database (rocpd): launches and microseconds per step, share of the device time"""
    import sqlite3
    rows = sqlite3.connect(db).execute('select name, count(*), sum(duration) from kernels group by name order by sum(duration) desc')
    rows = [(n.replace('(anonymous namespace)::', '').split('(')[0].replace('void ', ''), c, t / 1e3 / steps) for n, c, t in rows]
    total = sum(r[2] for r in rows)
    out = [f'{"us/step":>9} {"share":>6} {"calls/step":>10}  kernel', f'{total:9.1f} {100.0:6.1f} {sum(r[1] for r in rows) / steps:10.1f}  (all)']
    out += [f'{t:9.1f} {100 * t / total:6.1f} {c / steps:10.1f}  {n}' for n, c, t in rows]
    return '\n'.join(out)


def summary(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel-stats', default=None, help='rocpd database of a rocprofv3 --kernel-trace run: print the kernel table')
    ap.add_argument('--trace-steps', type=int, default=7, help='training steps the traced run took (warm-up included)')
    ap.add_argument('--batches', type=int, nargs='+', default=[50, 500])
    ap.add_argument('--forms', nargs='+', default=['fused', 'composed', 'eager'], choices=['fused', 'composed', 'eager'])
    ap.add_argument('--kind', default='qmugs', choices=['qm9', 'qmugs'], help='synthetic molecules: qmugs = drug-sized')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-head', action='store_true', help='skip the head-only timing (kernel traces of the whole step)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        print(kernel_stats(a.kernel_stats, a.trace_steps))
        return
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    lines = []
    for B in a.batches:
        case = Case(B, dev, a.kind)
        for form in a.forms:
            for _ in range(a.warmup):
                case.step(form)
                if not a.no_head:
                    case.head_step(form)
        step_ms = {f: [] for f in a.forms}
        head_ms = {f: [] for f in a.forms}
        for _ in range(a.runs):                      # interleaved: one run of every form, then the next round
            for form in a.forms:
                step_ms[form].append(timed(lambda: case.step(form), a.steps, dev))
                if not a.no_head:
                    head_ms[form].append(timed(lambda: case.head_step(form), a.steps, dev))
        for form in a.forms:
            r = dict(form=form, batch=B, kind=a.kind, atoms=case.atoms, pairs=case.pairs, runs=a.runs, steps=a.steps, warmup=a.warmup,
                     step_ms=summary(step_ms[form]), trunk='per-block' if form == 'eager' else 'whole-model',
                     device=torch.cuda.get_device_name(dev))
            if not a.no_head:
                r['head_ms'] = summary(head_ms[form])
                r['head_share'] = round(r['head_ms']['median'] / r['step_ms']['median'], 3)
            print(json.dumps(r), flush=True)
            lines.append(r)
    net3d_ae.FUSED_PAIR_HEAD = True
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
