"""Fixture of KLDivergenceMultiplePositives (reference commons/losses.py:261-314) and the metrics of its config
(configs/contrastive_training_multiple_positives_kl_div_loss.yml: conformer_3d_variance, conformer_2d_variance, batch_variance,
dimension_covariance; reference trainer/metrics.py:161-209): the unmodified reference classes on seeded inputs ->
tests/golden/kl_multiple_positives.npz.

    python tests/golden/gen_golden_kl.py          (imports the reference checkout, as gen_golden.py does)

Loss level, per case and norm setting ('loss/<case>/n0/' norm=False, the default; '.../n1/' norm=True): the reference's loss, dz1 and dz2
computed in fp32 ('loss32', 'dz1_32', 'dz2_32') and in fp64 on the same inputs ('loss64', ...); the inputs z1 [B, 2 D], z2 [B C, D] (fp32)
once per case ('loss/<case>/z1', '.../z2').  Cases (B, C, D): (1, 2, 8), (2, 2, 8), (5, 3, 24), (7, 5, 40), (3, 2, 7), (4, 9, 16) with
standard normal entries, and '5x3x24j': the conformers of a molecule are that molecule's base vector + 1e-2 noise (1 / v2 near its
largest).

Metrics ('metrics/<case>/...'): the four metrics of the config on the same inputs in fp64, the two conformer metrics with normalize
False ('..._n0') and True ('..._n1').

End to end ('e2e/...'): 4 synthetic molecules x 2 conformers through the reference PNA (hidden 16, target_dim 2 * 8, depth 2) and
Net3D (hidden 8, target_dim 8) batched by the reference's conformer_collate; the loss, both embeddings and every parameter gradient,
computed by the reference in fp64 from the fp32 weights and inputs stored beside them.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

CASES = [(1, 2, 8), (2, 2, 8), (5, 3, 24), (7, 5, 40), (3, 2, 7), (4, 9, 16)]
JITTER_CASE = (5, 3, 24)
ALL_CASES = [(c, False) for c in CASES] + [(JITTER_CASE, True)]
LOSS = 'KLDivergenceMultiplePositives'
E2E_MOLS, E2E_CONF, E2E_DIM = 4, 2, 8
# Coordinate noise of the synthetic conformers.  The gradient of this loss carries 1 / v2, so conformers whose embeddings nearly coincide
# make the parameter gradients ill-conditioned in fp32: at synth.conformers' default 0.05 the variance over the two conformers falls to
# 1.7e-7, below the loss's own 1e-6, and the reference's fp32 gradients miss its fp64 gradients by up to 6.8 x the bound of
# helpers.grads_close(5e-4) - no yardstick for another fp32 implementation.  At 0.3 they stay within 0.12 x that bound (main() asserts
# a quarter).  The near-coincident regime is covered at loss level ('5x3x24j'), where the rule scales with the reference's own error.
E2E_NOISE = 0.3
PNA_KW = dict(G.PNA_YML, hidden_dim=16, target_dim=2 * E2E_DIM, propagation_depth=2, readout_hidden_dim=16)
NET3D_KW = dict(G.NET3D_YML, hidden_dim=8, hidden_edge_dim=8, readout_hidden_dim=8, target_dim=E2E_DIM)


def case_tag(B, C, D, jitter=False):
    return f'{B}x{C}x{D}' + ('j' if jitter else '')


def case_inputs(B, C, D, jitter=False):
    g = torch.Generator().manual_seed(2000 * B + 10 * C + D + (7 if jitter else 0))
    z1 = torch.randn(B, 2 * D, generator=g)
    if jitter:
        z2 = (torch.randn(B, 1, D, generator=g) + 1e-2 * torch.randn(B, C, D, generator=g)).reshape(B * C, D)
    else:
        z2 = torch.randn(B * C, D, generator=g)
    return z1.contiguous(), z2.contiguous()


def run_loss(cls, z1, z2, dtype, norm):
    a = z1.to(dtype).clone().requires_grad_(True)
    b = z2.to(dtype).clone().requires_grad_(True)
    loss = cls(norm=norm)(a, b)
    loss.backward()
    return loss.detach().numpy().copy(), a.grad.numpy().copy(), b.grad.numpy().copy()


def e2e_molecules():
    mols = G.synth.make_dataset(E2E_MOLS, seed=67)
    rng = np.random.default_rng(13)
    return mols, [G.synth.conformers(m, rng, E2E_CONF, E2E_NOISE) for m in mols]


def import_reference_metrics():
    """trainer/metrics.py imports evaluators and dataset classes these metrics never touch: empty placeholders, as gen_golden_metrics.py"""
    for name, attrs in (('ogb', ()), ('ogb.graphproppred', ('Evaluator',)), ('ogb.lsc', ('PCQM4MEvaluator',)),
                        ('datasets.geom_drugs_dataset', ('GEOMDrugs',)), ('datasets.qm9_dataset', ('QM9Dataset',))):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, object)
        sys.modules[name] = m
    import trainer.metrics as M
    return M


def main():
    dgl, PNA, _, Net3D, _, _ = G.import_reference()
    sys.modules.setdefault('torch_geometric', types.ModuleType('torch_geometric'))    # custom_collate.py:6 (unused here)
    pkg = types.ModuleType('datasets')                                                 # bypass datasets/__init__.py
    pkg.__path__ = [os.path.join(G.REF, 'datasets')]
    sys.modules['datasets'] = pkg
    import commons.losses as ref_losses
    from datasets.custom_collate import conformer_collate
    M = import_reference_metrics()
    cls = getattr(ref_losses, LOSS)

    out = {}
    rel = lambda x, y: float(np.abs(x.astype(np.float64) - y).max() / max(np.abs(y).max(), 1e-30))
    for (B, C, D), jitter in ALL_CASES:
        z1, z2 = case_inputs(B, C, D, jitter)
        tag = case_tag(B, C, D, jitter)
        out[f'loss/{tag}/z1'], out[f'loss/{tag}/z2'] = z1.numpy(), z2.numpy()
        for norm in (False, True):
            p = f'loss/{tag}/n{int(norm)}/'
            l32, a32, b32 = run_loss(cls, z1, z2, torch.float32, norm)
            l64, a64, b64 = run_loss(cls, z1, z2, torch.float64, norm)
            out.update({p + 'loss32': l32, p + 'dz1_32': a32, p + 'dz2_32': b32, p + 'loss64': l64, p + 'dz1_64': a64, p + 'dz2_64': b64})
            lerr = abs(float(l32) - float(l64)) / max(abs(float(l64)), 1.0)
            print(f'{p} loss {float(l64):.6f} fp32 against fp64: loss {lerr:.2e} dz1 {rel(a32, a64):.2e} dz2 {rel(b32, b64):.2e}')
        a, b = z1.double(), z2.double()
        p = f'metrics/{tag}/'
        for norm in (False, True):
            out[p + f'conformer_3d_variance_n{int(norm)}'] = np.float64(M.Conformer3DVariance(normalize=norm)(a, b).item())
            out[p + f'conformer_2d_variance_n{int(norm)}'] = np.float64(M.Conformer2DVariance(normalize=norm)(a, b).item())
        if B > 1:          # std over a batch of one is NaN
            out[p + 'batch_variance'] = np.float64(M.BatchVariance()(a, b).item())
            out[p + 'dimension_covariance'] = np.float64(M.DimensionCovariance()(a, b).item())
        print(p, {k[len(p):]: float(v) for k, v in out.items() if k.startswith(p)})

    mols, confs = e2e_molecules()
    out.update(G.mols_to_npz(mols, prefix='e2e/mol'))
    out['e2e/conf_coords'] = np.concatenate([c for cs in confs for c in cs])          # molecule major, conformer minor

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
        torch.manual_seed(654)
        pna = PNA(avg_d=1.0, device='cpu', **PNA_KW)
        net = Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_KW)
        G.make_trained_like(pna, 23)
        G.make_trained_like(net, 29)
        sd = {**G.sd_np(pna, 'e2e/pna_sd'), **G.sd_np(net, 'e2e/net3d_sd')}
        pna.to(dtype).train(), net.to(dtype).train()
        items = [(graph2d(m), dgl.batch([graph3d(m, c, dtype) for c in cs])) for m, cs in zip(mols, confs)]
        (bg,), (bgc,) = conformer_collate(items)
        z1, z2 = pna(bg), net(bgc)
        loss = cls()(z1, z2)
        loss.backward()
        res = {'e2e/loss': np.array(loss.item()), 'e2e/z1': z1.detach().numpy(), 'e2e/z2': z2.detach().numpy(),
               **G.grads_np(pna, 'e2e/pna_grad'), **G.grads_np(net, 'e2e/net3d_grad')}
        return sd, res

    sd, r64 = run_e2e(torch.float64)
    _, r32 = run_e2e(torch.float32)
    out.update(sd)
    out.update(r64)
    v2 = torch.from_numpy(r64['e2e/z2']).reshape(E2E_MOLS, E2E_CONF, E2E_DIM).var(dim=1)
    print(f'e2e loss {float(r64["e2e/loss"]):.7f} (fp32 {float(r32["e2e/loss"]):.7f}) var over the conformers: min {v2.min().item():.2e} '
          f'median {v2.median().item():.2e}')
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
    path = os.path.join(HERE, 'kl_multiple_positives.npz')
    np.savez_compressed(path, **out)
    print('wrote kl_multiple_positives.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
