"""Fixture of the set-matching and per-conformer NT-Xent losses (reference commons/losses.py NTXentMultiplePositivesV2 :598-643,
NTXentMultiplePositivesV3 :646-689, NTXentMinimumMatching :747-794, NTXentMaximumSimilarity :839-886): the unmodified reference classes
on seeded inputs -> tests/golden/confmatch.npz.

    python tests/golden/gen_golden_confmatch.py          (imports the reference checkout, as gen_golden.py does)

Loss level, per loss ('v2', 'v3', 'min', 'max') and case: z1, z2 (fp32), and the reference's loss, dz1 and dz2 computed in fp32
('loss32', 'dz1_32', 'dz2_32') and in fp64 on the same inputs ('loss64', ...), the seed used and - matching losses - the selection gap.
tau = 0.1, everything else at the constructor defaults.  Matching losses: z1 [B, C D], z2 [B C, D]; V2 / V3: z1 [B, D], z2 [B C, D].
Cases (B, C, D): (2, 1, 8), (5, 3, 24), (7, 5, 40), (3, 2, 7) with standard normal entries, and '5x3x24n': every conformer of both views
of a molecule is that molecule's base vector + 0.3 noise (positives near exp(1 / tau)).

Selection condition of the matching inputs (selection_gap, in fp64): the best and the second-best s' differ by more than GAP = 1e-4 in
every C x C block for the minimum, in every block for the maximum, and in every row's set of matched entries {(j, l)} - about 1000 times
the rounding of an fp32 cosine, so the selected entry does not depend on the precision and the gradients of two precisions are
comparable.  A seed that fails it is replaced by seed + 100000 until one passes.

End to end ('e2e/...'): 4 synthetic molecules x 2 conformers through the reference PNA (hidden 16, depth 2) and Net3D (hidden 8,
target_dim 8) batched by the reference's conformer_collate: NTXentMinimumMatching (PNA target_dim 2 * 8) and NTXentMultiplePositivesV3
(PNA target_dim 8); per loss the loss, both embeddings, every parameter gradient and the state dicts.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_separate2d as GS  # noqa: E402

TAU = 0.1
GAP = 1e-4
CASES = [(2, 1, 8), (5, 3, 24), (7, 5, 40), (3, 2, 7)]
NEAR_CASE = (5, 3, 24)
ALL_CASES = [(c, False) for c in CASES] + [(NEAR_CASE, True)]
MATCHING = {'min': 'NTXentMinimumMatching', 'max': 'NTXentMaximumSimilarity'}
PER_CONFORMER = {'v2': 'NTXentMultiplePositivesV2', 'v3': 'NTXentMultiplePositivesV3'}
LOSSES = dict(MATCHING, **PER_CONFORMER)
E2E = {'min': dict(GS.PNA_KW), 'v3': dict(GS.PNA_KW, target_dim=GS.E2E_DIM)}


def case_tag(B, C, D, near=False):
    return f'{B}x{C}x{D}' + ('n' if near else '')


def base_seed(B, C, D, near=False):
    return 1000 * B + 10 * C + D + (7 if near else 0)


def matching_inputs(B, C, D, near=False, seed=None):
    """z1 [B, C D], z2 [B C, D], drawn as gen_golden_separate2d.case_inputs draws them"""
    g = torch.Generator().manual_seed(base_seed(B, C, D, near) if seed is None else seed)
    if near:
        base = torch.randn(B, 1, D, generator=g)
        z1 = (base + 0.3 * torch.randn(B, C, D, generator=g)).reshape(B, C * D)
        z2 = (base + 0.3 * torch.randn(B, C, D, generator=g)).reshape(B * C, D)
    else:
        z1, z2 = torch.randn(B, C * D, generator=g), torch.randn(B * C, D, generator=g)
    return z1.contiguous(), z2.contiguous()


def per_conformer_inputs(B, C, D, near=False, seed=None):
    """z1 [B, D], z2 [B C, D] from one generator"""
    g = torch.Generator().manual_seed(base_seed(B, C, D, near) if seed is None else seed)
    if near:
        base = torch.randn(B, 1, D, generator=g)
        z1 = (base + 0.3 * torch.randn(B, 1, D, generator=g)).reshape(B, D)
        z2 = (base + 0.3 * torch.randn(B, C, D, generator=g)).reshape(B * C, D)
    else:
        z1, z2 = torch.randn(B, D, generator=g), torch.randn(B * C, D, generator=g)
    return z1.contiguous(), z2.contiguous()


def selection_gap(z1, z2, norm=True):
    """the smallest difference, in fp64, between the best and the second-best s' over every selection the matching losses make: the
    minimum and the maximum of every C x C block, and the maximum of every row's matched entries {(j, l)}"""
    z1, z2 = torch.as_tensor(z1).double(), torch.as_tensor(z2).double()
    B, D = z1.shape[0], z2.shape[1]
    a, b = z1.reshape(B, -1, D), z2.reshape(B, -1, D)
    C = a.shape[1]
    S = torch.einsum('ilk,juk->ijlu', a, b)
    if norm:
        S = S / (a.norm(dim=2)[:, None, :, None] * b.norm(dim=2)[None, :, None, :])
    gaps = []
    if C > 1:
        blocks = S.reshape(B, B, C * C).sort(dim=2).values
        gaps += [(blocks[..., 1] - blocks[..., 0]).min().item(), (blocks[..., -1] - blocks[..., -2]).min().item()]
    matched = torch.diagonal(S, dim1=2, dim2=3).reshape(B, B * C).sort(dim=1).values
    gaps.append((matched[:, -1] - matched[:, -2]).min().item())
    return min(gaps)


def gapped_matching_inputs(B, C, D, near=False, scale=1.0, norm=True):
    """-> (z1, z2, seed, gap): the first seed of base, base + 100000, ... whose inputs meet the selection condition"""
    seed = base_seed(B, C, D, near)
    while True:
        z1, z2 = matching_inputs(B, C, D, near, seed)
        z1, z2 = scale * z1, scale * z2
        gap = selection_gap(z1, z2, norm)
        if gap > GAP:
            return z1, z2, seed, gap
        seed += 100000


def run_loss(cls, z1, z2, dtype):
    a = z1.to(dtype).clone().requires_grad_(True)
    b = z2.to(dtype).clone().requires_grad_(True)
    loss = cls(tau=TAU)(a, b)
    loss.backward()
    return loss.detach().numpy().copy(), a.grad.numpy().copy(), b.grad.numpy().copy()


def main():
    dgl, PNA, _, Net3D, _, _ = G.import_reference()
    sys.modules.setdefault('torch_geometric', types.ModuleType('torch_geometric'))    # custom_collate.py:6 (unused here)
    pkg = types.ModuleType('datasets')                                                 # bypass datasets/__init__.py
    pkg.__path__ = [os.path.join(G.REF, 'datasets')]
    sys.modules['datasets'] = pkg
    import commons.losses as ref_losses
    from datasets.custom_collate import conformer_collate

    out = {}
    rel = lambda x, y: float(np.abs(x.astype(np.float64) - y).max() / max(np.abs(y).max(), 1e-30))
    for key, name in LOSSES.items():
        cls = getattr(ref_losses, name)
        for (B, C, D), near in ALL_CASES:
            p = f'{key}/{case_tag(B, C, D, near)}/'
            if key in MATCHING:
                z1, z2, seed, gap = gapped_matching_inputs(B, C, D, near)
                assert gap > GAP
                out[p + 'gap'] = np.array(gap)
            else:
                seed, gap = base_seed(B, C, D, near), float('nan')
                z1, z2 = per_conformer_inputs(B, C, D, near)
            out[p + 'seed'] = np.array(seed)
            out[p + 'z1'], out[p + 'z2'] = z1.numpy(), z2.numpy()
            l32, a32, b32 = run_loss(cls, z1, z2, torch.float32)
            l64, a64, b64 = run_loss(cls, z1, z2, torch.float64)
            out.update({p + 'loss32': l32, p + 'dz1_32': a32, p + 'dz2_32': b32, p + 'loss64': l64, p + 'dz1_64': a64, p + 'dz2_64': b64})
            print(f'{p} seed {seed} gap {gap:.2e} loss {float(l64):.6f} fp32 against fp64: loss '
                  f'{abs(float(l32) - float(l64)) / max(abs(float(l64)), 1.0):.2e} dz1 {rel(a32, a64):.2e} dz2 {rel(b32, b64):.2e}')

    mols, confs = GS.e2e_molecules()
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

    for key, pna_kw in E2E.items():
        model_seed = 321
        while True:
            torch.manual_seed(model_seed)
            pna = PNA(avg_d=1.0, device='cpu', **pna_kw)
            net = Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **GS.NET3D_KW)
            G.make_trained_like(pna, 17)
            G.make_trained_like(net, 19)
            pna.train(), net.train()
            items = [(graph2d(m), dgl.batch([graph3d(m, c) for c in cs])) for m, cs in zip(mols, confs)]
            (bg,), (bgc,) = conformer_collate(items)
            z1, z2 = pna(bg), net(bgc)
            gap = selection_gap(z1.detach(), z2.detach()) if key in MATCHING else float('nan')
            if key not in MATCHING or gap > GAP:
                break
            model_seed += 1
        p = f'e2e/{key}/'
        out.update(G.sd_np(pna, p + 'pna_sd'))
        out.update(G.sd_np(net, p + 'net3d_sd'))
        loss = getattr(ref_losses, LOSSES[key])(tau=TAU)(z1, z2)
        loss.backward()
        out[p + 'loss'], out[p + 'z1'], out[p + 'z2'] = np.array(loss.item()), z1.detach().numpy(), z2.detach().numpy()
        out[p + 'gap'], out[p + 'model_seed'] = np.array(gap), np.array(model_seed)
        out.update(G.grads_np(pna, p + 'pna_grad'))
        out.update(G.grads_np(net, p + 'net3d_grad'))
        print(p, 'model seed', model_seed, 'gap', f'{gap:.2e}', 'loss', loss.item(), 'z1', tuple(z1.shape), 'z2', tuple(z2.shape))
    path = os.path.join(HERE, 'confmatch.npz')
    np.savez_compressed(path, **out)
    print('wrote confmatch.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
