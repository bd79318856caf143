"""Fixture of the non-contrastive objectives (reference commons/losses.py BarlowTwinsLoss :45-73, CosineSimilarityLoss :76-95,
RegularizationLoss :98-123, CriticLoss :33-42): the unmodified reference classes on seeded inputs -> tests/golden/batchstat.npz.

    python tests/golden/gen_golden_batchstat.py          (imports the reference checkout, as gen_golden.py does)

Inputs, once per shape (B, D) in (2, 8), (5, 13), (67, 13), (64, 64) under 'in/BxD/': z1 = randn(B, D) s with the column scale s_j
alternating 0.5, 1.5 - columns on both sides of the variance hinge relu(1 - sqrt(var + 1e-4)) - and z2_i = a_i z1_i + randn with
a_i = (0, 0.5, 3)[i mod 3]; 'seed' is the generator's seed.  CriticLoss takes z2 and `reconstruction(z1, z2, R)` [B, D, R], R in
(1, 3, 10), built from the stored pair with no further random numbers: repeat r is g_i z2_i + (0.5 + 0.1 r) z1 rolled by r + 1 rows,
g_i = (3, 0, 0.5)[i mod 3].  The case with the uniformity term gets both views scaled by D^-1/2 (`case_inputs`): on the unscaled pair at
D = 64 every exp(-2 |x_i - x_j|^2) underflows in fp32 and the reference's own fp32 loss is -inf.

Cases, per loss key and shape under '<key>/BxD/<tag>/': each class at its defaults; BarlowTwinsLoss and CosineSimilarityLoss also with
variance_reg = 1, covariance_reg = 0.04; BarlowTwinsLoss also with lambd = 1, scale_loss = 1; RegularizationLoss also with both
regularisers off and with uniformity_reg = 0.5.  Stored per case: the reference's loss in fp32 and fp64 ('loss32', 'loss64'), its fp64
gradients with respect to its two arguments as int32 fixed point relative to their largest entry ('g1_q', 'g1_scale', 'g2_q', 'g2_scale':
gen_golden_hardneg.encode / decode), and 'err32', the error of its fp32 loss and gradients against its fp64 ones in the measure of the
tests (gen_golden_hardneg.loss_err / grad_err).

Conditions, asserted here; the seed of a shape advances by 100000 until they hold: every column of z1 and of z2 keeps
|1 - sqrt(var + 1e-4)| > 1e-3 in fp64, so fp32 and fp64 take the same side of the hinge; in every shape with B >= 5 between 20 % and
80 % of the 2 D columns of the pair are on the active side; every fp32 result of the reference is finite.

The file is written with fixed zip time stamps and one torch thread: it regenerates bit-identically.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden_hardneg as GH  # noqa: E402

SHAPES = [(2, 8), (5, 13), (67, 13), (64, 64)]
LOSSES = {'barlow': 'BarlowTwinsLoss', 'cosine': 'CosineSimilarityLoss', 'regularization': 'RegularizationLoss', 'critic': 'CriticLoss'}
REPEATS = (1, 3, 10)
MARGIN = 1e-3
REGS = dict(variance_reg=1, covariance_reg=0.04)


def parameter_sets(key):
    """[(tag, constructor kwargs, R)]; R = 0: a two-view loss"""
    if key == 'barlow':
        return [('default', {}, 0), ('var1_cov0.04', dict(REGS), 0), ('lambd1_scale1', dict(lambd=1, scale_loss=1), 0)]
    if key == 'cosine':
        return [('default', {}, 0), ('var1_cov0.04', dict(REGS), 0)]
    if key == 'regularization':
        return [('default', {}, 0), ('var0_cov0', dict(variance_reg=0, covariance_reg=0), 0), ('unif0.5', dict(uniformity_reg=0.5), 0)]
    return [(f'R{R}', {}, R) for R in REPEATS]


def all_cases():
    return [(key, shape, tag) for key in LOSSES for shape in SHAPES for tag, _, _ in parameter_sets(key)]


def case_prefix(key, shape, tag):
    return f'{key}/{shape[0]}x{shape[1]}/{tag}/'


def pair(B, D, seed):
    """z1 [B, D], z2 [B, D] by the recipe above"""
    g = torch.Generator().manual_seed(seed)
    s = torch.tensor([0.5, 1.5])[torch.arange(D) % 2]
    z1 = torch.randn(B, D, generator=g) * s
    a = torch.tensor([0.0, 0.5, 3.0])[torch.arange(B) % 3]
    z2 = a[:, None] * z1 + torch.randn(B, D, generator=g)
    return z1.contiguous(), z2.contiguous()


def hinge_figures(z):
    """(share of the columns on the active side of relu(1 - sqrt(var + 1e-4)), the smallest distance of a column from the kink) in fp64"""
    h = 1.0 - torch.sqrt(torch.as_tensor(z).double().var(dim=0) + 1e-4)
    return (h > 0).double().mean().item(), h.abs().min().item()


def hinge_ok(z1, z2):
    share = 0.5 * (hinge_figures(z1)[0] + hinge_figures(z2)[0])
    margin = min(hinge_figures(z1)[1], hinge_figures(z2)[1])
    return margin > MARGIN and (z1.shape[0] < 5 or 0.2 <= share <= 0.8), share, margin


def base_inputs(B, D, finite=None):
    """(z1, z2, seed): the first seed of 1000 B + D, + 100000, ... whose pair meets the hinge conditions and - `finite(z1, z2)` given -
    that further condition"""
    seed = 1000 * B + D
    while True:
        z1, z2 = pair(B, D, seed)
        if hinge_ok(z1, z2)[0] and (finite is None or finite(z1, z2)):
            return z1, z2, seed
        seed += 100000


def reconstruction(z1, z2, R):
    """[B, D, R] from the pair alone"""
    z1, z2 = torch.as_tensor(z1), torch.as_tensor(z2)
    g = torch.tensor([3.0, 0.0, 0.5])[torch.arange(z1.shape[0]) % 3]
    return torch.stack([g[:, None] * z2 + (0.5 + 0.1 * r) * z1.roll(r + 1, 0) for r in range(R)], dim=2).contiguous()


def case_inputs(z1, z2, kw, R=0):
    """the two arguments a case's loss is called with"""
    z1, z2 = torch.as_tensor(z1), torch.as_tensor(z2)
    if R:
        return z2.contiguous(), reconstruction(z1, z2, R)
    if kw.get('uniformity_reg', 0) > 0:
        k = z1.shape[1] ** -0.5
        return (z1 * k).contiguous(), (z2 * k).contiguous()
    return z1.contiguous(), z2.contiguous()


def run_loss(cls, kw, x, y, dtype):
    a = x.to(dtype).clone().requires_grad_(True)
    b = y.to(dtype).clone().requires_grad_(True)
    loss = cls(**kw)(a, b)
    loss.backward()
    return loss.detach().numpy().copy(), a.grad.numpy().copy(), b.grad.numpy().copy()


def main():
    import gen_golden as G
    torch.set_num_threads(1)
    G.import_reference()
    import commons.losses as ref_losses

    def reference_fp32_finite(z1, z2):
        for key in LOSSES:
            for _, kw, R in parameter_sets(key):
                res = run_loss(getattr(ref_losses, LOSSES[key]), kw, *case_inputs(z1, z2, kw, R), torch.float32)
                if not all(np.isfinite(r).all() for r in res):
                    return False
        return True

    out = {}
    inputs = {}
    for B, D in SHAPES:
        z1, z2, seed = base_inputs(B, D, reference_fp32_finite)
        ok, share, margin = hinge_ok(z1, z2)
        assert ok
        inputs[B, D] = (z1, z2)
        out[f'in/{B}x{D}/z1'], out[f'in/{B}x{D}/z2'], out[f'in/{B}x{D}/seed'] = z1.numpy(), z2.numpy(), np.array(seed)
        print(f'inputs {B}x{D}: seed {seed} active columns {share:.2f} margin {margin:.2e}')
    for key, (B, D), tag in all_cases():
        kw, R = next((k, r) for t, k, r in parameter_sets(key) if t == tag)
        cls = getattr(ref_losses, LOSSES[key])
        x, y = case_inputs(*inputs[B, D], kw, R)
        p = case_prefix(key, (B, D), tag)
        l32, a32, b32 = run_loss(cls, kw, x, y, torch.float32)
        l64, a64, b64 = run_loss(cls, kw, x, y, torch.float64)
        assert np.isfinite(l32) and np.isfinite(l64) and np.isfinite(a32).all() and np.isfinite(b32).all()
        out[p + 'loss32'], out[p + 'loss64'] = l32, l64
        out[p + 'g1_q'], out[p + 'g1_scale'] = GH.encode(a64)
        out[p + 'g2_q'], out[p + 'g2_scale'] = GH.encode(b64)
        out[p + 'err32'] = np.array([GH.loss_err(l32, l64), GH.grad_err(a32, a64), GH.grad_err(b32, b64)])
        print(f'{p} loss {float(l64):.6f} fp32 against fp64: loss {out[p + "err32"][0]:.2e} g1 {out[p + "err32"][1]:.2e} '
              f'g2 {out[p + "err32"][2]:.2e}')
    path = os.path.join(HERE, 'batchstat.npz')
    GH.write_npz(path, out)
    print('wrote batchstat.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
