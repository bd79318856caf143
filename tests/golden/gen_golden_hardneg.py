"""Fixture of the single-positive losses that re-weight the negatives (reference commons/losses.py InfoNCE :998-1034, InfoNCEHard
:1037-1074, NTXentHard :1077-1114, NTXentExtraNegatives :889-943, NTXentShuffled :967-995): the unmodified reference classes on seeded
inputs -> tests/golden/hardneg.npz.

    python tests/golden/gen_golden_hardneg.py          (imports the reference checkout, as gen_golden.py does)

Inputs, once per shape (B, D) in (2, 8), (5, 13), (67, 13), (64, 64) under 'in/BxD/': z1 = randn(B, D), z2_i = a_i z1_i + randn with
a_i = (0, 0.5, 3)[i mod 3] - unaligned, half-aligned and well-aligned pairs - and a pool x [B, 3, D] of standard normal extra negatives;
NTXentExtraNegatives with U extras takes cat(z2, x[:, :U]).  A class whose default is norm=False (InfoNCEHard) gets z1 and z2 scaled by
D^-1/2 (`case_inputs`), so exp(<z1, z2> / tau) stays far below the fp32 overflow.

Cases, per loss key and shape under '<key>/BxD/<parameter tag>/': the class's defaults and tau = 0.1; the hard pair also tau = 0.1 with
beta = 1.0; NTXentExtraNegatives (U, extra_negatives_weight) = (1, 1), (3, 50) at the defaults and (1, 50), (3, 1) at tau = 0.1.  Stored
per case: the reference's loss in fp32 and fp64 ('loss32', 'loss64'), its fp64 gradients, and 'err32', the error of its fp32 loss, dz1
and dz2 against its fp64 ones in the measure of the tests (`loss_err`, `grad_err`).  To stay below 1 MiB the fp32 gradients themselves
are not stored, and an fp64 gradient is stored as int32 fixed point relative to its largest entry ('dz1_q', 'dz1_scale'; `decode`): a
step of 4.7e-10 of that entry, three orders below anything the tests resolve in that same measure.  NTXentShuffled: the seed given to
torch.manual_seed before the call and the permutation it draws ('seed', 'perm').  Hard pair: 'clamped', the share of rows with
Ng_i < floor, and 'margin', the smallest |Ng_i - floor| / max(|Ng_i|, floor), both in fp64.

Clamp conditions, asserted here: in every tau = 0.1 hard case with B >= 5 between 20 % and 80 % of the rows are clamped; every row of
every hard case has a margin above 1e-3, so fp32 and fp64 take the same branch; with NTXentHard's default parameters no row is clamped.
(InfoNCEHard's defaults do clamp: without normalisation the positive of a well-aligned row is e^6 against negatives near 1, and
tau_plus n pos_i outweighs the re-weighted sum in every such row.)

The file is written with fixed zip time stamps and one torch thread: it regenerates bit-identically.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SHAPES = [(2, 8), (5, 13), (67, 13), (64, 64)]
LOSSES = {'infonce': 'InfoNCE', 'infonce_hard': 'InfoNCEHard', 'ntxent_hard': 'NTXentHard', 'extra': 'NTXentExtraNegatives',
          'shuffled': 'NTXentShuffled'}
HARD = ('infonce_hard', 'ntxent_hard')
DEFAULT_NORM = {'infonce': True, 'infonce_hard': False, 'ntxent_hard': True, 'extra': True, 'shuffled': True}
DEFAULT_HARD = {'infonce_hard': dict(tau=0.5, tau_plus=0.1, beta=0.5), 'ntxent_hard': dict(tau=0.5, tau_plus=0.1, beta=0.1)}
POOL = 3
MARGIN = 1e-3
Q = 2 ** 31 - 1


def parameter_sets(key):
    """[(tag, constructor kwargs, U)]"""
    if key in HARD:
        return [('default', {}, 0), ('tau0.1', dict(tau=0.1), 0), ('tau0.1_beta1', dict(tau=0.1, beta=1.0), 0)]
    if key == 'extra':
        return [('default_U1_w1', dict(extra_negatives_weight=1), 1), ('default_U3_w50', dict(extra_negatives_weight=50), 3),
                ('tau0.1_U1_w50', dict(tau=0.1, extra_negatives_weight=50), 1), ('tau0.1_U3_w1', dict(tau=0.1, extra_negatives_weight=1), 3)]
    return [('default', {}, 0), ('tau0.1', dict(tau=0.1), 0)]


def all_cases():
    return [(key, shape, tag) for key in LOSSES for shape in SHAPES for tag, _, _ in parameter_sets(key)]


def case_prefix(key, shape, tag):
    return f'{key}/{shape[0]}x{shape[1]}/{tag}/'


def base_inputs(B, D, seed=None):
    """z1 [B, D], z2 [B, D], x [B, POOL, D] from one generator"""
    g = torch.Generator().manual_seed(1000 * B + D if seed is None else seed)
    z1 = torch.randn(B, D, generator=g)
    a = torch.tensor([0.0, 0.5, 3.0])[torch.arange(B) % 3]
    z2 = a[:, None] * z1 + torch.randn(B, D, generator=g)
    x = torch.randn(B, POOL, D, generator=g)
    return z1.contiguous(), z2.contiguous(), x.contiguous()


def case_inputs(z1, z2, x, norm, U=0):
    """the pair a loss is called with: scaled by D^-1/2 without normalisation, the first U extras of every row appended to z2"""
    z1, z2, x = torch.as_tensor(z1), torch.as_tensor(z2), torch.as_tensor(x)
    B, D = z1.shape
    if not norm:
        z1, z2 = z1 * D ** -0.5, z2 * D ** -0.5
    if U:
        z2 = torch.cat([z2, x[:, :U].reshape(B * U, D)])
    return z1.contiguous(), z2.contiguous()


def loss_err(got, ref):
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1.0)


def grad_err(got, ref):
    a, b = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def encode(x):
    """fp64 array -> (int32 fixed point, scale)"""
    scale = float(np.abs(x).max()) or 1.0
    return np.rint(x / scale * Q).astype(np.int32), np.array(scale)


def decode(z, prefix, name):
    return z[prefix + name + '_q'].astype(np.float64) * (float(z[prefix + name + '_scale']) / Q)


def hard_ng(z1, z2, norm=True, tau=0.5, tau_plus=0.1, beta=0.5):
    """(Ng [B] before the clamp, floor) of the hard pair in fp64"""
    z1, z2 = torch.as_tensor(z1).double(), torch.as_tensor(z2).double()
    B = z1.shape[0]
    s = z1 @ z2.T
    if norm:
        s = s / (z1.norm(dim=1)[:, None] * z2.norm(dim=1)[None, :])
    t = s / tau
    off = ~torch.eye(B, dtype=torch.bool)
    A = (torch.exp(beta * t) * off).sum(dim=1)
    C = (torch.exp((1 + beta) * t) * off).sum(dim=1)
    n = B - 1
    ng = (n * C / A - tau_plus * n * torch.exp(torch.diagonal(t))) / (1 - tau_plus)
    return ng, n * float(np.exp(-1.0 / tau))


def clamp_figures(z1, z2, norm, **kw):
    """(share of clamped rows, smallest |Ng - floor| / max(|Ng|, floor))"""
    ng, floor = hard_ng(z1, z2, norm, **kw)
    margin = ((ng - floor).abs() / torch.maximum(ng.abs(), torch.full_like(ng, floor))).min().item()
    return (ng < floor).double().mean().item(), margin


def run_loss(cls, kw, z1, z2, dtype, seed=None):
    a = z1.to(dtype).clone().requires_grad_(True)
    b = z2.to(dtype).clone().requires_grad_(True)
    if seed is not None:
        torch.manual_seed(seed)
    loss = cls(**kw)(a, b)
    loss.backward()
    return loss.detach().numpy().copy(), a.grad.numpy().copy(), b.grad.numpy().copy()


def shuffle_seed(B, D, tag):
    return 7000 + 10 * B + D + (1 if tag != 'default' else 0)


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    import gen_golden as G
    torch.set_num_threads(1)
    G.import_reference()
    import commons.losses as ref_losses

    out = {}
    for B, D in SHAPES:
        z1, z2, x = base_inputs(B, D)
        out[f'in/{B}x{D}/z1'], out[f'in/{B}x{D}/z2'], out[f'in/{B}x{D}/x'] = z1.numpy(), z2.numpy(), x.numpy()
    for key, (B, D), tag in all_cases():
        kw, U = next((k, u) for t, k, u in parameter_sets(key) if t == tag)
        cls = getattr(ref_losses, LOSSES[key])
        norm = DEFAULT_NORM[key]
        z1, z2 = case_inputs(*base_inputs(B, D), norm, U)
        p = case_prefix(key, (B, D), tag)
        seed = shuffle_seed(B, D, tag) if key == 'shuffled' else None
        l32, a32, b32 = run_loss(cls, kw, z1, z2, torch.float32, seed)
        l64, a64, b64 = run_loss(cls, kw, z1, z2, torch.float64, seed)
        assert np.isfinite(l32) and np.isfinite(l64) and np.isfinite(a32).all() and np.isfinite(b32).all()
        out[p + 'loss32'], out[p + 'loss64'] = l32, l64
        out[p + 'dz1_q'], out[p + 'dz1_scale'] = encode(a64)
        out[p + 'dz2_q'], out[p + 'dz2_scale'] = encode(b64)
        out[p + 'err32'] = np.array([loss_err(l32, l64), grad_err(a32, a64), grad_err(b32, b64)])
        note = ''
        if key == 'shuffled':
            torch.manual_seed(seed)
            out[p + 'seed'], out[p + 'perm'] = np.array(seed), torch.randperm(B).numpy()
        if key in HARD:
            share, margin = clamp_figures(z1, z2, norm, **dict(DEFAULT_HARD[key], **kw))
            out[p + 'clamped'], out[p + 'margin'] = np.array(share), np.array(margin)
            assert margin > MARGIN, (p, margin)
            if tag == 'default' and norm:
                assert share == 0.0, (p, share)
            elif B >= 5:
                assert 0.2 <= share <= 0.8, (p, share)
            note = f' clamped {share:.2f} margin {margin:.2e}'
        print(f'{p} loss {float(l64):.6f} fp32 against fp64: loss {out[p + "err32"][0]:.2e} dz1 {out[p + "err32"][1]:.2e} '
              f'dz2 {out[p + "err32"][2]:.2e}{note}')
    path = os.path.join(HERE, 'hardneg.npz')
    write_npz(path, out)
    print('wrote hardneg.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
