"""Fixture of the contrastive monitoring metrics on offset, collapsed and aligned inputs: the UNMODIFIED reference classes of
trainer/metrics.py (imported as gen_golden_metrics.py imports them) on fp32 inputs and on the same inputs cast to fp64
-> tests/golden/metrics_edges.npz.

    python tests/golden/gen_golden_metrics_edges.py                 (prints err_ref = |v32 - v64| per value)
    python tests/golden/gen_golden_metrics_edges.py --find-seeds    (prints the first admissible seed per base, see below)

What is stored: per base (BASES below) the seeded fp32 arrays 'n1' [B1, D], 'n2' [B2, D] (randn * 0.2), 'off' [D] and 'row' [2, D] (randn),
once; 'values' [case, NAMES, (v32, v64)]; 'checks' [case, (sum z1, sum z1^2, sum z2, sum z2^2)] in fp64.  The inputs of a case are NOT
stored: build(base, family) derives them from the base arrays with IEEE fp32 additions and multiplications by constants (numpy,
elementwise, one rounding each: the same bits everywhere), the generator and the tests share it, and 'checks' pins what it built.

Families (noise = the base's randn * 0.2):
    plain        z1 = n1, z2 = 0.5 n1 + 0.5 n2 (the correlated views of gen_golden_metrics.py), appended rows: n2's
    offset30     plain + 30 off (one offset per column, both views);  offset300: plain + 300 off;  const30: plain + 30
    collapsed    z1 = row[0] + 0.005 n1, z2 = row[1] + 0.005 n2       (one common row per view + 1e-3 randn)
    aligned      z1 = n1, z2 = n1 + 0.005 n2                          (x2 = x1 + 1e-3 randn);  aligned_off: aligned + 30 off
    zero_row     plain with row 3 of z1 set to 0

Two conditions hold for every case (tests/test_metrics_edges_cpu.py asserts them): in fp64 no pair's (cos + 1) / 2 lies within
RATE_MARGIN of the threshold, so that an fp32 cosine (good to ~1e-6) must give the same three rates; and each view's fp64
log mean exp(-2 d^2) is above UNIFORMITY_MIN, so that the reference's fp32 exp does not underflow.  With independent rows the first
condition is a matter of the seed (at (96, 64) about a dozen of the 9216 cosines are expected inside the margin): a base's seed is the
first one from its starting value on for which all its cases satisfy both conditions - what --find-seeds prints.
"""
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

NAMES = ('positive_similarity', 'negative_similarity', 'contrastive_accuracy', 'true_negative_rate', 'true_positive_rate', 'uniformity',
         'alignment', 'batch_variance', 'dimension_covariance', 'mean_pred', 'std_pred', 'mean_targets', 'std_targets')
RATES = ('contrastive_accuracy', 'true_negative_rate', 'true_positive_rate')
THRESHOLD, T, ALPHA = 0.5009, 2, 2          # train.py:261-266
RATE_MARGIN = 1e-4
UNIFORMITY_MIN = -80.0

# base -> (B1, D, appended rows, seed).  (96, 64) has a base of its own for the aligned families: their cosines are other numbers than
# the plain family's, and one seed that suits both sets is out of reach.
BASES = {'b2': (2, 16, 0, 2000), 'b96': (96, 64, 0, 19845), 'b96a': (96, 64, 0, 51795), 'b257': (257, 64, 0, 25700),
         'b40': (40, 300, 0, 4000), 'b32': (32, 64, 32, 3200)}
SEARCH_FROM = {'b2': 2000, 'b96': 9600, 'b96a': 9700, 'b257': 25700, 'b40': 4000, 'b32': 3200}      # where --find-seeds starts
FAMILIES = ('plain', 'offset30', 'offset300', 'const30', 'collapsed', 'aligned', 'aligned_off', 'zero_row')
CASES = [('b96', f) for f in ('plain', 'offset30', 'offset300', 'const30', 'collapsed', 'zero_row')] + \
        [('b96a', f) for f in ('aligned', 'aligned_off')] + \
        [(b, f) for b in ('b2', 'b257', 'b40', 'b32') for f in ('offset30', 'collapsed', 'aligned_off')]


def case_tag(base, family):
    B1, D, extra, _ = BASES[base]
    return f'{B1}x{D}' + (f'+{extra}' if extra else '') + f'_{family}'


TAGS = [case_tag(b, f) for b, f in CASES]


def base_arrays(base, seed=None):
    B1, D, extra, s = BASES[base]
    g = torch.Generator().manual_seed(s if seed is None else seed)
    n1 = (torch.randn(B1, D, generator=g) * 0.2).numpy()
    n2 = (torch.randn(B1 + extra, D, generator=g) * 0.2).numpy()
    return {'n1': n1, 'n2': n2, 'off': torch.randn(D, generator=g).numpy(), 'row': torch.randn(2, D, generator=g).numpy()}


def fixture_bases(z):
    return {b: {k: z[f'base/{b}/{k}'] for k in ('n1', 'n2', 'off', 'row')} for b in BASES}


def build(arrays, family):
    """-> z1 [B1, D], z2 [B2, D] (fp32) of one family from a base's arrays; fp32 elementwise operations only"""
    f = np.float32
    n1, n2, off, row = (np.asarray(arrays[k], dtype=f) for k in ('n1', 'n2', 'off', 'row'))
    B1 = n1.shape[0]
    if family == 'collapsed':
        return row[0][None, :] + f(0.005) * n1, row[1][None, :] + f(0.005) * n2
    z1, z2 = n1.copy(), n2.copy()                     # rows from B1 on ("noisy samples appended at the end"): n2's
    if family in ('aligned', 'aligned_off'):
        z2[:B1] = n1 + f(0.005) * n2[:B1]
    else:
        z2[:B1] = f(0.5) * n1 + f(0.5) * n2[:B1]
    shift = {'offset30': f(30) * off, 'offset300': f(300) * off, 'aligned_off': f(30) * off, 'const30': f(30)}.get(family)
    if shift is not None:
        z1, z2 = z1 + shift, z2 + shift
    if family == 'zero_row':
        z1[3] = 0
    assert z1.dtype == f and z2.dtype == f
    return z1, z2


def checks(z1, z2):
    a, b = z1.astype(np.float64), z2.astype(np.float64)
    return np.array([a.sum(), (a * a).sum(), b.sum(), (b * b).sum()])


def rate_margin(z1, z2):
    """the smallest fp64 distance of a pair's (cos + 1) / 2 from the threshold (pairs with a NaN cosine have none)"""
    a, b = torch.tensor(z1, dtype=torch.float64), torch.tensor(z2, dtype=torch.float64)[:len(z1)]
    c = (a @ b.T) / torch.outer(a.norm(dim=1), b.norm(dim=1))
    d = ((c + 1) / 2 - THRESHOLD).abs()
    d = d[~torch.isnan(d)]
    return float(d.min()) if d.numel() else float('inf')


def log_potentials(z1, z2):
    """fp64 log mean exp(-t d^2) over the pairs of each view"""
    return [float(torch.log(torch.exp(-T * torch.pdist(torch.tensor(z, dtype=torch.float64)).pow(2)).mean())) for z in (z1, z2)]


def admissible(z1, z2):
    return rate_margin(z1, z2) > RATE_MARGIN and (len(z1) < 2 or min(log_potentials(z1, z2)) > UNIFORMITY_MIN)


def find_seed(base):
    seed = SEARCH_FROM[base]
    while True:
        arrays = base_arrays(base, seed)
        if all(admissible(*build(arrays, f)) for b, f in CASES if b == base):
            return seed
        seed += 1


def reference_values(metrics, z1, z2):
    """the reference's thirteen values on the tensors as they are (fp32 or fp64)"""
    v = {name: m(z1, z2).item() for name, m in metrics.items()}
    # the four statistics of SelfSupervisedTrainer.evaluate_metrics (trainer/self_supervised_trainer.py:33-36)
    v['mean_pred'], v['std_pred'] = torch.mean(z1).item(), torch.std(z1).item()
    v['mean_targets'], v['std_targets'] = torch.mean(z2).item(), torch.std(z2).item()
    return [float(v[name]) for name in NAMES]


def save(path, arrays):
    """np.savez_compressed with fixed member dates: the same bytes on every run"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, 'w') as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arrays[name]), allow_pickle=False)


def main():
    if '--find-seeds' in sys.argv:
        for base in BASES:
            print(base, find_seed(base), flush=True)
        return
    from gen_golden_metrics import import_reference_metrics
    M = import_reference_metrics()
    metrics = {'positive_similarity': M.PositiveSimilarity(), 'negative_similarity': M.NegativeSimilarity(),
               'contrastive_accuracy': M.ContrastiveAccuracy(threshold=THRESHOLD), 'true_negative_rate': M.TrueNegativeRate(threshold=THRESHOLD),
               'true_positive_rate': M.TruePositiveRate(threshold=THRESHOLD), 'uniformity': M.Uniformity(t=T),
               'alignment': M.Alignment(alpha=ALPHA), 'batch_variance': M.BatchVariance(), 'dimension_covariance': M.DimensionCovariance()}
    out = {}
    for base in BASES:
        for k, a in base_arrays(base).items():
            out[f'base/{base}/{k}'] = a
    values, chk = np.zeros((len(CASES), len(NAMES), 2)), np.zeros((len(CASES), 4))
    for i, (base, family) in enumerate(CASES):
        z1, z2 = build(base_arrays(base), family)
        assert admissible(z1, z2), (TAGS[i], rate_margin(z1, z2), log_potentials(z1, z2))
        chk[i] = checks(z1, z2)
        t1, t2 = torch.from_numpy(z1), torch.from_numpy(z2)
        values[i, :, 0] = reference_values(metrics, t1, t2)
        values[i, :, 1] = reference_values(metrics, t1.double(), t2.double())
        for m, name in enumerate(NAMES):
            v32, v64 = map(float, values[i, m])
            print(f'{TAGS[i]} {name}: fp32 {v32!r} fp64 {v64!r} err_ref {abs(v32 - v64):.3e}')
    out['values'], out['checks'] = values, chk
    path = os.path.join(HERE, 'metrics_edges.npz')
    save(path, out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
