"""SMP on the MI355X: the geometry, bases and triplet kernels of csrc/smp.hip against the host mirror (tests/smp_reference.py) in fp64,
the model against the reference's own fp32 and fp64 runs (tests/golden/gen_golden_smp.py), the fused triplet step against the
composed one, the absence of a [T, int_emb] tensor, and a short training run.

The bound is the project's (tests/test_gpu_san.py): max |device - fp64| <= max(4 x max |fp32 mirror - fp64|, 2^-20 x the tensor's
largest magnitude) per tensor, asserted as err / tol <= 1 and printed.  Triplets with a torsion candidate within 1e-4 of the 0 / 2 pi
wrap in fp64 are left out of the torsion and `t` comparisons (the minimum jumps there); at most 1 % of the triplets may be.

Measured on the device, worst err / tol per tensor over all cases: dist 0.05, angle 0.04, torsion 0.02, sbf 0.12, t 0.07 (30 of 24 716
triplets left out at the wrap); triplet kernels out 0.16, dx 0.20, ds8 0.12, dt8 0.17, dw1 0.006, dw2 0.009; model against the fixture,
fused / composed: a 0.49 / 0.68, b 0.28 / 0.28, c 0.43 / 0.53, d 0.34 / 0.34; fused against composed under the same tolerance: a 0.68, b 0.16,
c 0.22, d 0.07 (DESIGN.md, section SMP)."""
import copy
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from helpers import amd, load

import gen_golden_smp as GS
import smp_reference as R

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
smp = importlib.import_module('3dinfomax_amd.smp')
graph = importlib.import_module('3dinfomax_amd.graph')
DEV = torch.device('cuda:0')
CUTOFF = 5.0
WRAP = 1e-4


def _ratio(got, ref64, ref32, keep=None):
    """err / tol of one tensor under the bound of the module docstring; rows outside `keep` are left out on all three sides"""
    got, ref64, ref32 = (np.asarray(a, dtype=np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    if keep is not None:
        got, ref64, ref32 = got[keep], ref64[keep], ref32[keep]
    if ref64.size == 0:
        return 0.0, 0.0, 0.0
    err, own = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    tol = max(4 * own, 2.0 ** -20 * float(np.abs(ref64).max()))
    return (err / tol if tol > 0 else (0.0 if err == 0 else math.inf)), err, own


# ---- inputs, computed once -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _molecules(kind):
    if kind == 'six':          # six QM9-sized molecules
        mols = amd.synth.make_dataset(6, seed=11)
        return np.concatenate([m.coords for m in mols]), tuple(m.n_atoms for m in mols)
    if kind == 'six+pair':     # and a two-atom molecule: two edges without a triplet
        pos, sizes = _molecules('six')
        return np.concatenate([pos, np.array([[0, 0, 0], [1.2, 0.1, 0]], dtype=np.float32)]), sizes + (2,)
    if kind == 'cluster':      # 40 atoms inside the cutoff: the cap cuts
        return R.cluster(), (40,)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _lists(kind):
    pos, sizes = _molecules(kind)
    src, dst, in_ptr = R.radius_graph(pos, sizes, CUTOFF)
    idx_kj, idx_ji, trip_ptr = R.triplets(src, dst, in_ptr)
    return dict(src=src, dst=dst, in_ptr=in_ptr, idx_kj=idx_kj, idx_ji=idx_ji, trip_ptr=trip_ptr)


@functools.lru_cache(maxsize=None)
def _angles(kind, fp64):
    pos, _ = _molecules(kind)
    L = _lists(kind)
    return R.angles(pos, L['src'], L['dst'], L['in_ptr'], L['trip_ptr'], np.float64 if fp64 else np.float32)


def _device_geometry(kind):
    pos, sizes = _molecules(kind)
    p = torch.from_numpy(pos).to(DEV)
    batch = torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes)).to(DEV)
    return p, ops.smp_geometry(p, batch, len(sizes), CUTOFF)


def _geometry_of(L):
    """ops.SmpGeometry on the device from the mirror's lists"""
    geo = ops.SmpGeometry()
    i32 = lambda a: torch.from_numpy(np.asarray(a)).to(torch.int32).to(DEV)          # noqa: E731
    geo.N, geo.E, geo.T = L['in_ptr'].shape[0] - 1, L['src'].shape[0], L['idx_kj'].shape[0]
    geo.src, geo.dst, geo.in_ptr, geo.trip_ptr = i32(L['src']), i32(L['dst']), i32(L['in_ptr']), i32(L['trip_ptr'])
    geo.idx_kj, geo.idx_ji = i32(L['idx_kj']), i32(L['idx_ji'])
    order = np.argsort(L['idx_kj'], kind='stable')
    geo.kj_order = i32(order)
    geo.kj_ptr = i32(np.concatenate([[0], np.cumsum(np.bincount(L['idx_kj'], minlength=geo.E))]))
    geo.dist = None
    return geo


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['six', 'six+pair', 'cluster'])
def test_edge_and_triplet_lists_equal_the_mirrors(kind):
    L = _lists(kind)
    _, geo = _device_geometry(kind)
    E, T = L['src'].shape[0], L['idx_kj'].shape[0]
    print(f'smp lists {kind}: N {geo.N} E {E} T {T}')
    assert (geo.E, geo.T) == (E, T)
    if kind == 'six':
        assert 1000 < E < 2500 and 12000 < T < 30000
    src, dst = geo.src.cpu().numpy(), geo.dst.cpu().numpy()
    assert np.all(np.diff(dst) >= 0) and np.array_equal(geo.in_ptr.cpu().numpy(), L['in_ptr'])          # sorted by destination
    assert set(zip(src.tolist(), dst.tolist())) == set(zip(L['src'].tolist(), L['dst'].tolist())) and len(set(zip(src, dst))) == E
    assert np.array_equal(src, L['src']) and np.array_equal(dst, L['dst'])
    kj, ji, ptr = geo.idx_kj.cpu().numpy(), geo.idx_ji.cpu().numpy(), geo.trip_ptr.cpu().numpy()
    assert np.array_equal(ptr, L['trip_ptr'])
    for e in range(E):          # as sets per ji group
        a, b = ptr[e], ptr[e + 1]
        assert np.all(ji[a:b] == e) and set(kj[a:b].tolist()) == set(L['idx_kj'][a:b].tolist()) and len(set(kj[a:b].tolist())) == b - a
    # the kj regrouping: a permutation of the same list, every group holding its kj edge only
    order, kptr = geo.kj_order.cpu().numpy(), geo.kj_ptr.cpu().numpy()
    assert np.array_equal(np.sort(order), np.arange(T)) and kptr[0] == 0 and kptr[-1] == T
    assert np.array_equal(np.repeat(np.arange(E), np.diff(kptr)), kj[order])
    if kind == 'cluster':
        assert np.all(np.diff(L['in_ptr']) == R.MAX_NBR) and (0, 39) in set(zip(src.tolist(), dst.tolist())) and (39, 0) not in set(zip(src.tolist(), dst.tolist()))
    if kind == 'six+pair':
        assert np.all(np.diff(ptr)[-2:] == 0)


def test_empty_inputs_launch_nothing_and_return_shaped_empties():
    tabs = [torch.from_numpy(a).to(DEV) for a in smp._BasisTables(3, 2, CUTOFF).host]
    none = torch.zeros(0, 3, device=DEV)
    geo = ops.smp_geometry(none, torch.zeros(0, dtype=torch.long, device=DEV), 0, CUTOFF)                       # N = 0
    assert (geo.N, geo.E, geo.T) == (0, 0, 0) and geo.in_ptr.tolist() == [0] and geo.trip_ptr.tolist() == [0] and geo.src.shape == (0,)
    far = torch.tensor([[0., 0, 0], [9, 0, 0], [0, 9, 0]], device=DEV)
    geo = ops.smp_geometry(far, torch.tensor([0, 0, 1], device=DEV), 2, CUTOFF)                                # E = 0
    assert (geo.N, geo.E, geo.T) == (3, 0, 0) and geo.in_ptr.tolist() == [0, 0, 0, 0] and geo.kj_ptr.tolist() == [0]
    angle, torsion, sbf, t = ops.smp_bases(far, geo, 3, 2, CUTOFF, *tabs)
    assert angle.shape == (0,) and torsion.shape == (0,) and sbf.shape == (0, 6) and t.shape == (0, 18)
    pair = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0]], device=DEV)
    geo = ops.smp_geometry(pair, torch.tensor([0, 0, 1, 1], device=DEV), 2, CUTOFF)                            # T = 0
    assert (geo.E, geo.T) == (4, 0) and geo.src.tolist() == [1, 0, 3, 2] and geo.trip_ptr.tolist() == [0] * 5 and geo.kj_ptr.tolist() == [0] * 5
    assert torch.allclose(geo.dist, torch.ones(4, device=DEV))
    assert ops.smp_bases(pair, geo, 3, 2, CUTOFF, *tabs)[3].shape == (0, 18)
    x, w = torch.randn(4, 24, device=DEV), torch.randn(24, 4, device=DEV)
    s8 = torch.zeros(0, 4, device=DEV)
    out = ops.smp_triplets_fwd(x, s8, s8, w, w, geo)
    assert out.shape == (4, 24) and torch.count_nonzero(out) == 0
    grads = ops.smp_triplets_bwd(torch.ones_like(x), x, s8, s8, w, w, geo)
    assert [g.shape for g in grads] == [x.shape, s8.shape, s8.shape, w.shape, w.shape] and all(torch.count_nonzero(g) == 0 for g in grads)


@pytest.mark.parametrize('n, k', [(n, k) for n in (1, 3, 7) for k in (1, 6)])
def test_angles_torsions_and_bases_against_fp64(n, k):
    kind = 'six'
    pos, sizes = _molecules(kind)
    L = _lists(kind)
    d64, a64, t64, margin, single = _angles(kind, True)
    d32, a32, t32, _, _ = _angles(kind, False)
    keep = margin >= WRAP
    left_out = int((~keep).sum())
    print(f'smp bases n={n} k={k}: T {keep.shape[0]}, left out at the wrap {left_out}')
    assert left_out <= 0.01 * keep.shape[0]
    host = smp._BasisTables(n, k, CUTOFF).host          # zeros, normalisers (rounded as the reference rounds them), prefactors
    s64, b64 = R.bases(d64, a64, t64, L['idx_kj'], n, k, CUTOFF, np.float64, host[:2])
    s32, b32 = R.bases(d32, a32, t32, L['idx_kj'], n, k, CUTOFF, np.float32, host[:2])
    p, geo = _device_geometry(kind)
    tabs = [torch.from_numpy(a).to(DEV) for a in host]
    angle, torsion, sbf, t = (a.cpu().numpy() for a in ops.smp_bases(p, geo, n, k, CUTOFF, *tabs))
    assert sbf.shape == (geo.T, n * k) and t.shape == (geo.T, n * n * k) and sbf.dtype == np.float32
    worst = {}
    for name, got, r64, r32, rows in (('dist', geo.dist.cpu().numpy(), d64, d32, None), ('angle', angle, a64, a32, None),
                                      ('torsion', torsion, t64, t32, keep), ('sbf', sbf, s64, s32, None), ('t', t, b64, b32, keep)):
        worst[name], err, own = _ratio(got, r64, r32, rows)
        print(f'smp bases n={n} k={k} {name}: err {err:.3e} fp32 mirror {own:.3e} err/tol {worst[name]:.3f}')
    assert max(worst.values()) <= 1.0, worst
    # k_n == k is the only candidate: exactly 2 pi
    assert single.sum() > 0 and np.all(torsion[single] == np.float32(2 * math.pi))
    assert np.all(torsion > 0) and np.all(torsion <= np.float32(2 * math.pi))


# ---- the triplet kernels ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _interaction_case(I, Bs):
    L = _lists('six+pair')
    c = R.make_interaction_case(I, Bs, 3, L)
    kj, ji = torch.from_numpy(L['idx_kj']), torch.from_numpy(L['idx_ji'])
    ref = R.interaction(c['x'], c['s8'], c['t8'], c['w1'], c['w2'], kj, ji, c['grad'], torch.float64)
    own = R.interaction(c['x'], c['s8'], c['t8'], c['w1'], c['w2'], kj, ji, c['grad'], torch.float32)
    return L, c, ref, own


def _device_interaction(c, geo):
    d = {k: v.to(DEV) for k, v in c.items()}
    out = ops.smp_triplets_fwd(d['x'], d['s8'], d['t8'], d['w1'], d['w2'], geo)
    dx, ds8, dt8, dw1, dw2 = ops.smp_triplets_bwd(d['grad'], d['x'], d['s8'], d['t8'], d['w1'], d['w2'], geo)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dict(out=out, dx=dx, ds8=ds8, dt8=dt8, dw1=dw1, dw2=dw2).items()}


@pytest.mark.parametrize('I, Bs', R.SHAPES)
def test_triplet_kernels_against_fp64(I, Bs):
    assert ops.smp_triplets_takes(I, Bs)
    L, c, ref, own = _interaction_case(I, Bs)
    geo = _geometry_of(L)
    got = _device_interaction(c, geo)
    assert set(got) == set(ref)
    worst = {}
    for k in ref:
        worst[k], err, o = _ratio(got[k].numpy(), ref[k].numpy(), own[k].numpy())
        print(f'smp triplets I={I} Bs={Bs} {k}: err {err:.3e} fp32 mirror {o:.3e} err/tol {worst[k]:.3f}')
    assert max(worst.values()) <= 1.0, worst
    empty = np.nonzero(np.diff(L['trip_ptr']) == 0)[0]
    assert len(empty) >= 2 and all(torch.count_nonzero(got['out'][e]) == 0 for e in empty)          # an edge without triplets
    unused = np.nonzero(np.bincount(L['idx_kj'], minlength=geo.E) == 0)[0]
    assert len(unused) >= 2 and all(torch.count_nonzero(got['dx'][e]) == 0 for e in unused)
    again = _device_interaction(c, geo)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_shapes_outside_the_lane_map_are_not_taken():
    assert ops.smp_triplets_takes(64, 8) and ops.smp_triplets_takes(24, 4) and ops.smp_triplets_takes(128, 8) and ops.smp_triplets_takes(256, 8)
    assert not ops.smp_triplets_takes(257, 8) and not ops.smp_triplets_takes(64, 9) and not ops.smp_triplets_takes(72, 20)
    with pytest.raises(ValueError):
        ops.smp_triplets_takes(0, 8)
    L = _lists('six+pair')
    geo = _geometry_of(L)
    x, s8, w = torch.randn(geo.E, 72, device=DEV), torch.randn(geo.T, 20, device=DEV), torch.randn(72, 20, device=DEV)
    assert ops.smp_triplets_fwd(x, s8, s8, w, w, geo) is None


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _model_and_batch(cfg):
    import test_smp_cpu as C
    z = load('smp.npz')
    return z, C.model_of(z, cfg).to(DEV), C.batch_of(z, cfg, DEV), C


@pytest.mark.parametrize('cfg', sorted(GS.CONFIGS))
def test_model_matches_the_fixture(cfg):
    z, model, data, C = _model_and_batch(cfg)
    C.check_against_fixture(model, data, z, cfg, 'fused')
    want = 'fused' if ops.smp_triplets_takes(GS.CONFIGS[cfg]['int_emb_size'], GS.CONFIGS[cfg]['basis_emb_size']) else 'composed'
    assert all(layer.path == want for layer in model.update_es) and (want == 'composed') == (cfg == 'd')
    geo, _ = model.geometry(data)
    for ours, theirs in (('src', 'j'), ('dst', 'i'), ('idx_kj', 'idx_kj'), ('idx_ji', 'idx_ji')):
        assert np.array_equal(getattr(geo, ours).cpu().numpy(), z[f'{cfg}/{theirs}']), ours


@pytest.mark.parametrize('cfg', sorted(GS.CONFIGS))
def test_composed_path_matches_the_fixture_too(cfg, monkeypatch):
    """the fused path against the composed one under the same bound: both have to stay within it of the reference's fp64 run"""
    z, model, data, C = _model_and_batch(cfg)
    monkeypatch.setattr(smp, 'FUSED_TRIPLETS', False)
    C.check_against_fixture(model, data, z, cfg, 'composed')
    assert all(layer.path == 'composed' for layer in model.update_es)


@pytest.mark.parametrize('cfg', sorted(GS.CONFIGS))
def test_fused_equals_composed_under_the_same_bound(cfg, monkeypatch):
    """the same model and batch with FUSED_TRIPLETS on and off: |fused - composed| within the fixture's bound of every tensor"""
    z, model, data, C = _model_and_batch(cfg)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(smp, 'FUSED_TRIPLETS', fused)
        res[fused] = C.outputs_of(copy.deepcopy(model), data, z, cfg)
    ratios = {}
    for k in res[True]:
        key32, key64 = C.fixture_keys(cfg, k)
        tol = C.bound(z[key32], z[key64])
        err = float(np.abs(res[True][k].astype(np.float64) - res[False][k]).max())
        ratios[k] = err / tol if tol > 0 else (0.0 if err == 0 else math.inf)
    worst = max(ratios, key=ratios.get)
    print(f'smp model {cfg} fused against composed: worst |difference| / tol {ratios[worst]:.3f} ({worst}), u {ratios["u"]:.3f}')
    assert ratios[worst] <= 1.0, {k: v for k, v in ratios.items() if v > 1.0}


def test_no_triplet_wide_tensor():
    """one fused forward + backward of the triplet step at T ~ 19 k, I = 64, Bs = 8: the peak of allocated memory rises by less than
    one [T, I] fp32 tensor over the level before the call"""
    L, c, _, _ = _interaction_case(64, 8)
    geo = _geometry_of(L)
    d = {k: v.to(DEV) for k, v in c.items()}

    def step():
        out = ops.smp_triplets_fwd(d['x'], d['s8'], d['t8'], d['w1'], d['w2'], geo)
        return out, ops.smp_triplets_bwd(d['grad'], d['x'], d['s8'], d['t8'], d['w1'], d['w2'], geo)

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, grads = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f'smp triplets fwd + bwd: T {geo.T}, peak rise {rise / 2 ** 20:.2f} MiB, one [T, I] tensor {geo.T * 64 * 4 / 2 ** 20:.2f} MiB')
    assert geo.T > 15000 and rise < geo.T * 64 * 4
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads)


def test_training_lowers_the_loss():
    z, model, data, C = _model_and_batch('a')
    target = torch.from_numpy(z['a/target']).to(DEV)
    opt = amd.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = torch.nn.L1Loss()(model(data), target)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print('smp training losses', [round(v, 4) for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_isolated_atoms_get_zero_rows_and_the_collate_feeds_the_model():
    mols = amd.synth.make_dataset(3, seed=4)
    lone = copy.deepcopy(mols[1])
    lone.n_atoms, lone.atom_feat, lone.coords = 1, lone.atom_feat[:1], lone.coords[:1]
    far = copy.deepcopy(mols[2])
    far.coords = far.coords.copy()
    far.coords[-1] += 50.0                                                # the LAST atom of the batch has no edge
    [data], y = graph.pytorch_geometric_collate([(m, torch.zeros(1)) for m in (mols[0], lone, far)])
    torch.manual_seed(0)
    model = smp.SMP(**GS.CONFIGS['c']).to(DEV)
    data = data.to(DEV)
    geo, B = model.geometry(data)
    deg = np.diff(geo.in_ptr.cpu().numpy())
    n0 = mols[0].n_atoms
    assert B == 3 and deg[n0] == 0 and deg[-1] == 0
    seen = []
    model.init_v.lin_up.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    u = model(data)
    assert u.shape == (3, 2) and torch.isfinite(u).all()
    assert seen[0].shape[0] == data.num_nodes and torch.count_nonzero(seen[0][n0]) == 0 and torch.count_nonzero(seen[0][-1]) == 0
