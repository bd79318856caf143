"""-m gpu: the plugin modules (PNA / PNALayer / Net3D / NT-Xent) running on the HIP kernels against the golden
fixtures produced by the reference itself (tests/golden/gen_golden.py) and against the oracle on bigger batches.
Bar: BASELINE.json:north_star - node embeddings and loss within 1e-4 relative fp32."""
import copy
import importlib
import os

import math
import numpy as np
import pytest
import torch

from fill import det_fill
from helpers import (NET3D_SMALL, NET3D_YML, PNA_SMALL, PNA_YML, close, grads_close, grads_close_l2, hip_routing, load, routing_flips,
                     mols_from_npz, rel_err, sd_from_npz, synth)
from oracle import pna3d_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope='module')
def amd():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return importlib.import_module('3dinfomax_amd')


def make_batch(amd, mols, device='cuda:0'):
    g2 = amd.batch([amd.bond_graph(m) for m in mols]).to(device)
    g3 = amd.batch([amd.complete_graph(m) for m in mols]).to(device)
    return g2, g3


def param_grads(module):
    return {k: p.grad for k, p in module.named_parameters()}


@pytest.mark.parametrize('regime', ['init', 'trained'])
def test_pna_layer_vs_reference_fixture(amd, regime):
    z = load('pna_layer.npz')
    F = 8
    layer = amd.PNALayer(in_dim=F, out_dim=F, in_dim_edges=F, aggregators=['mean', 'max', 'min', 'std'],
                         scalers=['identity', 'amplification', 'attenuation'], mid_batch_norm=True,
                         last_batch_norm=True, batch_norm_momentum=0.93, posttrans_layers=1, pretrans_layers=2)
    layer.load_state_dict(sd_from_npz(z, f'{regime}/sd'), strict=True)
    layer.cuda().train()
    g = amd.BatchedMolGraph(torch.from_numpy(z['src']), torch.from_numpy(z['dst']), int(z['n'])).to('cuda:0')
    h = torch.from_numpy(z['h']).cuda().requires_grad_(True)
    ef = torch.from_numpy(z['ef']).cuda().requires_grad_(True)
    g.ndata['feat'], g.edata['feat'] = h, ef
    out = layer(g)
    assert rel_err(out.cpu(), z[f'{regime}/h_out']) < TOL
    (out * torch.from_numpy(z[f'{regime}/cot']).cuda()).sum().backward()
    assert rel_err(h.grad.cpu(), z[f'{regime}/grad_h']) < 2e-4
    assert rel_err(ef.grad.cpu(), z[f'{regime}/grad_ef']) < 2e-4
    grads_close(param_grads(layer), sd_from_npz(z, f'{regime}/grad'), 2e-4)
    for k, v in sd_from_npz(z, f'{regime}/sd_after').items():
        if 'running' in k:
            assert close(layer.state_dict()[k], v, TOL, 1e-6), k


@pytest.mark.parametrize('regime', ['init', 'trained'])
def test_pna_and_net3d_vs_reference_fixture(amd, regime):
    z = load('models_small.npz')
    mols = mols_from_npz(z)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **PNA_SMALL)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_SMALL)
    # the reference's own state_dict loads strictly: identical keys and shapes
    pna.load_state_dict(sd_from_npz(z, f'{regime}/pna_sd'), strict=True)
    net.load_state_dict(sd_from_npz(z, f'{regime}/net3d_sd'), strict=True)
    pna.cuda().train(), net.cuda().train()
    g2, g3 = make_batch(amd, mols)
    z2, z3 = pna(g2), net(g3)
    assert rel_err(g2.ndata['feat'].cpu(), z[f'{regime}/pna_node_emb']) < TOL     # the side effect tensor
    assert rel_err(z2.cpu(), z[f'{regime}/pna_out']) < TOL
    assert rel_err(g3.ndata['feat'].cpu(), z[f'{regime}/net3d_node_emb']) < TOL
    assert rel_err(z3.cpu(), z[f'{regime}/net3d_out']) < TOL
    c2, c3 = torch.from_numpy(z[f'{regime}/cot2']).cuda(), torch.from_numpy(z[f'{regime}/cot3']).cuda()
    ((z2 * c2).sum() + (z3 * c3).sum()).backward()
    grads_close(param_grads(pna), sd_from_npz(z, f'{regime}/pna_grad'), 5e-4, 'pna ')
    grads_close(param_grads(net), sd_from_npz(z, f'{regime}/net3d_grad'), 5e-4, 'net3d ')
    for tag, mod in (('pna_sd_after', pna), ('net3d_sd_after', net)):
        sd = mod.state_dict()
        for k, v in sd_from_npz(z, f'{regime}/{tag}').items():
            if 'running' in k or 'num_batches' in k:
                assert close(sd[k], v, TOL, 1e-6), k
    pna.eval(), net.eval()
    g2, g3 = make_batch(amd, mols)
    with torch.no_grad():
        assert rel_err(pna(g2).cpu(), z[f'{regime}/pna_out_eval']) < TOL
        assert rel_err(net(g3).cpu(), z[f'{regime}/net3d_out_eval']) < TOL


@pytest.mark.parametrize('fixture', ['train3.npz', 'trainer3.npz'])
def test_three_adam_steps_vs_reference_fixture(amd, fixture):
    # train3.npz: a hand-written loop around the reference modules; trainer3.npz: the same three steps driven through
    # the reference's own SelfSupervisedTrainer.process_batch / forward_pass / initialize_optimizer and its
    # contrastive_collate (tests/golden/gen_golden_host.py) - SURVEY.md row a13
    z = load(fixture)
    mols = mols_from_npz(z)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **PNA_SMALL)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_SMALL)
    pna.load_state_dict(sd_from_npz(z, 'pna_sd'))
    net.load_state_dict(sd_from_npz(z, 'net3d_sd'))
    pna.cuda().train(), net.cuda().train()
    loss_fn = amd.NTXent(tau=0.1)
    named = list(pna.named_parameters()) + list(net.named_parameters())
    # the reference trainer builds `optim(param_groups, **optimizer_params)` by name: torch's class for one fixture, the
    # plugin's (one-launch kernel of csrc/adam.hip) for the other
    adam_cls = amd.Adam if fixture == 'trainer3.npz' else torch.optim.Adam
    optim = adam_cls([{'params': [p for k, p in named if 'batch_norm' in k], 'weight_decay': 0},
                      {'params': [p for k, p in named if 'batch_norm' not in k]}], lr=8e-5)
    g2, g3 = make_batch(amd, mols)
    losses = []
    for _ in range(3):
        a, b = g2.local_copy(), g3.local_copy()
        loss = loss_fn(pna(a), net(b), nodes_per_graph=a.batch_num_nodes())
        loss.backward()
        optim.step()
        optim.zero_grad()
        losses.append(loss.item())
    np.testing.assert_allclose(losses, z['losses'], rtol=1e-4)      # loss within 1e-4 of the reference
    if 'optim_group_sizes' in z.files:
        assert list(z['optim_group_sizes']) == [len(g['params']) for g in optim.param_groups]
    for tag, m in (('pna_sd_final', pna), ('net3d_sd_final', net)):
        for k, p in m.named_parameters():
            # weights only: a bias in front of a BatchNorm has an analytically zero gradient, Adam turns its rounding
            # noise into +-lr steps in every implementation (tests/test_oracle_golden.py)
            if k.endswith('.weight'):
                assert close(p.detach(), z[f'{tag}/{k}'], 1e-4, 2e-5), k


def test_three_adam_steps_in_the_bf16_matmul_mode_vs_reference_fixture(amd):
    """The three optimisation steps of train3.npz (the reference's fp32 trajectory) in the bf16 MATMUL mode (configs[3]'s mode:
    bf16-rounded operands on the bf16 matrix pipe, fp32 accumulation, fp32 tensors / statistics / master weights): what a
    user of that mode gets instead of the fp32 losses - every loss of the trajectory within BF16_TRAJ_TOL of the reference's."""
    ops = importlib.import_module('3dinfomax_amd.ops')
    z = load('train3.npz')
    mols = mols_from_npz(z)
    prev = ops.set_matmul_precision('bf16')
    try:
        pna = amd.PNA(avg_d=1.0, device='cuda:0', **PNA_SMALL)
        net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_SMALL)
        pna.load_state_dict(sd_from_npz(z, 'pna_sd'))
        net.load_state_dict(sd_from_npz(z, 'net3d_sd'))
        pna.cuda().train(), net.cuda().train()
        loss_fn = amd.NTXent(tau=0.1)
        named = list(pna.named_parameters()) + list(net.named_parameters())
        optim = amd.Adam([{'params': [p for k, p in named if 'batch_norm' in k], 'weight_decay': 0},
                          {'params': [p for k, p in named if 'batch_norm' not in k]}], lr=8e-5)
        g2, g3 = make_batch(amd, mols)
        losses = []
        for _ in range(3):
            a, b = g2.local_copy(), g3.local_copy()
            loss = loss_fn(pna(a), net(b), nodes_per_graph=a.batch_num_nodes())
            loss.backward()
            optim.step()
            optim.zero_grad()
            losses.append(loss.item())
    finally:
        ops.set_matmul_precision(prev)
    ref = np.asarray(z['losses'], dtype=np.float64)
    rel = np.abs(np.asarray(losses) - ref) / np.abs(ref)
    print('bf16 matmul mode, three Adam steps: losses', losses, 'reference', list(ref), 'relative', list(rel))
    assert float(rel.max()) < BF16_TRAJ_TOL, (losses, list(ref))
    # and the trajectory moves the way the reference's does (same sign of every step-to-step change that is above the bound)
    for i in range(2):
        if abs(ref[i + 1] - ref[i]) > 2 * BF16_TRAJ_TOL * abs(ref[i]):
            assert (losses[i + 1] - losses[i]) * (ref[i + 1] - ref[i]) > 0


BF16_TRAJ_TOL = 2e-2      # relative, per loss of the trajectory (measured 1.2e-4 / 3.5e-3 / 9.4e-3 on steps 1 / 2 / 3)


def _det_load(module, tag):
    new = {}
    for k, v in module.state_dict().items():
        if k.endswith('num_batches_tracked'):
            new[k] = v
        elif k.endswith('running_var') or k.endswith('batch_norm.weight'):
            new[k] = torch.from_numpy(det_fill(tuple(v.shape), f'{tag}/{k}', 0.2, 1.0))
        elif k.endswith('linear.weight'):
            new[k] = torch.from_numpy(det_fill(tuple(v.shape), f'{tag}/{k}', 1.2 / np.sqrt(v.shape[1])))
        elif 'embedding_list' in k or k == 'node_embedding':
            new[k] = torch.from_numpy(det_fill(tuple(v.shape), f'{tag}/{k}', 1.0))
        else:
            new[k] = torch.from_numpy(det_fill(tuple(v.shape), f'{tag}/{k}', 0.2))
    module.load_state_dict(new)


def _products(amd, request, wgrad, monkeypatch):
    """'exact': the fp32 mode's default (three-part split of both operands, six part products: csrc/gemm.hip); 'native_mfma':
    v_mfma_f32_32x32x2_f32 / 16x16x4_f32 everywhere; 'split_bf16': round 3's two-part split of the weight gradients (opt-in)"""
    if wgrad == 'split_bf16':
        monkeypatch.setenv('I3D_WGRAD_SPLIT_BF16', '1')
    if wgrad == 'native_mfma':
        prev = amd.set_fp32_products('native')
        request.addfinalizer(lambda: amd.set_fp32_products(prev))
    assert amd.get_fp32_products() == ('native' if wgrad == 'native_mfma' else 'split')


@pytest.mark.parametrize('L,wgrad', [(7, 'exact'), (4, 'exact'), (4, 'split_bf16'), (4, 'native_mfma')])
def test_full_yml_config_vs_reference_fixture(amd, L, wgrad, monkeypatch, request):
    """pre-train_QM9.yml dimensions (F=200, target 256; L=7 as in the yml, L=4 as in BASELINE.json), with every way the fp32 mode
    forms its products (_products) - the same bounds."""
    _products(amd, request, wgrad, monkeypatch)
    z = load('full_config.npz')
    mols = mols_from_npz(z)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **dict(PNA_YML, propagation_depth=L))
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_YML)
    _det_load(pna, f'pna{L}')
    _det_load(net, 'net3d')
    pna.cuda().train(), net.cuda().train()
    g2, g3 = make_batch(amd, mols)
    z2, z3 = pna(g2), net(g3)
    loss = amd.NTXent(tau=0.1)(z2, z3)
    loss.backward()
    assert abs(loss.item() - float(z[f'L{L}/loss'])) < TOL * abs(float(z[f'L{L}/loss']))
    assert rel_err(z2.cpu(), z[f'L{L}/pna_out']) < TOL
    assert rel_err(z3.cpu(), z[f'L{L}/net3d_out']) < TOL
    emb = g2.ndata['feat']
    assert rel_err(emb[::7].cpu(), z[f'L{L}/node_emb_rows']) < TOL
    w = pna.node_gnn.mp_layers[0].posttrans.fully_connected[0].linear.weight.grad
    assert rel_err(w[::16, ::64].cpu(), z[f'L{L}/pna_grad_sample/post0_w']) < 2e-3
    w = pna.node_gnn.mp_layers[L - 1].pretrans.fully_connected[0].linear.weight.grad
    assert rel_err(w[::16, ::32].cpu(), z[f'L{L}/pna_grad_sample/preL_w']) < 2e-3
    ref = {k: z[f'L{L}/net3d_grad/{k}'] for k, _ in net.named_parameters()}
    grads_close(param_grads(net), ref, 2e-3, 'net3d ')


@pytest.mark.parametrize('wgrad', ['exact', 'split_bf16', 'native_mfma'])
def test_batch64_vs_oracle_fwd_bwd(amd, wgrad, monkeypatch, request):
    """A bigger seeded batch (64 QM9-shaped molecules, F=200, L=2): forward, loss, and every parameter gradient
    against the oracle - with every way the fp32 mode forms its products (_products), same bounds."""
    _products(amd, request, wgrad, monkeypatch)
    mols = synth.make_dataset(64, seed=5)
    kw2 = dict(PNA_YML, propagation_depth=2)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **kw2)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_YML)
    _det_load(pna, 'pnaX')
    _det_load(net, 'net3dX')
    P2 = O.require_grad({k: v.clone() for k, v in pna.state_dict().items()})
    P3 = O.require_grad({k: v.clone() for k, v in net.state_dict().items()})
    og2, og3 = O.graphs_from_molecules(mols)
    r2, remb = O.pna_forward(og2, P2, O.pna_config(**kw2), True)
    r3, _ = O.net3d_forward(og3, P3, O.net3d_config(**NET3D_YML), True)
    rloss = O.ntxent(r2, r3, 0.1)
    rloss.backward()
    pna.cuda().train(), net.cuda().train()
    g2, g3 = make_batch(amd, mols)
    z2, z3 = pna(g2), net(g3)
    loss = amd.NTXent(tau=0.1)(z2, z3)
    loss.backward()
    assert abs(loss.item() - rloss.item()) < TOL * abs(rloss.item())
    assert rel_err(g2.ndata['feat'].cpu(), remb.detach()) < TOL
    assert rel_err(z2.cpu(), r2.detach()) < TOL and rel_err(z3.cpu(), r3.detach()) < TOL
    grads_close(param_grads(pna), {k: P2[k].grad for k in O.trainable(P2)}, 1e-3, 'pna ')
    grads_close(param_grads(net), {k: P3[k].grad for k in O.trainable(P3)}, 1e-3, 'net3d ')


@pytest.mark.parametrize('composite,fused_model,native', [(True, True, True), (True, True, False), (False, True, True),
                                                          (False, False, False), (True, False, True)])
def test_bond_table_path_matches_dense_bond_embeddings(amd, composite, fused_model, native, monkeypatch):
    """The [60, F] table of all bond-category combinations + per-edge codes (default) against materialised [E, F] bond
    embeddings multiplied by W_q in every layer (I3D_EDGE_TABLE=0): same outputs, side effects and gradients."""
    pna_mod = importlib.import_module('3dinfomax_amd.pna')
    layers_mod = importlib.import_module('3dinfomax_amd.layers')
    if not composite:       # one C call per block vs one per kernel
        monkeypatch.setattr(layers_mod, '_composite_ok', lambda *a, **k: False)
    if not native:          # one C call per layer vs the block Functions sequenced by pna.PNALayerFn
        monkeypatch.setattr(importlib.import_module('3dinfomax_amd.layer_native'), 'eligible', lambda *a, **k: False)
    if not fused_model:     # one autograd node per model vs one per layer
        monkeypatch.setattr(importlib.import_module('3dinfomax_amd.tape'), 'run_model', lambda module, run: run())
    if not (native and fused_model):    # the model C call stands on both
        monkeypatch.setattr(importlib.import_module('3dinfomax_amd.pna_native'), 'eligible', lambda *a, **k: False)
    mols = synth.make_dataset(48, seed=11)
    kw2 = dict(PNA_YML, propagation_depth=2)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **kw2)
    _det_load(pna, 'pnaT')
    pna.cuda().train()
    res = {}
    for mode in (True, False):
        monkeypatch.setattr(pna_mod, 'EDGE_TABLE', mode)
        pna.zero_grad()
        g2, _ = make_batch(amd, mols)
        z = pna(g2)
        (z * z).sum().backward()
        res[mode] = (z.detach().cpu(), g2.ndata['feat'].detach().cpu(), g2.edata['feat'].detach().cpu(),
                     {k: v.cpu() for k, v in param_grads(pna).items()})
    for i in range(3):
        assert rel_err(res[True][i], res[False][i]) < 1e-5, i
    grads_close(res[True][3], res[False][3], 1e-4, 'pna ')


@pytest.mark.parametrize('case', ['pretrans_2', 'posttrans_2', 'silu'])
def test_layer_planner_on_more_layer_shapes(amd, case, monkeypatch):
    """Both sequencers place a layer's buffers through one planner (i3d_pna_layer_place_fwd / _bwd); one forward and backward of a
    small model on layer shapes the tests above do not reach.  Two pretrans blocks: the whole-model C call against the
    Python-sequenced layer C calls, the same bits in the output, the node embeddings and every parameter gradient.  Two posttrans
    blocks, and an activation that keeps the Linear's output (the non-fused layer form: y of every pretrans block, pre_keep, the
    chain of plain posttrans blocks): the layer C call against the block path, the same bits in the output and the node
    embeddings.  Their parameter gradients are not the same bits, before the planner either (24 of 50 and 17 of 42 tensors equal:
    the layer call sums the weight gradients in one launch, the blocks in one per product), and are held to the bound
    test_bond_table_path_matches_dense_bond_embeddings sets between these two paths."""
    native = importlib.import_module('3dinfomax_amd.pna_native')
    layer_native = importlib.import_module('3dinfomax_amd.layer_native')
    kw = dict(PNA_SMALL, **{'pretrans_2': dict(pretrans_layers=2), 'posttrans_2': dict(posttrans_layers=2),
                            'silu': dict(activation='silu')}[case])
    mols = synth.make_dataset(24, seed=17)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **kw)
    _det_load(pna, 'pnaPlan')
    pna.cuda().train()
    sd0 = {k: v.clone() for k, v in pna.state_dict().items()}
    calls = []
    real_forward, real_eligible = layer_native.forward, layer_native.eligible
    monkeypatch.setattr(layer_native, 'forward', lambda *a, **k: (calls.append(1), real_forward(*a, **k))[1])

    def run(model_call, layer_call):
        monkeypatch.setattr(native, 'NATIVE_MODEL', model_call)
        monkeypatch.setattr(layer_native, 'eligible', real_eligible if layer_call else (lambda *a, **k: False))
        pna.load_state_dict(sd0)
        pna.zero_grad(set_to_none=True)
        g2, _ = make_batch(amd, mols)
        z = pna(g2)
        (z * z).sum().backward()
        return z.detach().clone(), g2.ndata['feat'].detach().clone(), {k: v.clone() for k, v in param_grads(pna).items()}
    if case == 'pretrans_2':
        ref = run(True, True)
        assert calls == [], 'the model C call takes this pass'
        res = run(False, True)
    else:
        res, ref = run(False, True), run(False, False)
    assert len(calls) == kw['propagation_depth'], 'the layer C call must take every layer of one pass, and of one only'
    assert torch.equal(res[0], ref[0]) and torch.equal(res[1], ref[1])
    assert sorted(res[2]) == sorted(ref[2]) and len(res[2]) > 20
    if case == 'pretrans_2':
        for k in res[2]:
            assert torch.equal(res[2][k], ref[2][k]), k
    else:
        grads_close({k: v.cpu() for k, v in res[2].items()}, {k: v.cpu() for k, v in ref[2].items()}, 1e-4, 'pna ')


def _star(n_leaves, seed):
    """a centre atom bonded to n_leaves atoms (in-degree n_leaves at the centre, 1 at the leaves)"""
    rng = np.random.default_rng(seed)
    n = n_leaves + 1
    src = np.concatenate([np.zeros(n_leaves, np.int64), np.arange(1, n, dtype=np.int64)])
    dst = np.concatenate([np.arange(1, n, dtype=np.int64), np.zeros(n_leaves, np.int64)])
    order = rng.permutation(len(src))                       # edge ids in arbitrary order
    return synth.Molecule(n, src[order], dst[order],
                          np.stack([rng.integers(0, d, n) for d in synth.ATOM_FEATURE_DIMS], 1).astype(np.int64),
                          np.stack([rng.integers(0, d, len(src)) for d in synth.BOND_FEATURE_DIMS], 1).astype(np.int64),
                          rng.normal(0, 1.5, (n, 3)).astype(np.float32))


def _lonely(seed):
    """a single atom: no bonds (in-degree 0: DGL leaves zero rows), a one-node complete graph without edges"""
    rng = np.random.default_rng(seed)
    return synth.Molecule(1, np.zeros(0, np.int64), np.zeros(0, np.int64),
                          np.stack([rng.integers(0, d, 1) for d in synth.ATOM_FEATURE_DIMS], 1).astype(np.int64),
                          np.zeros((0, 3), np.int64), rng.normal(0, 1.5, (1, 3)).astype(np.float32))


@pytest.mark.parametrize('case', ['ragged', 'tiny_batch', 'wide_degrees'])
def test_edge_case_batches_vs_oracle(amd, case):
    """Ragged and degenerate batches through the whole fast path (native layer, tape, side stream) against the oracle:
    isolated atoms (in-degree 0, a graph without edges), two-atom molecules, a hub of in-degree 33 (beyond the 32-entry
    scaler table), many distinct degrees (> 5 degree groups), a batch of six large graphs (one graph in training mode is an
    error in the reference too: BatchNorm over a single row)."""
    if case == 'ragged':
        mols = [_lonely(1), _star(1, 2), synth.make_dataset(3, seed=9)[0], _star(6, 3), _lonely(4), _star(33, 5),
                synth.make_dataset(3, seed=9)[1]]
    elif case == 'tiny_batch':
        mols = synth.make_dataset(6, seed=12, kind='qmugs')      # (two graphs: the head's BatchNorm over 2 rows is x_hat = +-1,
        #                                                          its gradient is rounding noise times 1/sqrt(var): not comparable)
    else:
        mols = [_star(k, 20 + k) for k in (1, 2, 3, 5, 7, 8, 9, 12, 17)] + synth.make_dataset(4, seed=13)
    kw2 = dict(PNA_SMALL, aggregators=['mean', 'sum', 'std', 'var'], readout_aggregators=['mean', 'sum'])   # smooth: no arg-max routing
    kw3 = dict(NET3D_SMALL, readout_aggregators=['mean', 'sum'])
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **kw2)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **kw3)
    _det_load(pna, 'pnaE')
    _det_load(net, 'net3dE')
    P2 = O.require_grad({k: v.clone() for k, v in pna.state_dict().items()})
    P3 = O.require_grad({k: v.clone() for k, v in net.state_dict().items()})
    og2, og3 = O.graphs_from_molecules(mols)
    r2, remb = O.pna_forward(og2, P2, O.pna_config(**kw2), True)
    r3, _ = O.net3d_forward(og3, P3, O.net3d_config(**kw3), True)
    pna.cuda().train(), net.cuda().train()
    g2, g3 = make_batch(amd, mols)
    z2, z3 = pna(g2), net(g3)
    assert rel_err(g2.ndata['feat'].cpu(), remb.detach()) < TOL
    assert rel_err(z2.cpu(), r2.detach()) < TOL and rel_err(z3.cpu(), r3.detach()) < TOL
    if len(mols) > 1:
        rloss = O.ntxent(r2, r3, 0.1)
        loss = amd.NTXent(tau=0.1)(z2, z3)
        assert abs(loss.item() - rloss.item()) < TOL * abs(rloss.item())
    else:                       # NT-Xent of a single pair has no negatives: compare through a plain quadratic loss
        rloss, loss = (r2 * r2).sum() + (r3 * r3).sum(), (z2 * z2).sum() + (z3 * z3).sum()
    rloss.backward()
    loss.backward()
    gtol = 1e-3
    grads_close(param_grads(pna), {k: P2[k].grad for k in O.trainable(P2)}, gtol, 'pna ')
    grads_close(param_grads(net), {k: P3[k].grad for k in O.trainable(P3)}, gtol, 'net3d ')


SMOOTH = dict(aggregators=['mean', 'sum', 'std', 'var'], readout_aggregators=['mean', 'sum'])
ROUTED_TOL = 3e-3       # max-norm bound on parameter gradients when the oracle's max / min gradients follow the HIP routing


def routed_tol(depth):
    """What is left after the routing are the ReLU gates: an activation within fp32 rounding of 0 is cut on one side and
    passed on the other, one whole gradient element either way - measured 1e-3 relative at depth <= 4 and up to 1.6e-2 on
    single weights at depth 7 (every layer adds its gates); still max-norm, where the un-routed bound was 5e-2 relative L2."""
    return ROUTED_TOL if depth <= 4 else 2e-2


@pytest.mark.parametrize('variant,n_mols,hidden,depth', [('as_configured', 10, 64, 2), ('smooth', 10, 64, 2), ('as_configured', 64, 64, 2),
                                                         ('smooth', 64, 64, 2), ('as_configured', 32, 200, 7)])
def test_qmugs_conformers_multiple_positives_vs_oracle(amd, variant, n_mols, hidden, depth):
    _qmugs_vs_oracle(amd, variant, n_mols, 'fp32', hidden=hidden, depth=depth)


@pytest.mark.parametrize('variant,n_mols,hidden,depth', [('smooth', 64, 64, 2), ('as_configured', 64, 64, 2),
                                                         ('as_configured', 32, 200, 7)])
def test_qmugs_conformers_bf16_matmul_vs_oracle(amd, variant, n_mols, hidden, depth, monkeypatch):
    """configs[3] shape with the bf16 matmul precision (bf16-rounded operands on the bf16 matrix pipe, fp32 accumulation,
    fp32 tensors / BatchNorm statistics) against the fp32 CPU oracle, molecules x 3 conformers: loss within 5e-3 relative,
    embeddings within 3e-2 of their scale, every parameter gradient within 0.15 relative L2 + 2e-3 of the largest gradient
    norm for the analytically-zero ones (the stated bf16 tolerance; the fp32 path holds 1e-4 / 2e-3 on the same case).
    as_configured: max / min aggregators and readouts as in the yml - the oracle's max / min gradients follow the positions
    the HIP kernels picked (bf16 rounding moves many more near-ties than fp32 rounding does; which atom wins one is not what
    this test is about); also at the yml's hidden 200 / depth 7, where seven layers of rounded products add up: measured and
    stated bounds in _qmugs_vs_oracle."""
    ops = importlib.import_module('3dinfomax_amd.ops')
    # the bf16 STORAGE form of the 3D network's edge stage at these (small) sizes too: it switches on by size
    monkeypatch.setattr(importlib.import_module('3dinfomax_amd.net3d_native'), 'BF16_STORE_MIN_EDGES', 0)
    monkeypatch.setenv('I3D_MSG_BF16', 'force')      # and of the 2D network's messages (csrc/model.hip: msg_bf16_storage)
    prev = ops.set_matmul_precision('bf16')
    try:
        _qmugs_vs_oracle(amd, variant, n_mols, 'bf16', hidden=hidden, depth=depth)
    finally:
        ops.set_matmul_precision(prev)


# relative L2 bounds (2D network, 3D network) of the end-to-end bf16 check at 256 molecules x 3 conformers
E2E_BF16_TOL = {'smooth': (0.13, 0.1), 'as_configured': (0.1, 0.1)}      # measured: smooth <= 0.115 (sum / var aggregators), as configured <= 0.096


@pytest.mark.parametrize('variant', ['smooth', 'as_configured'])
def test_qmugs_conformers_bf16_matmul_end_to_end_at_256_molecules(amd, variant, monkeypatch):
    """The bf16 matmul mode END TO END: configs[3] shape at 256 molecules x 3 conformers - where
    the projection head's BatchNorm backward is well-conditioned, unlike the 32-row case of the test above - with the
    loss's own gradient flowing into both networks: every parameter gradient within 0.1 relative L2 of the fp32 CPU oracle
    (2e-3 of the largest gradient norm as the floor for the analytically-zero ones), loss 5e-3, embeddings 3e-2.  The size
    gates of the bf16 storage forms are forced on as in the test above."""
    ops = importlib.import_module('3dinfomax_amd.ops')
    monkeypatch.setattr(importlib.import_module('3dinfomax_amd.net3d_native'), 'BF16_STORE_MIN_EDGES', 0)
    monkeypatch.setenv('I3D_MSG_BF16', 'force')
    prev = ops.set_matmul_precision('bf16')
    try:
        _qmugs_vs_oracle(amd, variant, 256, 'bf16_e2e', hidden=64, depth=2)
    finally:
        ops.set_matmul_precision(prev)


def _qmugs_vs_oracle(amd, variant, n_mols, precision, hidden=64, depth=2):
    """Gradient check at scale, two variants: `as_configured` keeps the max/min aggregators and readouts - fp32
    rounding may flip the arg-max of a near-tie between two atoms, so the gradients are held to a relative L2 bound;
    `smooth` swaps them for mean/sum/std/var (no arg-max anywhere) and holds every gradient to the strict max-norm
    bound.  The arg-max routing itself is pinned by the reference fixtures and the kernel tests.

    BASELINE config 4 shape (pre-train_QMugs.yml): QMugs-shaped molecules (degrees <= 6, up to ~100 atoms here),
    3 conformers per molecule batched with conformer_collate, NTXentMultiplePositives - fp32 parity vs the oracle."""
    rng = np.random.default_rng(3)
    mols = [m for m in synth.make_dataset(4 * n_mols, seed=11, kind='qmugs') if m.n_atoms <= 100][:n_mols]
    assert len(mols) == n_mols
    confs = [synth.conformers(m, rng, 3) for m in mols]
    items = [(amd.bond_graph(m), amd.batch([amd.complete_graph(m, c) for c in cs])) for m, cs in zip(mols, confs)]
    (g2,), (g3,) = amd.conformer_collate(items)
    assert g3.batch_num_nodes().shape[0] == 3 * len(mols)
    kw2 = dict(PNA_YML, propagation_depth=depth, hidden_dim=hidden, readout_hidden_dim=hidden, target_dim=48)
    kw3 = dict(NET3D_YML, target_dim=48)
    if variant == 'smooth':
        kw2.update(SMOOTH)
        kw3.update(readout_aggregators=['mean', 'sum'])
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **kw2)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **kw3)
    _det_load(pna, 'pnaQ')
    _det_load(net, 'net3dQ')
    P2 = O.require_grad({k: v.clone() for k, v in pna.state_dict().items()})
    P3 = O.require_grad({k: v.clone() for k, v in net.state_dict().items()})
    og2, _ = O.graphs_from_molecules(mols)
    # oracle 3D graph: conformers of a molecule are consecutive graphs (molecule-major, conformer-minor)
    flat_mols = [m for m in mols for _ in range(3)]
    flat_xyz = [c for cs in confs for c in cs]
    _, og3 = O.graphs_from_molecules(flat_mols, flat_xyz)
    pna.cuda().train(), net.cuda().train()
    g2d = g2.to('cuda:0')
    z2, z3 = pna(g2d), net(g3.to('cuda:0'))
    # as_configured: the oracle routes its max / min gradients (2D model: aggregators and readout) to the positions the HIP
    # kernels picked - near-ties that fp32 rounding resolves differently no longer move whole gradient rows, so the 2D
    # gradients are held to the strict max-norm bound of the smooth variant; the flips are counted and must be rare
    routed = variant == 'as_configured'
    route = hip_routing(pna, g2d, z2) if routed else None
    cap = {} if routed else None
    r2, _ = O.pna_forward(og2, P2, O.pna_config(**kw2), True, capture=cap, route=route)
    r3, _ = O.net3d_forward(og3, P3, O.net3d_config(**kw3), True)
    rloss = O.ntxent_multiple_positives(r2, r3, 0.1)
    if precision == 'bf16_e2e':
        # END TO END at a batch where the head's BatchNorm backward is well-conditioned (>= 256 molecules): the loss's OWN
        # gradient as the upstream of both networks, every parameter gradient against the fp32 oracle in relative L2
        rloss.backward()
        loss = amd.NTXentMultiplePositives(tau=0.1)(z2, z3)
        loss.backward()
        assert abs(loss.item() - rloss.item()) < 5e-3 * abs(rloss.item())
        assert rel_err(z2.cpu(), r2.detach()) < 3e-2 and rel_err(z3.cpu(), r3.detach()) < 3e-2
        grads_close_l2(param_grads(pna), {k: P2[k].grad for k in O.trainable(P2)}, E2E_BF16_TOL[variant][0], 'pna ', floor=2e-3)
        grads_close_l2(param_grads(net), {k: P3[k].grad for k in O.trainable(P3)}, E2E_BF16_TOL[variant][1], 'net3d ', floor=2e-3)
        return
    if precision == 'bf16':      # (b) below: a fixed, well-conditioned upstream gradient instead of the loss's
        gen = torch.Generator().manual_seed(17)
        u2, u3 = torch.randn(r2.shape, generator=gen) * 0.01, torch.randn(r3.shape, generator=gen) * 0.01
        torch.autograd.backward([r2, r3], [u2.to(r2), u3.to(r3)])
    else:
        rloss.backward()
    assert z3.shape[0] == 3 * z2.shape[0]
    if precision == 'bf16':
        # Two well-conditioned halves instead of one ill-conditioned whole.  With the loss's own gradient as the upstream of the
        # networks, EVERY parameter gradient of the depth-7 / 32-molecule case is 62 % off in relative L2 - one factor, the same
        # on every tensor from the head down: at tau = 0.1 and 32 rows the part of dL/dz that survives the head's BatchNorm
        # backward (dy - mean(dy) - xhat mean(dy xhat)) is a small difference of large terms, and 1e-2 of bf16 noise on xhat
        # is most of it; the linear backward pass carries that factor down.  (The same HIP kernels against their own fp32
        # run with a random upstream: 14-25 % median.)  So: (a) the loss and its gradient at the embeddings
        # the HIP models produced against the oracle's loss AT THOSE embeddings; (b) the networks' backward pass from a fixed
        # random upstream gradient, the same on both sides: every parameter gradient against the oracle's.
        z2h, z3h = z2.detach().requires_grad_(True), z3.detach().requires_grad_(True)
        loss = amd.NTXentMultiplePositives(tau=0.1)(z2h, z3h)
        loss.backward()
        o2, o3 = z2.detach().cpu().requires_grad_(True), z3.detach().cpu().requires_grad_(True)
        oloss = O.ntxent_multiple_positives(o2, o3, 0.1)
        oloss.backward()
        # (the similarity GEMM and the two gradient GEMMs of the loss round their operands too: 2^-9 on a similarity, / tau)
        if os.environ.get('I3D_TEST_VERBOSE'):
            print(f'bf16 loss at the same embeddings: {abs(loss.item() - oloss.item()) / abs(oloss.item()):.2e}, dz '
                  f'{rel_err(z2h.grad.cpu(), o2.grad):.2e} {rel_err(z3h.grad.cpu(), o3.grad):.2e}')
        assert abs(loss.item() - oloss.item()) < 5e-4 * abs(oloss.item())
        assert rel_err(z2h.grad.cpu(), o2.grad) < 5e-2 and rel_err(z3h.grad.cpu(), o3.grad) < 5e-2
        deep = depth > 4
        assert abs(loss.item() - rloss.item()) < 5e-3 * abs(rloss.item())
        assert rel_err(z2.cpu(), r2.detach()) < 3e-2 and rel_err(z3.cpu(), r3.detach()) < 3e-2
        torch.autograd.backward([z2, z3], [u2.to(z2), u3.to(z3)])
        # measured relative L2 per tensor: smooth <= 0.07; as_configured median 0.14 at both sizes, the first head block (fed
        # by the max / min readouts) 0.26-0.37 (weight) / 0.31-0.50 (bias), posttrans BatchNorm biases up to 0.33
        grads_close_l2(param_grads(pna), {k: P2[k].grad for k in O.trainable(P2)}, 0.15 if variant == 'smooth' else 0.6, 'pna ', floor=2e-3)
        # the 3D network with its edge-stage activations STORED as bf16 (net3d_native.BF16_STORE; x_msg about a centre:
        # csrc/net3d_edge.hip n3_center_kernel): measured 0.04-0.18 per tensor (raw, un-centred storage: 0.14-0.96 on the
        # 32-molecule case - the BatchNorm behind a nearly constant column divides the rounding error by its tiny deviation)
        grads_close_l2(param_grads(net), {k: P3[k].grad for k in O.trainable(P3)}, 0.25, 'net3d ', floor=2e-3)
        return
    loss = amd.NTXentMultiplePositives(tau=0.1)(z2, z3)
    loss.backward()
    assert abs(loss.item() - rloss.item()) < TOL * abs(rloss.item())
    assert rel_err(z2.cpu(), r2.detach()) < TOL and rel_err(z3.cpu(), r3.detach()) < TOL
    if routed:      # forward against the oracle's OWN extrema as well (no routing): outputs, node embeddings and loss to 1e-4
        with torch.no_grad():
            u2, uemb = O.pna_forward(og2, {k: v.detach() for k, v in P2.items()}, O.pna_config(**kw2), True)
            uloss = O.ntxent_multiple_positives(u2, r3.detach(), 0.1)
        assert abs(loss.item() - uloss.item()) < TOL * abs(uloss.item())
        assert rel_err(z2.detach().cpu(), u2) < TOL and rel_err(g2d.ndata['feat'].cpu(), uemb) < TOL
    if variant == 'smooth':    # 2e-3: the weight gradients reduce over ~10^3-10^4 rows in fp32 (split-K) on both sides
        grads_close(param_grads(pna), {k: P2[k].grad for k in O.trainable(P2)}, 2e-3, 'pna ')
        grads_close(param_grads(net), {k: P3[k].grad for k in O.trainable(P3)}, 2e-3, 'net3d ')
    else:
        flips, total = routing_flips(route, cap, kw2['propagation_depth'])
        assert flips <= 2e-3 * total, (flips, total)
        # 3e-3 max-norm (smooth variant: 2e-3; the std aggregator's relu gate at var ~ 0 still sits on each side's own
        # rounding) - it was 5e-2 relative L2 before the routing
        grads_close(param_grads(pna), {k: P2[k].grad for k in O.trainable(P2)}, routed_tol(depth), 'pna ',
                    gate_floor=0.0 if depth <= 4 else 1e-2)
        # the 3D network's own min / max readout is not routed (its three nodes-per-feature candidates are far apart on
        # these molecules; no flip has been seen): relative L2 as before
        grads_close_l2(param_grads(net), {k: P3[k].grad for k in O.trainable(P3)}, 5e-2, 'net3d ')


# un-routed gradient bound (relative L2 per tensor of the 2D model; measured values in DESIGN.md section 6)
# measured: depth 4 worst 2.0e-4 / median 9.6e-5 at 256 molecules; depth 7 / 128 molecules worst 1.7e-2 (a bias) / median 2.5e-3.
# An arg-max near-tie that the two sides resolve differently moves a whole row: the bounds leave room for a few of those.
# Bounds = 2 x the measured worst (round 5: 2.6e-3 at 512 molecules / depth 4, 1.7e-2 at depth 7 / 128 molecules).
UNROUTED_L2 = {4: 5.2e-3, 7: 3.5e-2}


@pytest.mark.parametrize('batch,depth', [(512, 4), (256, 4), (128, 7)])
def test_pretraining_config_hidden_200_vs_oracle_with_routed_extrema(amd, batch, depth):
    """BASELINE.json configs[1] at hidden 200 / depth 4 AT ITS OWN SIZE (512 molecules; also 256, and the yml's depth 7 on
    128) against the CPU oracle, trained-like weights (_det_load), aggregators and readouts AS CONFIGURED (mean / max / min /
    std, min / max / mean): loss, node embeddings and outputs to 1e-4, every parameter gradient of the 2D model to 2e-3
    max-norm with the oracle's max / min gradients routed to the positions the HIP kernels picked; flips (near-ties resolved
    differently by fp32 rounding) are counted.  Next to it the UN-routed statement: the same gradients against the oracle
    with its own arg-max / arg-min choices, relative L2 per tensor, printed and bounded (the routed comparison is a
    refinement of this one, not the only evidence)."""
    mols = synth.make_dataset(batch, seed=41)
    kw2 = dict(PNA_YML, propagation_depth=depth)
    kw3 = dict(NET3D_YML)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **kw2)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **kw3)
    _det_load(pna, 'pnaR')
    _det_load(net, 'net3dR')
    P2 = O.require_grad({k: v.clone() for k, v in pna.state_dict().items()})
    P3 = O.require_grad({k: v.clone() for k, v in net.state_dict().items()})
    og2, og3 = O.graphs_from_molecules(mols)
    pna.cuda().train(), net.cuda().train()
    g2, g3 = make_batch(amd, mols)
    z2, z3 = pna(g2), net(g3)
    route = hip_routing(pna, g2, z2)
    cap = {}
    r2, remb = O.pna_forward(og2, P2, O.pna_config(**kw2), True, capture=cap, route=route)
    r3, _ = O.net3d_forward(og3, P3, O.net3d_config(**kw3), True)
    rloss = O.ntxent(r2, r3, 0.1)
    rloss.backward()
    loss = amd.NTXent(tau=0.1)(z2, z3)
    loss.backward()
    assert abs(loss.item() - rloss.item()) < TOL * abs(rloss.item())
    assert rel_err(g2.ndata['feat'].cpu(), remb.detach()) < TOL
    assert rel_err(z2.cpu(), r2.detach()) < TOL and rel_err(z3.cpu(), r3.detach()) < TOL
    flips, total = routing_flips(route, cap, depth)
    assert flips <= 2e-3 * total, (flips, total)
    ref2 = {k: P2[k].grad for k in O.trainable(P2)}
    # depth 7: which side of 0 an activation lands on moves with the GEMM's summation order (the tile configuration): one
    # flipped gate measured 9.5e-4 absolute = 4e-3 of the largest gradient on layer 5's first pretrans weight (max 1.4e-2,
    # the other tensors at 1.5e-4); max-norm with that much room, and the tensors as a whole to 1e-2 relative L2
    # 512 molecules: twice the rows of the 256 case, twice the ReLU gates within rounding of 0 - one cut on one side and passed
    # on the other measured 5.4e-5 absolute = 6e-4 of the largest gradient on layer 1's first pretrans weight (bound without
    # room for a gate: 3.7e-5); every other tensor sits below a third of its bound
    grads_close(param_grads(pna), ref2, routed_tol(depth), 'pna ',
                gate_floor=(1e-3 if batch >= 512 else 0.0) if depth <= 4 else 1e-2)
    if depth > 4:
        grads_close_l2(param_grads(pna), ref2, 1e-2, 'pna ', floor=5e-5)      # floor: the biases in front of a BatchNorm (noise)
    grads_close_l2(param_grads(net), {k: P3[k].grad for k in O.trainable(P3)}, 5e-2, 'net3d ')
    # ---- un-routed: the oracle alone decides where its max / min gradients go (reference semantics: first index of the
    # extremum of ITS fp32 values).  A near-tie that the two sides' roundings resolve differently moves one gradient row.
    U2 = O.require_grad({k: v.detach().clone() for k, v in P2.items()})
    U3 = O.require_grad({k: v.detach().clone() for k, v in P3.items()})
    u2, uemb = O.pna_forward(og2, U2, O.pna_config(**kw2), True)
    u3, _ = O.net3d_forward(og3, U3, O.net3d_config(**kw3), True)
    uloss = O.ntxent(u2, u3, 0.1)
    uloss.backward()
    # the FORWARD statement against the oracle's own extrema (no routing involved: a HIP kernel that picked a wrong - not
    # near-tied - neighbour would move these): loss, node embeddings (`ndata['feat']`) and outputs to north_star's 1e-4
    assert abs(loss.item() - uloss.item()) < TOL * abs(uloss.item())
    assert rel_err(g2.ndata['feat'].cpu(), uemb.detach()) < TOL
    assert rel_err(z2.cpu(), u2.detach()) < TOL and rel_err(z3.cpu(), u3.detach()) < TOL
    mine = param_grads(pna)
    worst, rows = 0.0, []
    for k in O.trainable(U2):
        if k not in mine or U2[k].grad is None:
            continue
        ref, got = U2[k].grad, mine[k].cpu()
        if ref.norm().item() < 5e-5:          # biases in front of a BatchNorm: analytically zero, noise on both sides
            continue
        e = ((got - ref).norm() / ref.norm()).item()
        rows.append((e, k))
        worst = max(worst, e)
    rows.sort(reverse=True)
    print(f'un-routed 2D gradients vs the oracle (batch {batch}, depth {depth}): worst relative L2 {worst:.2e} ({rows[0][1]}), '
          f'median {rows[len(rows) // 2][0]:.2e}')
    assert worst < UNROUTED_L2[depth], rows[:5]


@pytest.mark.parametrize('variant,depth', [('as_configured', 3), ('smooth', 3), ('as_configured', 7)])
def test_finetune_config_pna_only_l1_vs_oracle(amd, variant, depth):
    """BASELINE config 5 (tune_QM9_homo.yml): PNA only, readout min/max/mean/SUM, target_dim 1, BN momentum 0.1,
    L1 loss (reference trainer/trainer.py:111-114) - forward/backward parity vs the oracle, batch 128."""
    mols = synth.make_dataset(128, seed=77)
    kw = dict(PNA_YML, propagation_depth=depth, target_dim=1, batch_norm_momentum=0.1,
              readout_aggregators=['min', 'max', 'mean', 'sum'])
    if variant == 'smooth':
        kw.update(SMOOTH)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **kw)
    _det_load(pna, 'pnaF')
    P = O.require_grad({k: v.clone() for k, v in pna.state_dict().items()})
    og2, _ = O.graphs_from_molecules(mols)
    target = torch.from_numpy(det_fill((128, 1), 'homo_targets', 2.0))
    pna.cuda().train()
    g2, _ = make_batch(amd, mols)
    pred = pna(g2)
    routed = variant == 'as_configured'
    route = hip_routing(pna, g2, pred) if routed else None      # (see test_pretraining_config_hidden_200_...)
    cap = {} if routed else None
    rp, _ = O.pna_forward(og2, P, O.pna_config(**kw), True, capture=cap, route=route)
    rloss = torch.nn.functional.l1_loss(rp, target)
    rloss.backward()
    loss = torch.nn.L1Loss()(pred, target.cuda())
    loss.backward()
    assert abs(loss.item() - rloss.item()) < TOL * abs(rloss.item())
    assert rel_err(pred.cpu(), rp.detach()) < TOL
    if routed:
        flips, total = routing_flips(route, cap, depth)
        assert flips <= 2e-3 * total, (flips, total)
        # forward against the oracle's OWN extrema as well (no routing): prediction, node embeddings and loss to 1e-4
        with torch.no_grad():
            up, uemb = O.pna_forward(og2, {k: v.detach() for k, v in P.items()}, O.pna_config(**kw), True)
            uloss = torch.nn.functional.l1_loss(up, target)
        assert abs(loss.item() - uloss.item()) < TOL * abs(uloss.item())
        assert rel_err(pred.detach().cpu(), up) < TOL and rel_err(g2.ndata['feat'].cpu(), uemb) < TOL
    grads_close(param_grads(pna), {k: P[k].grad for k in O.trainable(P)}, routed_tol(depth) if routed else 2e-3, 'pna ')


@pytest.mark.parametrize('side_stream', [True, False])
def test_training_step_is_bit_deterministic(amd, side_stream, monkeypatch):
    monkeypatch.setattr(importlib.import_module('3dinfomax_amd.streams'), 'NET3D_STREAM', side_stream)
    _training_step_is_bit_deterministic(amd)


@pytest.mark.parametrize('async_backward', [False])      # (the helper-thread backward is gone; the case keeps its id)
def test_net3d_side_stream_equals_single_stream(amd, monkeypatch, async_backward):
    """Net3D next to PNA on a side stream (streams.py) gives the same bits as the single-stream schedule, over several
    optimisation steps (parameter updates, BN buffers and the side effects on the graph included)."""
    streams = importlib.import_module('3dinfomax_amd.streams')
    mols = synth.make_dataset(128, seed=33)
    res = {}
    for mode in (True, False):
        monkeypatch.setattr(streams, 'NET3D_STREAM', mode)
        torch.manual_seed(3)
        pna = amd.PNA(avg_d=1.0, device='cuda:0', **dict(PNA_YML, propagation_depth=3)).cuda().train()
        net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_YML).cuda().train()
        loss_fn = amd.NTXent(tau=0.1)
        params = list(pna.parameters()) + list(net.parameters())
        optim = amd.Adam(params, lr=1e-3)
        g2, g3 = make_batch(amd, mols)
        for _ in range(6):
            a, b = g2.local_copy(), g3.local_copy()
            loss = loss_fn(pna(a), net(b))
            loss.backward()
            optim.step()
            optim.zero_grad()
        torch.cuda.synchronize()
        res[mode] = ([p.detach().clone() for p in params] + [bf.detach().clone().float() for bf in net.buffers()]
                     + [b.ndata['feat'].detach().clone(), b.edata['d'].detach().clone()], loss.item())
    assert res[True][1] == res[False][1]
    for x, y in zip(res[True][0], res[False][0]):
        assert torch.equal(x, y)


def _training_step_is_bit_deterministic(amd):
    """Two runs of three optimisation steps from the same initial state end in bit-identical parameters: every
    reduction on the path has a fixed summation order (segmented sums, two-stage column reductions, split-K slices
    through the scratch, embedding-table gradients as a multi-hot GEMM) - no atomics."""
    mols = synth.make_dataset(96, seed=21)

    def run():
        torch.manual_seed(7)
        pna = amd.PNA(avg_d=1.0, device='cuda:0', **dict(PNA_YML, propagation_depth=2)).cuda().train()
        net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_YML).cuda().train()
        loss_fn = amd.NTXent(tau=0.1)
        params = list(pna.parameters()) + list(net.parameters())
        optim = amd.Adam(params, lr=1e-3)
        for _ in range(3):
            g2, g3 = make_batch(amd, mols)
            loss = loss_fn(pna(g2), net(g3))
            loss.backward()
            optim.step()
            optim.zero_grad()
        return loss.item(), [p.detach().clone() for p in params]

    l1, p1 = run()
    l2, p2 = run()
    assert l1 == l2
    for a, b in zip(p1, p2):
        assert torch.equal(a, b)


@pytest.mark.parametrize('second_group_wd', [1e-3, 0])
@pytest.mark.parametrize('native', [False, True])
def test_adam_fast_path_is_torch_adam(amd, second_group_wd, native, monkeypatch):
    """infomax3d_amd.Adam against torch.optim.Adam(fused=True) over several steps, a changing lr, and a state_dict round
    trip; with two groups of different and of identical hyper-parameters.  native=False: cached tensor lists in front of
    torch._fused_adam_ - bit-identical parameters and state.  native=True: the one-launch kernel of csrc/adam.hip (groups
    with identical hyper-parameters; torch's kernel otherwise) - the same expressions, held to the last bits of fp32
    (torch's kernel is compiled with floating-point contraction, ours without: single elements differ by one ulp)."""
    monkeypatch.setattr(importlib.import_module('3dinfomax_amd.optim'), 'NATIVE_ADAM', native)

    def same(a, b):
        if not native:
            return torch.equal(a, b)
        return (a - b).abs().max().item() <= 4e-7 * max(b.abs().max().item(), 1e-30)
    torch.manual_seed(0)
    shapes = [(200, 600), (200,), (7, 3), (1,), (64, 64)]
    pa = [torch.randn(s, device='cuda:0').requires_grad_() for s in shapes]
    pb = [p.detach().clone().requires_grad_() for p in pa]

    def groups(ps):
        return [{'params': ps[:2], 'weight_decay': 0}, {'params': ps[2:], 'weight_decay': second_group_wd}]
    oa, ob = amd.Adam(groups(pa), lr=8e-5, fused=True), torch.optim.Adam(groups(pb), lr=8e-5, fused=True)
    for it in range(6):
        if it == 3:
            for o in (oa, ob):
                for gr in o.param_groups:
                    gr['lr'] = 3e-4
            ob2 = torch.optim.Adam(groups(pb), lr=1.0, fused=True)      # state_dict written by amd.Adam loads into torch's
            ob2.load_state_dict(copy.deepcopy(oa.state_dict()))
            oa.load_state_dict(copy.deepcopy(ob.state_dict()))   # (torch shares the tensors of a state_dict it loads)
        gs = [torch.randn(s, device='cuda:0') for s in shapes]
        for p, q, g_ in zip(pa, pb, gs):
            p.grad, q.grad = g_.clone(), g_.clone()
        oa.step()
        ob.step()
        oa.zero_grad()
        ob.zero_grad()
        for p, q in zip(pa, pb):
            assert same(p, q), it
    for p, q in zip(pa, pb):
        assert same(oa.state[p]['exp_avg_sq'], ob.state[q]['exp_avg_sq'])
        assert same(oa.state[p]['exp_avg'], ob.state[q]['exp_avg'])
        assert float(oa.state[p]['step']) == float(ob.state[q]['step']) == 6
    pa[0].grad = None                       # a parameter without gradient: falls back to torch's step
    for p in pa[1:]:
        p.grad = torch.ones_like(p)
    oa.step()


def test_native_adam_skips_parameters_that_never_get_a_gradient(amd):
    """Parameters the forward never uses (the reference builds some: PNAGNNOriginal.MLP_layer, models/pna_original.py:179) have no
    gradient and no optimizer state - torch.optim.Adam skips them.  They must not keep the one-launch kernel off: same values
    as torch over several steps with the native path taken, and a late first gradient for such a parameter is honoured."""
    torch.manual_seed(2)
    shapes = [(64, 40), (40,), (9, 5), (12,)]
    pa = [torch.randn(s, device='cuda:0').requires_grad_() for s in shapes]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    oa, ob = amd.Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3, fused=True)

    def step(with_last):
        gs = [torch.randn(s, device='cuda:0') for s in shapes]
        for i, (p, q, g_) in enumerate(zip(pa, pb, gs)):
            none = (not with_last) and i == len(shapes) - 1
            p.grad, q.grad = (None, None) if none else (g_.clone(), g_.clone())
        oa.step()
        ob.step()

    def close():
        return all((p - q).abs().max().item() <= 4e-7 * max(q.abs().max().item(), 1e-30) for p, q in zip(pa, pb))
    for _ in range(4):
        step(False)
    assert close() and oa._native is not None and oa._host_step == 4 and len(oa._gradless) == 1
    assert torch.equal(pa[-1], pb[-1]) and pa[-1] not in oa.state or len(oa.state[pa[-1]]) == 0
    for _ in range(3):
        step(True)                  # the parameter gets its first gradient: torch creates its state, step counts differ
    assert close()
    assert [float(oa.state[p]['step']) for p in pa] == [7.0, 7.0, 7.0, 3.0] == [float(ob.state[q]['step']) for q in pb]


def test_native_adam_with_unequal_step_counts_a_moved_parameter_and_an_lr_schedule(amd):
    """The one-launch Adam takes ONE step count for its bias corrections: parameters whose `step` differs (a parameter
    that had no gradient for some steps, add_param_group on a trained optimizer, unfreezing) must get torch's
    per-parameter arithmetic; a parameter whose storage was swapped (`p.data = ...`) must not be updated through the old
    pointers; a learning-rate schedule must not switch the steady-state fast path off."""
    optim_mod = importlib.import_module('3dinfomax_amd.optim')
    torch.manual_seed(1)
    shapes = [(64, 40), (40,), (9, 5)]
    pa = [torch.randn(s, device='cuda:0').requires_grad_() for s in shapes]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    oa, ob = amd.Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3, fused=True)

    def step(skip_last=False, lr=None):
        gs = [torch.randn(s, device='cuda:0') for s in shapes]
        for o in (oa, ob):
            if lr is not None:
                for gr in o.param_groups:
                    gr['lr'] = lr
        for i, (p, q, g_) in enumerate(zip(pa, pb, gs)):
            none = skip_last and i == len(shapes) - 1
            p.grad, q.grad = (None, None) if none else (g_.clone(), g_.clone())
        oa.step()
        ob.step()

    def close():
        return all((p - q).abs().max().item() <= 4e-7 * max(q.abs().max().item(), 1e-30) for p, q in zip(pa, pb))
    for _ in range(3):
        step()
    assert close() and oa._native is not None and oa._host_step == 3
    for _ in range(2):
        step(skip_last=True)                 # torch skips the parameter: its step counter lags behind now
    for _ in range(3):
        step()
    assert [float(oa.state[p]['step']) for p in pa] == [8.0, 8.0, 6.0] == [float(ob.state[q]['step']) for q in pb]
    assert close(), 'unequal step counts: the bias corrections must be per parameter'
    # an lr schedule: after one general step the fast path is back
    oa2, ob2 = oa, ob
    pa2 = [torch.randn(s, device='cuda:0').requires_grad_() for s in shapes]
    pb2 = [p.detach().clone().requires_grad_() for p in pa2]
    pa[:], pb[:] = pa2, pb2
    oa, ob = amd.Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3, fused=True)
    grads = [torch.randn(s, device='cuda:0') for s in shapes]

    def step_same_objects(lr):
        for o in (oa, ob):
            for gr in o.param_groups:
                gr['lr'] = lr
        for p, q, g_ in zip(pa, pb, grads):
            if p.grad is None:
                p.grad, q.grad = g_.clone(), g_.clone()
        oa.step()
        ob.step()
    for it in range(6):
        step_same_objects(1e-3 * (it + 1))
    assert close()
    assert oa._native_fast.__self__ is oa and oa._native.key[0] == 6e-3, 'hyper-parameter key follows the schedule'
    calls = []
    real = oa._step_general
    oa._step_general = lambda closure=None: (calls.append(1), real(closure))[1]
    step_same_objects(6e-3)
    assert calls == [], 'steady state goes straight to the launch'
    # swap a parameter's storage: the next step must see it
    pa[0].data = pa[0].data.clone()
    pb[0].data = pb[0].data.clone()
    step_same_objects(6e-3)
    assert calls == [1] and close()
    del oa2, ob2, optim_mod


def test_eval_and_no_grad_forward_through_the_native_sequencer(amd, monkeypatch):
    """The validation pass of the reference (trainer/trainer.py:72-78: model.eval() under no_grad) and inference.py's
    train-mode forward under no_grad run through the whole-model C sequencer: same output and node embeddings as the
    per-block path, eval mode leaves every BatchNorm buffer untouched, train mode under no_grad updates them."""
    native = importlib.import_module('3dinfomax_amd.pna_native')
    mols = synth.make_dataset(48, seed=33)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **dict(PNA_YML, propagation_depth=3)).cuda().train()
    _det_load(pna, 'pnaEval')
    calls = []
    real_run = native.run
    monkeypatch.setattr(native, 'run', lambda *a, **k: (calls.append(1), real_run(*a, **k))[1])
    sd0 = {k: v.clone() for k, v in pna.state_dict().items()}

    def fwd(native_on, train):
        pna.load_state_dict(sd0)
        pna.train(train)
        monkeypatch.setattr(native, 'NATIVE_MODEL', native_on)
        g2, _ = make_batch(amd, mols)
        with torch.no_grad():
            out = pna(g2)
        return out.clone(), g2.ndata['feat'].clone(), {k: v.clone() for k, v in pna.state_dict().items()}
    for train in (False, True):
        n0 = len(calls)
        a = fwd(True, train)
        assert len(calls) == n0 + 1, 'the native sequencer must take this call'
        b = fwd(False, train)
        assert len(calls) == n0 + 1
        assert rel_err(a[0].cpu(), b[0].cpu()) < 1e-5 and rel_err(a[1].cpu(), b[1].cpu()) < 1e-5
        for k in sd0:
            if 'running' in k or 'num_batches' in k:
                if train:
                    assert close(a[2][k].cpu(), b[2][k].cpu(), 1e-5, 1e-7), k
                    if 'num_batches' in k:
                        assert int(a[2][k]) == int(sd0[k]) + 1
                else:
                    assert torch.equal(a[2][k], sd0[k]), k
    # eval mode WITH autograd (gradients through frozen statistics) stays on the per-block path
    pna.eval()
    monkeypatch.setattr(native, 'NATIVE_MODEL', True)
    g2, _ = make_batch(amd, mols)
    n0 = len(calls)
    pna(g2).sum().backward()
    assert len(calls) == n0


def test_parameter_gradients_stored_by_the_model_node(amd, monkeypatch):
    """tape.ModelFn stores `.grad` itself when the parameters are plain leaves: same values as through autograd's
    AccumulateGrad nodes (I3D_DIRECT_PARAM_GRADS=0), gradient accumulation over two backward passes still sums, and a
    tensor hook on a parameter still fires (both fall back to autograd's own accumulation)."""
    tape = importlib.import_module('3dinfomax_amd.tape')
    mols = synth.make_dataset(24, seed=21)
    kw2 = dict(PNA_SMALL)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **kw2).cuda().train()
    _det_load(pna, 'pnaG')

    def grads(direct, passes=1, hook=None):
        monkeypatch.setattr(tape, 'DIRECT_PARAM_GRADS', direct)
        pna.zero_grad()
        handle = next(iter(pna.parameters())).register_hook(hook) if hook else None
        for _ in range(passes):
            g2, _ = make_batch(amd, mols)
            (pna(g2) ** 2).sum().backward()
        if handle is not None:
            handle.remove()
        return {k: p.grad.clone() for k, p in pna.named_parameters() if p.grad is not None}

    a, b = grads(True), grads(False)
    assert a.keys() == b.keys() and len(a) > 10
    for k in a:
        assert torch.equal(a[k], b[k]), k
    twice = grads(True, passes=2)
    for k in a:
        assert torch.allclose(twice[k], 2 * a[k], rtol=1e-5, atol=1e-6 * float(a[k].abs().max())), k
    seen = []
    hooked = grads(True, hook=lambda g: seen.append(g.shape))
    assert len(seen) == 1
    for k in a:
        assert torch.equal(hooked[k], a[k]), k


@pytest.mark.parametrize('composite', [True, False])
def test_num_batches_tracked_counts_forward_passes(amd, monkeypatch, composite):
    """BatchNorm1d.num_batches_tracked goes up by one per training forward (the statistics kernel bumps it on the composite
    paths, one multi-tensor add per model on the per-kernel path) and stays put in eval mode."""
    if not composite:       # (net3d_native holds the function under its own name; PNA's model C call does not ask it in eval mode)
        for mod, name in (('layers', '_composite_ok'), ('net3d_native', '_composite_ok'), ('pna_native', 'eligible')):
            monkeypatch.setattr(importlib.import_module('3dinfomax_amd.' + mod), name, lambda *a, **k: False)
    mols = synth.make_dataset(12, seed=3)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **PNA_SMALL).cuda().train()
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_SMALL).cuda().train()
    for _ in range(3):
        g2, g3 = make_batch(amd, mols)
        (pna(g2).sum() + net(g3).sum()).backward()
    pna.eval(), net.eval()
    with torch.no_grad():
        g2, g3 = make_batch(amd, mols)
        pna(g2), net(g3)
    torch.cuda.synchronize()
    counters = [(k, int(v)) for m in (pna, net) for k, v in m.state_dict().items() if k.endswith('num_batches_tracked')]
    assert len(counters) > 5 and all(v == 3 for _, v in counters), counters


def test_process_level_switches_give_the_same_bits(tmp_path):
    """Switches that are read once per process (-> subprocesses): the weight-gradient side stream of the backward
    composites off / with two forks, freshly allocated parameter gradients, the in-launch finalisation off - three
    optimisation steps end in the same bits as the default."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import importlib, sys, torch\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import helpers\n"
        "amd = importlib.import_module('3dinfomax_amd')\n"
        "mols = amd.synth.make_dataset(96, seed=21)\n"
        "torch.manual_seed(7)\n"
        "pna = amd.PNA(avg_d=1.0, device='cuda:0', **dict(helpers.PNA_YML, propagation_depth=2)).cuda().train()\n"
        "net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **helpers.NET3D_YML).cuda().train()\n"
        "loss_fn = amd.NTXent(tau=0.1)\n"
        "params = list(pna.parameters()) + list(net.parameters())\n"
        "optim = amd.Adam(params, lr=1e-3)\n"
        "for _ in range(3):\n"
        "    g2 = amd.batch([amd.bond_graph(m) for m in mols]).to('cuda:0')\n"
        "    g3 = amd.batch([amd.complete_graph(m) for m in mols]).to('cuda:0')\n"
        "    loss_fn(pna(g2), net(g3)).backward()\n"
        "    optim.step(); optim.zero_grad()\n"
        "torch.save([p.detach().cpu() for p in params], sys.argv[1])\n") % (root, os.path.join(root, 'tests'))
    res = {}
    variants = {'default': {}, 'no_wgrad_stream': {'I3D_WGRAD_STREAM': '0'},
                # the loss sequenced from Python runs the first version's kernels (two norm launches, row_axpy after the
                # GEMMs): the same bits as the C sequencer with I3D_LOSS_FUSED=0
                'python_sequenced_loss': {'I3D_LOSS_COMPOSITE': '0'}, 'unfused_loss': {'I3D_LOSS_FUSED': '0'},
                'torch_adam_kernel': None,
                'fresh_grads': {'I3D_PERSISTENT_GRADS': '0'},
                # round 6: the BatchNorm backward as one launch takes its row sums in another order than the two-pass kernels
                # (tests/test_gpu_ops.py: test_bn_bwd_one_launch_...): allclose against the default; the separate finalisation
                # launches (which imply the two-pass kernels) bit for bit against THAT
                'two_pass_bn_backward': {'I3D_BN_BWD_ONE_LAUNCH': '0'},
                'separate_final': {'I3D_FUSED_FINAL': '0', 'I3D_BN_BWD_ONE_LAUNCH': '0'},
                # the whole PNA pass from one C call per direction (csrc/model.hip) vs. sequenced layer by layer from Python
                'python_sequenced_model': {'I3D_NATIVE_MODEL': '0'},
                'python_sequenced_fresh_grads': {'I3D_NATIVE_MODEL': '0', 'I3D_PERSISTENT_GRADS': '0'},
                'autograd_param_grads': {'I3D_DIRECT_PARAM_GRADS': '0'}}
    variants = {k: v for k, v in variants.items() if v is not None}
    for name, env in variants.items():
        path = str(tmp_path / f'switch_{name}.pt')
        subprocess.run([sys.executable, '-c', code, path], check=True, env=dict(os.environ, **env), timeout=600)
        res[name] = torch.load(path)
    assert len(res['default']) > 50
    for name in variants:
        base = 'unfused_loss' if name == 'python_sequenced_loss' else ('two_pass_bn_backward' if name == 'separate_final' else 'default')
        if name in ('unfused_loss', 'two_pass_bn_backward'):
            # another summation order (against the oracle to 2e-5: test_gpu_ops.test_ntxent_fwd_bwd_vs_oracle; against fp64 and each
            # other: test_gpu_ops.test_bn_bwd_one_launch_against_the_two_pass_kernels); three Adam steps turn rounding-level
            # differences of near-zero gradients into +-lr steps, so the trajectories are not compared element by element
            continue
        for a, b in zip(res[base], res[name]):
            assert torch.equal(a, b), name


@pytest.mark.parametrize('cfg', ['yml', 'deep'])
def test_native_net3d_equals_block_path(amd, monkeypatch, cfg):
    """Net3D as one tape node sequenced over raw pointers (net3d_native.py) gives the same bits as the per-block path:
    output, side effects on the graph, every parameter gradient, BatchNorm buffers - and it is the path that runs."""
    native = importlib.import_module('3dinfomax_amd.net3d_native')
    kw = dict(NET3D_YML) if cfg == 'yml' else dict(NET3D_YML, propagation_depth=3, message_net_layers=2, update_net_layers=2,
                                                     node_wise_output_layers=2, readout_layers=2, reduce_func='sum')
    mols = synth.make_dataset(40, seed=17)
    calls = []
    real_forward = native.forward
    monkeypatch.setattr(native, 'forward', lambda *a, **k: (calls.append(1), real_forward(*a, **k))[1])
    res = {}
    monkeypatch.setattr(native, 'FUSED_EDGE', False)      # the fused edge stage is a different summation order: below
    for mode in (True, False):
        monkeypatch.setattr(native, 'NATIVE_NET3D', mode)
        res[mode] = _net3d_two_steps(amd, kw, mols)
    assert len(calls) == 2                      # the native path ran (both forward passes of the first model)
    assert len(res[True]) == len(res[False]) > 20
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        assert torch.equal(a, b), i


def _net3d_two_steps(amd, kw, mols):
    torch.manual_seed(11)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **kw).cuda().train()
    outs = []
    for _ in range(2):
        _, g3 = make_batch(amd, mols)
        z = net(g3)
        (z * torch.linspace(-1, 1, z.shape[1], device='cuda:0')).sum().backward()
        outs += [z.detach().clone(), g3.ndata['feat'].detach().clone(), g3.edata['d'].detach().clone()]
    outs += [p.grad.clone() for p in net.parameters()] + [b.clone().float() for b in net.buffers()]
    return outs


@pytest.mark.parametrize('cfg', ['yml', 'sum', 'raw_distance', 'large', 'hidden16'])
def test_fused_net3d_edge_stage_matches_block_path(amd, monkeypatch, cfg):
    """The edge stage of the 3D network in one lane per edge (csrc/net3d_edge.hip: Fourier features, edge-input block,
    message block, gate, reduce - and their backward with the weight gradients on the MFMA unit) against the per-block
    kernels: output, node / distance embeddings left on the graph, every parameter gradient, BatchNorm buffers.  Same
    arithmetic in a different summation order: outputs and embeddings within 1e-5 of the tensor's scale (the acceptance
    bound of the path is 1e-4); gradients (summed over two steps) within 3e-4 of the scale + 5e-5 - several are small
    differences of large sums (a bias in front of a BatchNorm), and against a float64 torch model both paths sit at the
    same distance (tools/probes/net3d_edge_vs_fp64.py)."""
    native = importlib.import_module('3dinfomax_amd.net3d_native')
    kw = {'yml': dict(NET3D_YML), 'sum': dict(NET3D_YML, reduce_func='sum'),
          'raw_distance': dict(NET3D_YML, fourier_encodings=0), 'large': dict(NET3D_YML),
          'hidden16': dict(NET3D_YML, hidden_dim=16, hidden_edge_dim=16, fourier_encodings=2)}[cfg]
    mols = synth.make_dataset(700 if cfg == 'large' else 40, seed=23)      # 'large': several edge chunks per block, ragged tail
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(native, 'FUSED_EDGE', fused)
        res[fused] = _net3d_two_steps(amd, kw, mols)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **kw).cuda().train()
    assert native.fused_edge_ok(net) is False and native.FUSED_EDGE is False
    monkeypatch.setattr(native, 'FUSED_EDGE', True)
    assert native.fused_edge_ok(net) is True                   # the structure is eligible: the fused stage is what ran above
    assert len(res[True]) == len(res[False]) > 20
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        assert a.shape == b.shape
        scale = b.abs().max().item() + 1e-12
        tol = 1e-5 * scale + 1e-7 if i < 6 else 3e-4 * scale + 5e-5
        assert (a - b).abs().max().item() <= tol, (i, (a - b).abs().max().item(), scale)


def test_dist_warm_up_runs(amd):
    """dist.warm_up: the throw-away steps a data-parallel rank runs before it creates its communicator"""
    importlib.import_module('3dinfomax_amd.dist').warm_up('cuda:0', steps=1)


def test_missing_library_fails_loudly(amd, monkeypatch):
    L = importlib.import_module('3dinfomax_amd._lib')
    monkeypatch.setattr(L, '_lib', None)
    monkeypatch.setattr(L, 'LIB_PATH', '/nonexistent/lib3dinfomax_hip.so')
    with pytest.raises(L.HipLibraryError):
        L.load()


# embeddings (max-norm) / loss / all gradients (relative L2) under a reordering of the batch, trained-like weights
FULL_SIZE_TOL = (2e-5, 1e-5, 5e-3)


def test_full_size_batch_properties(amd):
    """configs[1] at its full size (512 molecules, hidden 200, depth 4 + Net3D + NT-Xent), through properties that do not
    need the oracle at that size: (1) reordering the molecules of the batch reorders the rows of both embeddings and
    leaves the loss unchanged (BatchNorm statistics and NT-Xent are sums over the batch: only the summation order moves,
    1e-5); (2) two copies of one molecule get bit-identical rows (every kernel computes a row / node / edge from its own
    inputs and batch-wide statistics only, whatever tile it lands in); (3) the parameter gradients of the reordered batch
    agree (relative L2 2e-3: arg-max near-ties of the max / min aggregators may move single rows)."""
    mols = synth.make_dataset(511, seed=31)
    mols = mols + [mols[7]]                                   # molecule 7 twice: rows 7 and 511
    perm = np.random.default_rng(5).permutation(512)

    def step(order):
        torch.manual_seed(9)
        pna = amd.PNA(avg_d=1.0, device='cuda:0', **dict(PNA_YML, propagation_depth=4))
        net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_YML)
        # trained-like weights: with the reference init (gain 1 / in_dim) the pre-BatchNorm variance is far below eps and
        # the embeddings barely depend on the input - the properties would be checked on near-constant rows
        _det_load(pna, 'pnaR')
        _det_load(net, 'net3dR')
        pna.cuda().train(), net.cuda().train()
        g2, g3 = make_batch(amd, [mols[i] for i in order])
        z2, z3 = pna(g2), net(g3)
        loss = amd.NTXent(tau=0.1)(z2, z3)
        loss.backward()
        grads = torch.cat([p.grad.flatten() for p in list(pna.parameters()) + list(net.parameters())])
        return z2.detach(), z3.detach(), loss.item(), grads

    z2, z3, loss, grads = step(range(512))
    assert z2.shape == (512, 256) and z3.shape == (512, 256) and math.isfinite(loss)
    assert z2.std(0).mean().item() > 1e-2 and z3.std(0).mean().item() > 1e-2      # the rows DO depend on the molecule
    assert torch.equal(z2[7], z2[511]) and torch.equal(z3[7], z3[511])
    z2p, z3p, lossp, gradsp = step(perm)
    idx = torch.from_numpy(perm).cuda()
    errs = [((a - b).abs().max() / b.abs().max()).item() for a, b in ((z2[idx], z2p), (z3[idx], z3p))]
    gerr = ((grads - gradsp).norm() / grads.norm()).item()
    print(f'full-size properties (configs[1]): embeddings {errs}, loss {abs(loss - lossp) / abs(loss):.2e}, gradients {gerr:.2e}')
    assert max(errs) <= FULL_SIZE_TOL[0]
    assert abs(loss - lossp) <= FULL_SIZE_TOL[1] * abs(loss)
    assert gerr <= FULL_SIZE_TOL[2]


def _full_size_properties(amd, step, n, tol_z, tol_loss, tol_grad, dup=(7, None)):
    """shared body of the full-size property tests: `step(order)` -> (z2, z3 or None, conformers per molecule, loss, grads)"""
    last = n - 1
    perm = np.random.default_rng(5).permutation(n)
    z2, z3, conf, loss, grads = step(list(range(n)))
    assert z2.shape[0] == n and math.isfinite(loss) and bool(torch.isfinite(grads).all())
    assert torch.equal(z2[dup[0]], z2[last])                       # the duplicated molecule: bit-identical rows
    if z3 is not None:
        assert z3.shape[0] == n * conf
        assert torch.equal(z3[dup[0] * conf:(dup[0] + 1) * conf], z3[last * conf:(last + 1) * conf])
    z2p, z3p, _, lossp, gradsp = step(list(perm))
    idx = torch.from_numpy(perm).cuda()
    pairs = [(z2[idx], z2p)]
    if z3 is not None:
        idx3 = (idx[:, None] * conf + torch.arange(conf, device='cuda')[None, :]).flatten()
        pairs.append((z3[idx3], z3p))
    errs = [((a - b).abs().max() / b.abs().max()).item() for a, b in pairs]
    gerr = ((grads - gradsp).norm() / grads.norm()).item()
    print(f'full-size properties: embeddings {errs}, loss {abs(loss - lossp) / abs(loss):.2e}, gradients {gerr:.2e}')
    assert all(e <= tol_z for e in errs), errs
    assert abs(loss - lossp) <= tol_loss * abs(loss)
    assert gerr <= tol_grad, gerr


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_full_size_qmugs_batch_properties(amd, precision):
    """configs[3] at its FULL size (pre-train_QMugs.yml: 500 molecules x 3 conformers, un-filtered atom counts, hidden 200,
    depth 7, NTXentMultiplePositives; ~24 k atoms, ~3.9 M complete-graph edges), fp32 and the bf16 matmul mode with its size
    gates NATURALLY on (bf16 storage of the 3D edge stage from 2^20 edges, of the messages from 32 MB; split-K slice counts
    for K in the 100 k) - through the properties of test_full_size_batch_properties: the duplicated molecule gets
    bit-identical rows in both embeddings (all three conformers), reordering the molecules reorders the rows and leaves
    loss and gradients unchanged up to summation order (bf16: up to operands that round the other way, 2^-9 each)."""
    ops = importlib.import_module('3dinfomax_amd.ops')
    n = 500
    mols = synth.make_dataset(n - 1, seed=61, kind='qmugs')
    mols = mols + [mols[7]]
    rng = np.random.default_rng(62)
    confs = [synth.conformers(m, rng, 3) for m in mols[:-1]]
    confs.append(confs[7])

    def step(order):
        torch.manual_seed(9)
        pna = amd.PNA(avg_d=1.0, device='cuda:0', **dict(PNA_YML, propagation_depth=7))
        net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_YML)
        _det_load(pna, 'pnaQ7')          # trained-like weights (see test_full_size_batch_properties)
        _det_load(net, 'net3dQ7')
        pna.cuda().train(), net.cuda().train()
        g2 = amd.batch([amd.bond_graph(mols[i]) for i in order]).to('cuda:0')
        g3 = amd.batch([amd.complete_graph(mols[i], c) for i in order for c in confs[i]]).to('cuda:0')
        if precision == 'bf16':      # the gates are on by size, not forced
            assert g3.number_of_edges() >= importlib.import_module('3dinfomax_amd.net3d_native').BF16_STORE_MIN_EDGES
            assert g2.number_of_edges() * 200 * 4 >= 32 << 20
        z2, z3 = pna(g2), net(g3)
        loss = amd.NTXentMultiplePositives(tau=0.1)(z2, z3)
        loss.backward()
        grads = torch.cat([p.grad.flatten() for p in list(pna.parameters()) + list(net.parameters())])
        return z2.detach(), z3.detach(), 3, loss.item(), grads

    prev = ops.set_matmul_precision(precision)
    try:
        # measured with trained-like weights: fp32 embeddings 2.3e-6, loss 0, gradients 1.1e-3; bf16 1.7e-2 / 7.5e-6 / 0.23 -
        # in the bf16 mode a reordering moves every GEMM tile boundary, operands round the other way (2^-9 each) and the
        # depth-7 backward pass amplifies it: two runs of the mode are as far from each other as each is from the fp32
        # oracle (0.10-0.15 relative L2, test_qmugs_conformers_bf16_matmul_end_to_end_at_256_molecules); with the reference init the same
        # test read 3.7e-2 because the embeddings barely depended on the input
        tz, tl, tg = (1e-5, 1e-5, 5e-3) if precision == 'fp32' else (3e-2, 1e-3, 0.35)
        _full_size_properties(amd, step, n, tz, tl, tg)
    finally:
        ops.set_matmul_precision(prev)


def test_full_size_finetune_batch_properties(amd):
    """configs[4] at its FULL size (tune_QM9_homo.yml: PNA only, batch 1024, depth 7, readout min / max / mean / sum, L1 loss
    on one target): duplicate-molecule bit equality, batch-order equivariance of the predictions, loss and gradients."""
    n = 1024
    mols = synth.make_dataset(n - 1, seed=71)
    mols = mols + [mols[7]]
    targets = torch.randn(n, 1, generator=torch.Generator().manual_seed(72))
    targets[n - 1] = targets[7]
    kw = dict(PNA_YML, target_dim=1, batch_norm_momentum=0.1, propagation_depth=7, readout_aggregators=['min', 'max', 'mean', 'sum'])

    def step(order):
        torch.manual_seed(9)
        pna = amd.PNA(avg_d=1.0, device='cuda:0', **kw)
        _det_load(pna, 'pnaF7')          # trained-like weights (see test_full_size_batch_properties)
        pna.cuda().train()
        g2 = amd.batch([amd.bond_graph(mols[i]) for i in order]).to('cuda:0')
        z = pna(g2)
        loss = torch.nn.L1Loss()(z, targets[torch.as_tensor(order)].cuda())
        loss.backward()
        grads = torch.cat([p.grad.flatten() for p in pna.parameters()])
        return z.detach(), None, 1, loss.item(), grads

    # (the sign() of an L1 residual within rounding of 0 may flip with the summation order: one row's gradient either way)
    _full_size_properties(amd, step, n, 1e-5, 1e-5, 2e-3)      # measured 6e-7 / 0 / 1e-4


def test_pna_and_net3d_with_dropout(amd):
    """dropout > 0 (reference models/base_layers.py:84-85, 104-105: nn.Dropout between activation and BatchNorm in every FCLayer of
    the MLPs; no BASELINE config sets it) takes the per-kernel path: the models train (finite loss, every parameter gets a
    gradient), two runs from the same seed are bit-identical, and in eval mode the outputs equal the dropout-free models'."""
    mols = synth.make_dataset(48, seed=13)
    kw2 = dict(PNA_YML, propagation_depth=2, hidden_dim=40, readout_hidden_dim=40, target_dim=16)
    kw3 = dict(NET3D_YML, target_dim=16)

    def build(p):
        torch.manual_seed(4)
        pna = amd.PNA(avg_d=1.0, device='cuda:0', **dict(kw2, dropout=p)).cuda().train()
        net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **dict(kw3, dropout=p)).cuda().train()
        return pna, net

    def run():
        pna, net = build(0.2)
        g2, g3 = make_batch(amd, mols)
        torch.manual_seed(11)
        loss = amd.NTXent(tau=0.1)(pna(g2), net(g3))
        loss.backward()
        return loss.item(), [p.grad.clone() for p in list(pna.parameters()) + list(net.parameters())], pna, net
    l1, g1, pna, net = run()
    l2, g2_, _, _ = run()
    assert math.isfinite(l1) and l1 == l2
    for a, b in zip(g1, g2_):
        assert a is not None and torch.equal(a, b)
    p0, n0 = build(0.0)
    p0.load_state_dict(pna.state_dict()), n0.load_state_dict(net.state_dict())
    for m in (pna, net, p0, n0):
        m.eval()
    ga, gb = make_batch(amd, mols)
    a1, a2, b1, b2 = ga.local_copy(), ga.local_copy(), gb.local_copy(), gb.local_copy()      # (a forward overwrites the graph's features)
    with torch.no_grad():
        assert rel_err(pna(a1).cpu(), p0(a2).cpu()) < 1e-5
        assert rel_err(net(b1).cpu(), n0(b2).cpu()) < 1e-5


def test_pna_with_pairwise_distances_vs_reference_fixture(amd):
    """PNA(pairwise_distances=True), reference models/pna.py:105, 239-249: every layer's pretrans MLP also sees the squared distance of
    the edge's end points (ndata['x']).  The reference's own state_dict loads strictly (in_dim 3 F + 1); outputs, node embeddings,
    gradients and running statistics against the fixture tests/golden/gen_golden_pairwise.py made from the reference."""
    from test_oracle_golden import PNA_PAIRWISE
    z = load('pna_pairwise.npz')
    mols = mols_from_npz(z)
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **PNA_PAIRWISE)
    pna.load_state_dict(sd_from_npz(z, 'sd'), strict=True)
    pna.cuda().train()
    graphs = []
    for m in mols:
        g = amd.bond_graph(m)
        g.ndata['x'] = torch.from_numpy(m.coords.astype(np.float32))
        graphs.append(g)
    g2 = amd.batch(graphs).to('cuda:0')
    g_eval = g2.local_copy()             # (the forward overwrites ndata['feat'] / edata['feat'] with the embeddings, as the reference's)
    out = pna(g2)
    assert rel_err(g2.ndata['feat'].cpu(), z['node_emb']) < TOL
    assert rel_err(out.cpu(), z['out']) < TOL
    (out * torch.from_numpy(z['cot']).cuda()).sum().backward()
    grads_close(param_grads(pna), sd_from_npz(z, 'grad'), 5e-4)
    for k, v in sd_from_npz(z, 'sd_after').items():
        if 'running' in k:
            assert close(pna.state_dict()[k], v, TOL, 1e-6), k
    # eval mode (running statistics) through the same path
    pna.eval()
    with torch.no_grad():
        assert torch.isfinite(pna(g_eval)).all()
