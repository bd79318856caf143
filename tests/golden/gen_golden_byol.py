"""Fixture of BYOL pre-training (reference trainer/byol_wrapper.py BYOLwrapper :12-53, trainer/byol_trainer.py BYOLTrainer.forward_pass
:10-19, commons/losses.py CosineSimilarityLoss): the unmodified reference classes on seeded inputs -> tests/golden/byol.npz, data only.

    python tests/golden/gen_golden_byol.py          (imports the reference checkout, as gen_golden.py does)

Inputs: 6 synthetic molecules of six different sizes (synth.make_dataset(6, seed=5); every one has atoms of in-degree 1, asserted),
stored as in the other fixtures ('mol_*').  Models: PNA hidden 32, depth 2, target 32 and Net3D hidden 20, depth 1, target 32, the
other parameters of the yml files - except the PNA aggregators (max, std) and scalers (identity, attenuation): the posttrans weight is
(aggregators x scalers + 1) x hidden x hidden, and six copies of the yml's 13 x 32 x 32 per layer put the file above 1 MiB.
Wrappers (constructor arguments under WRAPPERS), two pairs as BYOLTrainer holds them (model, model3d):

    p1:  'pna_bn'   PNA,   predictor_layers 2, predictor_batchnorm True     'net3d_p1'  Net3D, predictor_layers 1, no BatchNorm
    p2:  'net3d_p2' Net3D, predictor_layers 2, predictor_batchnorm False    'net3d_p0'  Net3D, predictor_layers 0
         (p2: two 3D wrappers on the 3D graph - the pair only has to exercise forward_pass's two loss directions)

Weights: gen_golden.det_state_dict over the wrapper's whole state_dict (closed form; 'student.*' and 'teacher.*' get different values, so
the teacher is NOT a copy of the student here).  Stored per wrapper under '<name>/':
    sd/<key>              the full reference state_dict the forward starts from
    prediction_s, projection_t
    grad/<key>            gradients of every student and predictor parameter of the pair's loss
    bn_after/<key>        the teacher's BatchNorm buffers after that forward (train mode: batch statistics, buffers moved)
    student_after/<key>   student parameters after one torch.optim.Adam step (lr 1e-3) on those gradients
    teacher_after/<key>   teacher parameters after ma_teacher_update() with ma_decay = 0.9
(the teacher parameters in front of that update are the 'teacher.*' entries of sd - the optimizer does not hold them; asserted here and
not stored a second time: with them the file is above 1 MiB)
and per pair 'p1/loss', 'p2/loss': the symmetric loss of BYOLTrainer.forward_pass with the reference CosineSimilarityLoss, and its two
directions 'loss_a' (model's prediction against model3d's teacher) and 'loss_b'.

The file is written with fixed zip time stamps and one torch thread: it regenerates bit-identically.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

PNA_KW = dict(target_dim=32, hidden_dim=32, mid_batch_norm=True, last_batch_norm=True, readout_batchnorm=True, batch_norm_momentum=0.93,
              readout_hidden_dim=32, readout_layers=2, dropout=0.0, propagation_depth=2, aggregators=['max', 'std'],
              scalers=['identity', 'attenuation'], readout_aggregators=['min', 'max', 'mean'], pretrans_layers=2,
              posttrans_layers=1, residual=True)
NET3D_KW = dict(target_dim=32, hidden_dim=20, hidden_edge_dim=20, node_wise_output_layers=0, message_net_layers=1, update_net_layers=1,
                reduce_func='mean', fourier_encodings=4, propagation_depth=1, dropout=0.0, batch_norm=True, readout_batchnorm=True,
                batch_norm_momentum=0.93, readout_hidden_dim=20, readout_layers=1, readout_aggregators=['min', 'max', 'mean'])
# name -> (constructor arguments, further keyword arguments as train.py passes them, which graph)
WRAPPERS = {
    'pna_bn': (dict(model_type='PNA', model_parameters=PNA_KW, predictor_layers=2, predictor_hidden_size=24, predictor_batchnorm=True,
                    metric_dim=32), dict(avg_d=1.0, device='cpu'), '2d'),
    'net3d_p1': (dict(model_type='Net3D', model_parameters=NET3D_KW, predictor_layers=1, predictor_hidden_size=24, metric_dim=32),
                 dict(node_dim=0, edge_dim=1, avg_d=1.0), '3d'),
    'net3d_p2': (dict(model_type='Net3D', model_parameters=NET3D_KW, predictor_layers=2, predictor_hidden_size=24, predictor_batchnorm=False,
                      metric_dim=32), dict(node_dim=0, edge_dim=1, avg_d=1.0), '3d'),
    'net3d_p0': (dict(model_type='Net3D', model_parameters=NET3D_KW, predictor_layers=0), dict(node_dim=0, edge_dim=1, avg_d=1.0), '3d'),
}
PAIRS = {'p1': ('pna_bn', 'net3d_p1'), 'p2': ('net3d_p2', 'net3d_p0')}
MOL_SEED = 5
LR = 1e-3
MA_DECAY = 0.9


def main():
    import gen_golden as G
    import gen_golden_hardneg as GH
    import gen_golden_host as H
    torch.set_num_threads(1)
    dgl, PNA, Net3D, _, _, _ = H.import_host_side()
    from models.base_layers import MLP
    sys.modules['models'].__dict__.update(PNA=PNA, Net3D=Net3D, MLP=MLP)          # `from models import *` of byol_wrapper.py:8
    BYOLwrapper = importlib.import_module('trainer.byol_wrapper').BYOLwrapper
    BYOLTrainer = importlib.import_module('trainer.byol_trainer').BYOLTrainer
    CosineSimilarityLoss = importlib.import_module('commons.losses').CosineSimilarityLoss

    mols = G.synth.make_dataset(6, seed=MOL_SEED)
    assert len({m.n_atoms for m in mols}) == 6
    assert all((np.bincount(m.dst, minlength=m.n_atoms) == 1).any() for m in mols)
    out = G.mols_to_npz(mols)
    for pair, (na, nb) in PAIRS.items():
        ws = {}
        for name in (na, nb):
            kw, extra, _ = WRAPPERS[name]
            w = BYOLwrapper(**kw, **extra)
            w.load_state_dict(G.det_state_dict(w, f'byol/{name}'))
            w.train()
            assert not any(p.requires_grad for p in w.teacher.parameters())
            out.update(G.sd_np(w, f'{name}/sd'))
            ws[name] = w
        graphs = {}
        for name in (na, nb):
            g2, g3 = G.dgl_graphs(dgl, mols)
            graphs[name] = g2 if WRAPPERS[name][2] == '2d' else g3
        loss_func = CosineSimilarityLoss()
        trainer = types.SimpleNamespace(model=ws[na], model3d=ws[nb], loss_func=loss_func)
        loss, pred_a, pred_b = BYOLTrainer.forward_pass(trainer, (graphs[na], graphs[nb]))
        out[f'{pair}/loss'] = loss.detach().numpy().copy()
        loss.backward()
        for name, pred in ((na, pred_a), (nb, pred_b)):
            w = ws[name]
            out[f'{name}/prediction_s'] = pred.detach().numpy().copy()
            named = [(k, p) for k, p in w.named_parameters() if not k.startswith('teacher.')]
            assert all(p.grad is not None for _, p in named)
            assert all(p.grad is None for p in w.teacher.parameters())
            out.update({f'{name}/grad/{k}': p.grad.numpy().copy() for k, p in named})
            out.update({f'{name}/bn_after/{k}': v.numpy().copy() for k, v in w.state_dict().items()
                        if k.startswith('teacher.') and ('running' in k or 'num_batches' in k)})
        # forward_pass does not hand the teachers' projections out: a second wrapper with the same weights on the same input (the
        # wrappers above keep the state of exactly ONE forward: their BatchNorm buffers were taken just now)
        proj = {}
        for name in (na, nb):
            kw, extra, _ = WRAPPERS[name]
            w2 = BYOLwrapper(**kw, **extra)
            w2.load_state_dict(G.det_state_dict(w2, f'byol/{name}'))
            w2.train()
            g2, g3 = G.dgl_graphs(dgl, mols)
            p_s, p_t = w2(g2 if WRAPPERS[name][2] == '2d' else g3)
            assert not p_t.requires_grad
            assert torch.equal(p_s.detach(), torch.from_numpy(out[f'{name}/prediction_s']))
            proj[name] = p_t
            out[f'{name}/projection_t'] = p_t.numpy().copy()
        la = loss_func(torch.from_numpy(out[f'{na}/prediction_s']), proj[nb])
        lb = loss_func(proj[na], torch.from_numpy(out[f'{nb}/prediction_s']))
        assert torch.equal(la + lb, loss.detach())
        out[f'{pair}/loss_a'], out[f'{pair}/loss_b'] = la.numpy().copy(), lb.numpy().copy()
        print(f'{pair}: loss {float(loss):.6f} = {float(la):.6f} + {float(lb):.6f}')
        # one optimizer step over both wrappers' trainable parameters, then the teacher update of each
        params = [p for name in (na, nb) for p in ws[name].parameters() if p.requires_grad]
        torch.optim.Adam(params, lr=LR).step()
        for name in (na, nb):
            w = ws[name]
            w.ma_decay = MA_DECAY
            student = {k: p.detach().numpy().copy() for k, p in w.student.named_parameters()}
            before = {k: p.detach().numpy().copy() for k, p in w.teacher.named_parameters()}
            for k, v in before.items():
                assert np.array_equal(v, out[f'{name}/sd/teacher.{k}'])
            w.ma_teacher_update()
            after = {k: p.detach().numpy().copy() for k, p in w.teacher.named_parameters()}
            assert any(not np.array_equal(student[k], out[f'{name}/sd/student.{k}']) for k in student)
            out.update({f'{name}/student_after/{k}': v for k, v in student.items()})
            out.update({f'{name}/teacher_after/{k}': v for k, v in after.items()})
    out['lr'], out['ma_decay'] = np.array(LR), np.array(MA_DECAY)
    path = os.path.join(HERE, 'byol.npz')
    GH.write_npz(path, out)
    print('wrote byol.npz', len(out), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
