"""BYOL pre-training on the MI355X: the one-launch teacher update of csrc/ema.hip through its C ABI, and amd.BYOLwrapper
(3dinfomax_amd/byol.py) against the reference's own results (tests/golden/byol.npz, written by tests/golden/gen_golden_byol.py).

Kernel: one table of many tensors - every length around one float4 sweep of a block (1024) and around the chunk size the library reports -
at every alignment of the two pointers that decides between the float4 and the scalar loop, cut out of larger buffers whose other elements
(at least 8 on each side of every tensor) must come back bit-identical.  After ONE launch the teacher equals `t * d + s * (1 - d)` as torch
evaluates it on the same device with the Python float d, BIT FOR BIT; independently every element lies within 4 * 2^-24 * (|d t| + |(1 - d) s|)
of the fp64 value (two scalar conversions, two products and one sum at half an ulp each, rounded up).
Wrapper: outputs, both loss directions, gradients and the teacher's BatchNorm buffers with the tolerances and helpers tests/test_gpu_models.py
applies to PNA and Net3D against their own fixtures; three optimisation steps in which every teacher update is bit-exact, is one launch
over a table built once, and is what the teacher's next forward reads."""
import functools
import importlib

import pytest
import torch

import gen_golden_byol as GB
from helpers import close, grads_close, load, mols_from_npz, rel_err, sd_from_npz

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TOL = 1e-4                                           # tests/test_gpu_models.py
GUARD = 8
SHIFTS = [(0, 0), (1, 0), (0, 1), (1, 1)]            # elements, for (teacher, student)
DECAYS = [0.9, 0.99, 0.995, 0.0, 1.0]
byol = importlib.import_module('3dinfomax_amd.byol')          # (absent on the parent commit: every test here fails at import)


@pytest.fixture(scope='module')
def amd():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return importlib.import_module('3dinfomax_amd')


@pytest.fixture(scope='module')
def z():
    return load('byol.npz')


def _mods():
    return importlib.import_module('3dinfomax_amd._lib'), importlib.import_module('3dinfomax_amd.ops')


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ kernel

def lengths(chunk):
    return [1, 3, 4, 5, 1023, 1024, 1025, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]


@functools.lru_cache(maxsize=None)
def layout(chunk):
    """slots of one buffer per kind (teacher, student): tensor k of length n starts GUARD + shift elements into a slot that begins at a
    multiple of 4 elements and leaves at least GUARD elements behind it.  Returns (slots, total, idx): idx[kind] maps the concatenated
    logical elements of all tensors to positions of that kind's buffer."""
    slots, off = [], 0
    for n in lengths(chunk):
        for sh in SHIFTS:
            slots.append((off, n, sh))
            off += (n + 1 + 2 * GUARD + 3) // 4 * 4
    idx = [torch.cat([torch.arange(o + GUARD + sh[k], o + GUARD + sh[k] + n) for o, n, sh in slots]) for k in range(2)]
    return slots, off, idx


@functools.lru_cache(maxsize=None)
def logical_inputs(n_total):
    """teacher and student values of magnitudes 1e-6 .. 1e3 with both signs, drawn independently: elements where either term of the sum
    dominates by nine orders, and elements where they nearly cancel"""
    gen = torch.Generator().manual_seed(11)
    out = []
    for _ in range(2):
        mag = 10.0 ** (torch.rand(n_total, generator=gen, dtype=torch.float64) * 9.0 - 6.0)
        sign = 1.0 - 2.0 * torch.randint(0, 2, (n_total,), generator=gen).double()
        out.append((mag * sign).float())
    assert all(1e-6 <= float(x.abs().min()) and float(x.abs().max()) <= 1e3 and bool((x < 0).any()) and bool((x > 0).any()) for x in out)
    return tuple(out)


@pytest.fixture(scope='module')
def chunk(amd):
    return _mods()[0].load().i3d_ema_chunk_elems()


@pytest.mark.parametrize('d', DECAYS)
def test_kernel_is_the_torch_expression_bit_for_bit_and_within_the_fp64_allowance(chunk, d):
    Lm, ops = _mods()
    L = Lm.load()
    slots, total, idx = layout(chunk)
    t, s = logical = logical_inputs(idx[0].numel())
    host, dev = [], []
    for k in range(2):
        b = 12345.0 + torch.arange(total, dtype=torch.float32) * (k + 1)           # sentinels: finite, all different
        b[idx[k]] = logical[k]
        host.append(b)
        dev.append(b.to(DEV))
        assert dev[k].data_ptr() % 16 == 0
    views = [[dev[k][o + GUARD + sh[k]: o + GUARD + sh[k] + n] for o, n, sh in slots] for k in range(2)]
    for k in range(2):
        for (o, n, sh), w in zip(slots, views[k]):
            assert w.numel() == n and (w.data_ptr() % 16 == 0) == (sh[k] == 0)
    table = byol._EmaTable(*views)
    assert not table.fallback and table.n_chunks == sum((n + chunk - 1) // chunk for _, n, _ in slots)
    # what the reference's line computes on this device, from the same inputs, with the Python float d
    td, sd = t.to(DEV), s.to(DEV)
    want = (td * d + sd * (1. - d)).cpu()
    Lm.check(L.i3d_ema_update(table.table.data_ptr(), table.n_chunks, d, 1.0 - d, ops._stream()), 'i3d_ema_update')
    torch.cuda.synchronize()
    out = [x.cpu() for x in dev]
    assert torch.equal(_bits(out[1]), _bits(host[1])), 'the student buffer changed'
    outside = torch.ones(total, dtype=torch.bool)
    outside[idx[0]] = False
    assert int(outside.sum()) >= 2 * GUARD * len(slots)
    assert torch.equal(_bits(out[0])[outside], _bits(host[0])[outside]), 'a guard element of the teacher buffer changed'
    got = out[0][idx[0]]
    t64, s64 = t.double(), s.double()
    exact = d * t64 + (1.0 - d) * s64
    allow = 4 * 2.0 ** -24 * ((d * t64).abs() + ((1.0 - d) * s64).abs())
    err = (got.double() - exact).abs()
    ratio = torch.where(allow > 0, err / allow.clamp(min=1e-300), (err > 0).double() * float('inf'))
    print(f'ema kernel d={d}: largest error / allowance {float(ratio.max()):.3f} over {got.numel()} elements in {len(slots)} tensors, '
          f'{table.n_chunks} chunks; bit mismatches against torch {int((_bits(got) != _bits(want)).sum())}')
    assert torch.equal(_bits(got), _bits(want)), 'not the reference expression bit for bit'
    assert float(ratio.max()) <= 1.0
    if d == 1.0:
        assert torch.equal(_bits(got), _bits(t)), 'ma_decay 1 leaves the teacher bit-identical'
    elif d == 0.0:
        assert torch.equal(_bits(got), _bits(s)), 'ma_decay 0 makes the teacher bit-equal to the student'
    else:
        assert not torch.equal(got, t)


def test_kernel_entry_point_refuses_bad_arguments(amd):
    L = _mods()[0].load()
    table = torch.zeros(24, dtype=torch.uint8, device=DEV)
    assert L.i3d_ema_update(None, 1, 0.9, 0.1, None) == -1 and b'bad arguments' in L.i3d_last_error()
    for n in (0, -1):
        assert L.i3d_ema_update(table.data_ptr(), n, 0.9, 0.1, None) == -1 and b'bad arguments' in L.i3d_last_error()


# ----------------------------------------------------------------------------------------------------------------- wrapper

def make(amd, z, name):
    kw, extra, _ = GB.WRAPPERS[name]
    if 'device' in extra:
        extra = dict(extra, device='cuda:0')
    w = amd.BYOLwrapper(**kw, **extra)
    w.load_state_dict(sd_from_npz(z, f'{name}/sd'), strict=True)
    return w.cuda().train()


def graph_for(amd, z, name):
    mols = mols_from_npz(z)
    build = amd.bond_graph if GB.WRAPPERS[name][2] == '2d' else amd.complete_graph
    return amd.batch([build(m) for m in mols]).to('cuda:0')


def trainable_grads(w, part):
    return {k[len(part) + 1:]: p.grad for k, p in w.named_parameters() if k.startswith(part + '.')}


@pytest.mark.parametrize('pair', sorted(GB.PAIRS))
def test_wrappers_vs_reference_fixture(amd, z, pair):
    na, nb = GB.PAIRS[pair]
    wa, wb = make(amd, z, na), make(amd, z, nb)
    pred_a, proj_a = wa(graph_for(amd, z, na))
    pred_b, proj_b = wb(graph_for(amd, z, nb))
    for name, pred, proj in ((na, pred_a, proj_a), (nb, pred_b, proj_b)):
        assert pred.requires_grad and not proj.requires_grad and proj.grad_fn is None
        assert rel_err(pred.detach().cpu(), z[f'{name}/prediction_s']) < TOL, name
        assert rel_err(proj.cpu(), z[f'{name}/projection_t']) < TOL, name
    loss_fn = amd.CosineSimilarityLoss()
    la, lb = loss_fn(pred_a, proj_b), loss_fn(proj_a, pred_b)          # reference trainer/byol_trainer.py:16-18
    loss = la + lb
    for got, key in ((la, 'loss_a'), (lb, 'loss_b'), (loss, 'loss')):
        ref = float(z[f'{pair}/{key}'])
        assert abs(got.item() - ref) < TOL * abs(ref), key
    loss.backward()
    for name, w in ((na, wa), (nb, wb)):
        ref = sd_from_npz(z, f'{name}/grad')
        for part in ('student', 'predictor') if w.predictor_layers > 0 else ('student',):
            grads_close(trainable_grads(w, part), {k[len(part) + 1:]: v for k, v in ref.items() if k.startswith(part + '.')}, 5e-4,
                        f'{name} {part} ')
        assert all(p.grad is None for p in w.teacher.parameters())
        sd = w.state_dict()
        after = sd_from_npz(z, f'{name}/bn_after')
        assert after and all(k.startswith('teacher.') for k in after)
        for k, v in after.items():
            assert close(sd[k], v, TOL, 1e-6), k


def byol_step(amd, z, wa, wb, ga, gb, loss_fn, opt):
    pred_a, proj_a = wa(ga.local_copy())
    pred_b, proj_b = wb(gb.local_copy())
    loss = loss_fn(pred_a, proj_b) + loss_fn(proj_a, pred_b)
    loss.backward()
    opt.step()
    opt.zero_grad()
    return proj_a, proj_b


def fresh_teacher_output(amd, name, w, g):
    """a newly built model of the inner type with the teacher's current state_dict (copied), run the way the wrapper runs its teacher:
    train mode, without autograd, parameters frozen"""
    kw, extra, _ = GB.WRAPPERS[name]
    m = getattr(amd, kw['model_type'])(**kw['model_parameters'], **extra)
    m.load_state_dict({k: v.detach().clone().cpu() for k, v in w.teacher.state_dict().items()}, strict=True)
    m.cuda().train()
    for p in m.parameters():
        p.requires_grad = False
    with torch.no_grad():
        return m(g.local_copy())


def test_three_steps_leave_no_stale_state_and_launch_once_per_update(amd, z, monkeypatch):
    Lm, _ = _mods()
    L = Lm.load()
    count = {'launch': 0, 'build': 0}
    real = L.i3d_ema_update
    monkeypatch.setattr(L, 'i3d_ema_update', lambda *a: (count.__setitem__('launch', count['launch'] + 1), real(*a))[1])

    class CountedTable(byol._EmaTable):
        def __init__(self, *a):
            count['build'] += 1
            super().__init__(*a)
    monkeypatch.setattr(byol, '_EmaTable', CountedTable)

    na, nb = GB.PAIRS['p1']
    ws = {na: make(amd, z, na), nb: make(amd, z, nb)}
    gs = {na: graph_for(amd, z, na), nb: graph_for(amd, z, nb)}
    d = 0.9
    for w in ws.values():
        w.ma_decay = d
    loss_fn = amd.CosineSimilarityLoss()
    opt = amd.Adam([p for w in ws.values() for p in w.parameters() if p.requires_grad], lr=1e-3)
    expected = None
    for step in range(4):
        proj = dict(zip((na, nb), byol_step(amd, z, ws[na], ws[nb], gs[na], gs[nb], loss_fn, opt)))
        if expected is not None:
            # the teacher's forward after an update reads the updated weights: the same bits as a model built from them just now
            for name in ws:
                assert torch.equal(_bits(proj[name]), _bits(expected[name])), (step, name)
                assert not torch.equal(proj[name], last[name]), 'the projection did not move with the update'
        last = proj
        if step == 3:
            break
        for name, w in ws.items():
            before = [p.detach().clone() for p in w.teacher.parameters()]
            ptrs = [p.data_ptr() for p in w.teacher.parameters()]
            launches = count['launch']
            w.ma_teacher_update()
            assert count['launch'] == launches + 1, 'ONE launch for all parameter pairs'
            for t, t0, s in zip(w.teacher.parameters(), before, w.student.parameters()):
                assert torch.equal(_bits(t), _bits(t0 * d + s.detach() * (1. - d))), (step, name)
            assert [p.data_ptr() for p in w.teacher.parameters()] == ptrs
        expected = {name: fresh_teacher_output(amd, name, w, gs[name]) for name, w in ws.items()}
    assert count == {'launch': 6, 'build': 2}, count                 # two wrappers: one table each over the three steps
    for name, w in ws.items():
        tab = w.__dict__['_i3d_ema']
        assert not tab.fallback and tab.n_chunks >= len(list(w.teacher.parameters()))
    # every parameter in a new storage (the old ones stay alive, so the allocator cannot hand their addresses out again)
    w = ws[na]
    old = [p.data for p in w.parameters()]
    old_bits = [_bits(x).clone() for x in old]
    w.to('cpu')
    w.to('cuda:0')
    assert all(p.data_ptr() != o.data_ptr() for p, o in zip(w.parameters(), old))
    before = [p.detach().clone() for p in w.teacher.parameters()]
    w.ma_teacher_update()
    assert count == {'launch': 7, 'build': 3}, count
    for t, t0, s in zip(w.teacher.parameters(), before, w.student.parameters()):
        assert torch.equal(_bits(t), _bits(t0 * d + s.detach() * (1. - d)))
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(o), b) for o, b in zip(old, old_bits)), 'the old storage was written'
    w.ma_teacher_update()
    assert count == {'launch': 8, 'build': 3}, count


@pytest.mark.parametrize('name', ['pna_bn', 'net3d_p1'])
def test_caller_s_graph_holds_the_student_s_state_and_its_inputs_are_unchanged(amd, z, name):
    w = make(amd, z, name)
    g = graph_for(amd, z, name)
    inputs = {('n', k): v for k, v in g.ndata.items()}
    inputs.update({('e', k): v for k, v in g.edata.items()})
    keep = {k: v.clone() for k, v in inputs.items()}
    alone, for_teacher = g.local_copy(), g.local_copy()
    w(g)
    z_alone = w.student(alone)                     # what the inner model leaves on a graph it is given directly
    assert z_alone.requires_grad
    assert set(g.ndata) == set(alone.ndata) and set(g.edata) == set(alone.edata)
    for k in alone.ndata:
        assert torch.equal(g.ndata[k], alone.ndata[k]), k
    for k in alone.edata:
        assert torch.equal(g.edata[k], alone.edata[k]), k
    assert g.ndata['feat'].dtype == torch.float32
    with torch.no_grad():
        w.teacher(for_teacher)
    assert not torch.equal(g.ndata['feat'], for_teacher.ndata['feat']), "the teacher's node state landed on the caller's graph"
    for k, v in inputs.items():
        assert torch.equal(v, keep[k]), k
