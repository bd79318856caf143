"""BYOLwrapper (3dinfomax_amd/byol.py) without a GPU: the plugin surface, the state_dict against the reference's own (tests/golden/byol.npz,
written by tests/golden/gen_golden_byol.py from the unmodified reference classes), and the teacher update's arithmetic on the CPU path -
`t.mul_(d).add_(s * (1 - d))`, which must give the reference's `t * d + s * (1 - d)` BIT FOR BIT (three roundings per element)."""
import copy
import importlib
import inspect

import pytest
import torch

import gen_golden_byol as GB
import launch_reference as launcher
from helpers import amd, load, mols_from_npz, sd_from_npz

byol = importlib.import_module('3dinfomax_amd.byol')
SYMBOLS = ('i3d_ema_chunk_elems', 'i3d_ema_chunk_bytes', 'i3d_ema_update')


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def make(name, **over):
    kw, extra, _ = GB.WRAPPERS[name]
    return amd.BYOLwrapper(**dict(kw, **over), **extra)


@pytest.fixture(scope='module')
def z():
    return load('byol.npz')


def after_adam(z, name):
    """the wrapper in the fixture's state in front of ma_teacher_update(): student after the Adam step, teacher as loaded"""
    w = make(name)
    w.load_state_dict(sd_from_npz(z, f'{name}/sd'), strict=True)
    w.student.load_state_dict(sd_from_npz(z, f'{name}/student_after'), strict=False)
    w.ma_decay = float(z['ma_decay'])
    return w


# ------------------------------------------------------------------------------------------------------------- surface

def test_name_resolves_from_the_package_the_alias_and_the_launcher():
    alias = importlib.import_module('infomax3d_amd')
    assert 'BYOLwrapper' in amd.__all__ and 'BYOLwrapper' in alias.__all__
    assert amd.BYOLwrapper is alias.BYOLwrapper is byol.BYOLwrapper is launcher.plugin_names()['BYOLwrapper']
    assert amd.byol is byol
    assert not hasattr(amd.BYOLwrapper, 'attach_group')          # no data-parallel form of its own
    namespace = {'BYOLwrapper': object()}
    assert 'BYOLwrapper' in launcher.rebind(namespace, launcher.plugin_names()) and namespace['BYOLwrapper'] is amd.BYOLwrapper


def test_constructor_signature_and_defaults_are_the_reference_s():
    """reference trainer/byol_wrapper.py:17-25"""
    params = [q for q in inspect.signature(amd.BYOLwrapper.__init__).parameters.values() if q.name != 'self']
    assert [(q.name, q.default) for q in params[:-1]] == [
        ('model_type', inspect.Parameter.empty), ('model_parameters', inspect.Parameter.empty), ('predictor_layers', 1),
        ('predictor_hidden_size', 256), ('predictor_batchnorm', False), ('metric_dim', 256), ('ma_decay', 0.99)]
    assert params[-1].name == 'kwargs' and params[-1].kind is inspect.Parameter.VAR_KEYWORD
    assert [q.name for q in inspect.signature(amd.BYOLwrapper.forward).parameters.values()] == ['self', 'graph']
    assert list(inspect.signature(amd.BYOLwrapper.ma_teacher_update).parameters) == ['self']
    w = amd.BYOLwrapper('Net3D', GB.NET3D_KW, node_dim=0, edge_dim=1, avg_d=1.0)
    assert w.ma_decay == 0.99 and w.predictor_layers == 1
    fc = list(w.predictor.fully_connected)
    assert len(fc) == 1 and fc[0].in_dim == GB.NET3D_KW['target_dim'] and fc[0].out_dim == 256 and fc[0].batch_norm is None


def test_header_declares_the_kernel_and_the_library_exports_it():
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module('3dinfomax_amd._lib')
    lib = L.load()
    declared = L.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.i3d_abi_version() == 2
    assert lib.i3d_ema_chunk_bytes() == 24 and lib.i3d_ema_chunk_elems() >= 1024 and lib.i3d_ema_chunk_elems() % 4 == 0
    # argument validation happens on the host before any launch: no GPU needed
    assert lib.i3d_ema_update(None, 4, 0.9, 0.1, None) == -1 and b'bad arguments' in lib.i3d_last_error()
    for n in (0, -3):
        assert lib.i3d_ema_update(ctypes_address(), n, 0.9, 0.1, None) == -1 and b'bad arguments' in lib.i3d_last_error()


def ctypes_address():
    import ctypes
    return ctypes.addressof(ctypes.create_string_buffer(64))


def test_unknown_inner_model_type_is_a_value_error():
    for name in ('NoSuchModel', 'batch', 'BYOLwrapper', 'synth'):
        with pytest.raises(ValueError, match=name):
            amd.BYOLwrapper(name, dict(target_dim=8))


# ---------------------------------------------------------------------------------------------------------- state_dict

@pytest.mark.parametrize('name', sorted(GB.WRAPPERS))
def test_state_dict_is_the_reference_s_and_loads_strictly(z, name):
    ref = sd_from_npz(z, f'{name}/sd')
    w = make(name)
    own = w.state_dict()
    assert set(own) == set(ref)
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    assert {k.split('.')[0] for k in own} == ({'student', 'teacher', 'predictor'} if GB.WRAPPERS[name][0]['predictor_layers'] else {'student', 'teacher'})
    w.load_state_dict(ref, strict=True)
    for k, v in w.state_dict().items():
        assert torch.equal(v, ref[k]), k
    # reference train.py:218-221: a BYOL checkpoint's student goes into the bare model by key.replace('student.', '')
    inner = getattr(amd, GB.WRAPPERS[name][0]['model_type'])(**GB.WRAPPERS[name][0]['model_parameters'], **GB.WRAPPERS[name][1])
    inner.load_state_dict({k.replace('student.', ''): v for k, v in ref.items() if k.startswith('student.')}, strict=True)


@pytest.mark.parametrize('name', sorted(GB.WRAPPERS))
def test_teacher_is_a_frozen_copy_that_shares_nothing_with_the_student(name):
    w = make(name)
    assert all(p.requires_grad for p in w.student.parameters())
    assert all(not p.requires_grad for p in w.teacher.parameters())
    if w.predictor_layers > 0:
        assert all(p.requires_grad for p in w.predictor.parameters())
    ts = list(w.teacher.state_dict().items())
    ss = list(w.student.state_dict().items())
    assert [k for k, _ in ts] == [k for k, _ in ss]
    s_ptrs = {v.untyped_storage().data_ptr() for _, v in ss}
    for (k, t), (_, s) in zip(ts, ss):
        assert torch.equal(t, s), k                                      # a copy of the initial student ...
        assert t.untyped_storage().data_ptr() not in s_ptrs, k           # ... in storages of its own
    # nothing the package caches per module exists on either copy before the first forward
    for m in list(w.student.modules()) + list(w.teacher.modules()):
        assert not [k for k in m.__dict__ if k.startswith('_i3d_') or k == '_comb_cache'], type(m)


def test_cached_views_of_the_two_copies_hold_their_own_parameters():
    """layers.FCLayer.hot() and tape._param_list() fill on first use: each copy's entries are that copy's own Parameter objects"""
    tape = importlib.import_module('3dinfomax_amd.tape')
    layers = importlib.import_module('3dinfomax_amd.layers')
    w = make('pna_bn')
    own = {}
    for tag, m in (('student', w.student), ('teacher', w.teacher)):
        ids = {id(p) for p in m.parameters()}
        own[tag] = ids
        assert [id(p) for p in tape._param_list(m)] == [id(p) for p in m.parameters()]
        for fc in m.modules():
            if isinstance(fc, layers.FCLayer):
                h = fc.hot()
                assert all(id(t) in ids for t in h[:4] if isinstance(t, torch.nn.Parameter))
    assert not (own['student'] & own['teacher'])
    assert tape.model_state(w.student) is not tape.model_state(w.teacher)
    both = copy.deepcopy(w)                                               # and a copy of the whole wrapper starts without tape state
    assert '_i3d_state' not in both.student.__dict__ or both.student.__dict__['_i3d_state'] is None


# ------------------------------------------------------------------------------------------------------ teacher update

@pytest.mark.parametrize('name', sorted(GB.WRAPPERS))
def test_cpu_update_gives_the_reference_s_teacher_bit_for_bit(z, name):
    w = after_adam(z, name)
    ptrs = [p.data_ptr() for p in w.teacher.parameters()]
    buffers = {k: v.clone() for k, v in w.teacher.named_buffers()}
    student = [p.detach().clone() for p in w.student.parameters()]
    w.ma_teacher_update()
    want = sd_from_npz(z, f'{name}/teacher_after')
    got = dict(w.teacher.named_parameters())
    assert set(got) == set(want)
    changed = 0
    for k, p in got.items():
        assert torch.equal(_bits(p), _bits(want[k])), k
        changed += int(not torch.equal(p.detach(), sd_from_npz(z, f'{name}/sd')['teacher.' + k]))
        assert not p.requires_grad and p.grad is None
    assert changed == len(got)
    assert [p.data_ptr() for p in w.teacher.parameters()] == ptrs, 'the update is in place'
    for k, v in w.teacher.named_buffers():
        assert torch.equal(v, buffers[k]), f'buffer {k} was averaged'
    for p, q in zip(w.student.parameters(), student):
        assert torch.equal(_bits(p), _bits(q))


def test_ma_decay_is_read_at_call_time_and_its_end_points_are_exact(z):
    w = after_adam(z, 'net3d_p1')
    before = [p.detach().clone() for p in w.teacher.parameters()]
    w.ma_decay = 1
    w.ma_teacher_update()
    for p, q in zip(w.teacher.parameters(), before):
        assert torch.equal(_bits(p), _bits(q))
    w.ma_decay = 0.5
    w.ma_teacher_update()
    for p, q, s in zip(w.teacher.parameters(), before, w.student.parameters()):
        assert torch.equal(_bits(p), _bits(q * 0.5 + s.detach() * 0.5))
    w.ma_decay = 0
    w.ma_teacher_update()
    for p, s in zip(w.teacher.parameters(), w.student.parameters()):
        assert not bool(((s == 0) & torch.signbit(s)).any())          # (t * 0 + s is +0 where s is -0: none here)
        assert torch.equal(_bits(p), _bits(s))
    assert all(p.data_ptr() != s.data_ptr() for p, s in zip(w.teacher.parameters(), w.student.parameters()))


def test_a_non_contiguous_pair_takes_the_torch_expression_and_gives_the_same_bits(z):
    name = 'net3d_p2'
    w = after_adam(z, name)
    key = 'output.fully_connected.0.linear.weight'
    for m in (w.teacher, w.student):
        p = dict(m.named_parameters())[key]
        p.data = p.data.t().contiguous().t()               # same values, transposed memory
        assert not p.is_contiguous()
    tab = byol._EmaTable(list(w.teacher.parameters()), list(w.student.parameters()))
    assert tab.n_chunks == 0 and len(tab.fallback) == len(list(w.teacher.parameters()))      # (CPU: every pair)
    w.ma_teacher_update()
    want = sd_from_npz(z, f'{name}/teacher_after')
    for k, p in w.teacher.named_parameters():
        assert torch.equal(_bits(p), _bits(want[k])), k
    assert not dict(w.teacher.named_parameters())[key].is_contiguous()


# -------------------------------------------------------------------------------------------------------------- forward

class _Recorder(torch.nn.Module):
    """stands in for an inner model (which runs on the GPU only): records the graph it was given, overwrites its frames as the models do"""

    def __init__(self, value):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((1,), float(value)))
        self.seen = None

    def forward(self, g):
        self.seen = (g, dict(g.ndata), dict(g.edata), torch.is_grad_enabled())
        g.ndata['feat'] = torch.zeros(g.number_of_nodes(), 3) + self.w
        g.edata['feat'] = torch.zeros(g.number_of_edges(), 3) + self.w
        return self.w.expand(g.batch_size, 4) * 1.0


class _DglLike:
    """the surface as_batched_graph accepts"""

    def __init__(self, g):
        self._g = g
        self.ndata, self.edata = dict(g.ndata), dict(g.edata)

    def edges(self):
        return self._g.edges()

    def number_of_nodes(self):
        return self._g.number_of_nodes()

    def batch_num_nodes(self):
        return self._g.batch_num_nodes()


@pytest.mark.parametrize('dgl_like', [False, True])
@pytest.mark.parametrize('predictor_layers', [0, 1])
def test_forward_hands_the_teacher_frames_of_its_own_around_the_same_tensors(z, predictor_layers, dgl_like):
    mols = mols_from_npz(z)
    g = amd.batch([amd.bond_graph(m) for m in mols])
    feat, efeat = g.ndata['feat'], g.edata['feat']
    keep = (feat.clone(), efeat.clone())
    graph = _DglLike(g) if dgl_like else g
    w = make('net3d_p1', predictor_layers=predictor_layers, metric_dim=4)
    w.student, w.teacher = _Recorder(2.0), _Recorder(5.0)
    for p in w.teacher.parameters():
        p.requires_grad = False
    if predictor_layers:
        w.predictor = torch.nn.Identity()
    was_training = w.training
    pred, proj = w(graph)
    assert w.training == was_training
    sg, s_nd, s_ed, s_grad = w.student.seen
    tg, t_nd, t_ed, t_grad = w.teacher.seen
    assert s_grad and not t_grad
    assert pred.requires_grad and not proj.requires_grad
    assert float(pred.detach()[0, 0]) == 2.0 and float(proj[0, 0]) == 5.0
    if predictor_layers == 0:
        assert pred.grad_fn is not None and pred.data_ptr() != proj.data_ptr()
    # both saw the caller's input tensors themselves (no copy) ...
    assert s_nd['feat'] is feat and t_nd['feat'] is feat and s_ed['feat'] is efeat and t_ed['feat'] is efeat
    # ... through different frames and the same kernel index
    assert tg is not sg and tg.ndata is not sg.ndata and tg.edata is not sg.edata
    assert tg.index() is sg.index()
    # the caller's graph holds the STUDENT's node state; its input tensors are unchanged
    assert float(graph.ndata['feat'][0, 0]) == 2.0 and float(graph.edata['feat'][0, 0]) == 2.0
    assert float(tg.ndata['feat'][0, 0]) == 5.0
    assert torch.equal(feat, keep[0]) and torch.equal(efeat, keep[1])


def test_predictor_layers_zero_returns_the_projection_itself(z):
    w = make('net3d_p0')
    assert not hasattr(w, 'predictor')
    out = torch.ones(6, 4, requires_grad=True) * 3.0
    w.student = type('S', (torch.nn.Module,), {'forward': lambda self, g: out})()
    w.teacher = type('T', (torch.nn.Module,), {'forward': lambda self, g: torch.zeros(6, 4)})()
    g = amd.batch([amd.bond_graph(m) for m in mols_from_npz(z)])
    pred, proj = w(g)
    assert pred is out and not proj.requires_grad
