"""The one-launch Adam step on the MI355X against fp64 (tests/adam_reference.py): the kernel of csrc/adam.hip through `_NativeTable`
and `i3d_adam_step` directly, and `amd.Adam` (3dinfomax_amd/optim.py) on bare parameters through the changes of its host state.

Kernel: every tensor length around one float4 sweep of a block (1024) and around the chunk size the library reports, at every
alignment of the four pointers that decides between the float4 and the scalar loop, cut out of larger buffers whose other elements
(at least 8 on each side of every tensor) must come back bit-identical.  All tensors of one case are ONE launch - the kernel's own
use: a table of many tensors - and one fp64 evaluation over all their elements.
Optimizer: gradients assigned by hand, every step checked from the fp32 state in front of it with each parameter's OWN step count;
`torch._fused_adam_` and the library's `i3d_adam_step` are counted, and every scenario says which of the two ran at which step.
Every check prints its error / allowance ratios (exp_avg, exp_avg_sq, param) before it asserts; DESIGN.md ('Adam step') has the largest."""
import copy
import functools
import importlib
import math

import pytest
import torch

import adam_reference as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GUARD = 8
SHIFTS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)]      # elements, for (p, g, m, v)
HYPERS = {                       # lr, betas, eps, weight_decay
    'default': (1e-3, (0.9, 0.999), 1e-8, 0.0),
    'reference_lr': (8e-5, (0.9, 0.999), 1e-8, 0.0),
    'weight_decay': (1e-3, (0.9, 0.999), 1e-8, 1e-2),
    'beta1_zero': (1e-3, (0.0, 0.5), 1e-3, 0.0),
    'lr_zero': (0.0, (0.9, 0.999), 1e-8, 0.0),
}
STEP_COUNTS = [1, 2, 10, 1000, 10 ** 6]
WORST = {'kernel': [0.0, 0.0, 0.0], 'optimizer': [0.0, 0.0, 0.0]}


@pytest.fixture(scope='module')
def amd():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return importlib.import_module('3dinfomax_amd')


def _mods():
    return (importlib.import_module('3dinfomax_amd.optim'), importlib.import_module('3dinfomax_amd._lib'),
            importlib.import_module('3dinfomax_amd.ops'))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _note(kind, tag, ratios):
    WORST[kind] = [max(a, b) for a, b in zip(WORST[kind], ratios)]
    print(f'{tag}: error / allowance  m {ratios[0]:.3f}  v {ratios[1]:.3f}  p {ratios[2]:.3f}   '
          f'(largest so far, {kind}: m {WORST[kind][0]:.3f}  v {WORST[kind][1]:.3f}  p {WORST[kind][2]:.3f})')


# ------------------------------------------------------------------------------------------------------------------ kernel

def lengths(chunk):
    return [1, 3, 4, 5, 1023, 1024, 1025, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 3 * chunk]


@functools.lru_cache(maxsize=None)
def layout(chunk, only=None, shifts=tuple(SHIFTS)):
    """slots of one buffer per kind (p, g, m, v): tensor k of length n starts GUARD + shift elements into a slot that begins at a
    multiple of 4 elements and leaves GUARD elements behind it.  Returns (slots, total, idx): idx[kind] maps the concatenated logical
    elements of all tensors to positions of that kind's buffer."""
    slots, off = [], 0
    for n in (lengths(chunk) if only is None else only):
        for sh in shifts:
            slots.append((off, n, sh))
            off += (n + 1 + 2 * GUARD + 3) // 4 * 4
    idx = [torch.cat([torch.arange(o + GUARD + sh[k], o + GUARD + sh[k] + n) for o, n, sh in slots]) for k in range(4)]
    return slots, off, idx


def logical_inputs(n_total, seed, zero=False):
    """p of the parameter scales; g, m, v of the gradient scale list with both signs - m and v on scales of their own, so that
    |m| / sqrt(v) is far from 1 in both directions in many elements"""
    gen = torch.Generator().manual_seed(seed)
    p = R.param_values(n_total, gen)
    if zero:
        z = torch.zeros(n_total)
        return p, z, z.clone(), z.clone()
    i = torch.arange(n_total)
    scales = torch.tensor(R.GRAD_SCALES, dtype=torch.float64)
    g = R.grad_values(n_total, gen)
    sign = 1.0 - 2.0 * torch.randint(0, 2, (n_total,), generator=gen).double()
    m = (scales[(i + i // 8) % 8] * R.unit(n_total, gen) * sign).float()
    v = ((scales[(i + i // 64) % 8] * R.unit(n_total, gen)) ** 2).float()
    return p, g, m, v


def run_kernel(chunk, lay, logical, hyper, t, n_steps=3):
    """one launch over every tensor of the layout; asserts g, the step counters' neighbours and every sentinel bit-identical;
    returns the logical (p, m, v) after the step and the step counters before / after"""
    O, Lm, ops = _mods()
    L = Lm.load()
    slots, total, idx = lay
    lr, betas, eps, wd = hyper
    host, dev = [], []
    for k in range(4):
        b = 12345.0 + torch.arange(total, dtype=torch.float32) * (k + 1)           # sentinels: finite, all different
        b[idx[k]] = logical[k]
        host.append(b)
        dev.append(b.to(DEV))
        assert dev[k].data_ptr() % 16 == 0
    views = [[dev[k][o + GUARD + sh[k]: o + GUARD + sh[k] + n] for o, n, sh in slots] for k in range(4)]
    for k in range(4):
        for (o, n, sh), w in zip(slots, views[k]):
            assert w.numel() == n and (w.data_ptr() % 16 == 0) == (sh[k] == 0)
    table = O._NativeTable(*views)
    assert table.n_chunks == sum((n + chunk - 1) // chunk for _, n, _ in slots)
    steps_host = torch.full((n_steps + 2 * GUARD,), -7.0)
    steps_host[GUARD:GUARD + n_steps] = torch.arange(n_steps, dtype=torch.float32) * 3.0 + (t - 1)
    steps = steps_host.to(DEV)
    bc1, bc2s = 1 - betas[0] ** t, math.sqrt(1 - betas[1] ** t)                   # as optim.py forms them
    Lm.check(L.i3d_adam_step(table.table.data_ptr(), table.n_chunks, steps[GUARD:].data_ptr(), n_steps, float(lr), float(betas[0]),
                             float(betas[1]), float(wd), float(eps), bc1, bc2s, ops._stream()), 'i3d_adam_step')
    torch.cuda.synchronize()
    out = [d.cpu() for d in dev]
    assert torch.equal(_bits(out[1]), _bits(host[1])), 'the gradient buffer changed'
    for k in (0, 2, 3):
        outside = torch.ones(total, dtype=torch.bool)
        outside[idx[k]] = False
        assert int(outside.sum()) >= 2 * GUARD * len(slots)
        assert torch.equal(_bits(out[k])[outside], _bits(host[k])[outside]), f'a sentinel of buffer {"pgmv"[k]} changed'
    steps_out = steps.cpu()
    inside = torch.zeros_like(steps_host, dtype=torch.bool)
    inside[GUARD:GUARD + n_steps] = True
    assert torch.equal(_bits(steps_out)[~inside], _bits(steps_host)[~inside]), 'a sentinel of the step counters changed'
    assert torch.equal(steps_out[inside], steps_host[inside] + 1.0), 'every step counter rises by exactly 1.0'
    return out[0][idx[0]], out[2][idx[2]], out[3][idx[3]]


@pytest.fixture(scope='module')
def chunk(amd):
    return _mods()[1].load().i3d_adam_chunk_elems()


@pytest.mark.parametrize('t', STEP_COUNTS)
@pytest.mark.parametrize('hyper', list(HYPERS))
def test_kernel_against_fp64(chunk, hyper, t):
    lay = layout(chunk)
    p, g, m, v = logical = logical_inputs(lay[2][0].numel(), seed=7)
    lr, betas, eps, wd = HYPERS[hyper]
    p_out, m_out, v_out = run_kernel(chunk, lay, logical, HYPERS[hyper], t)
    ratios = R.adam_ratios(p, g, m, v, p_out, m_out, v_out, t, lr, betas, eps, wd)
    _note('kernel', f'kernel {hyper} t={t}', ratios)
    assert max(ratios) <= 1.0, ratios
    if lr == 0:
        assert torch.equal(_bits(p_out), _bits(p)), 'lr 0 leaves the parameters bit-identical'
        assert not torch.equal(m_out, m) and not torch.equal(v_out, v), 'lr 0: exp_avg and exp_avg_sq still advance'
    else:
        assert not torch.equal(p_out, p)


@pytest.mark.parametrize('hyper', ['default', 'reference_lr', 'beta1_zero', 'lr_zero'])
def test_kernel_zero_gradient_and_state_leave_the_parameters_alone(chunk, hyper):
    lay = layout(chunk)
    p, g, m, v = logical = logical_inputs(lay[2][0].numel(), seed=8, zero=True)
    p_out, m_out, v_out = run_kernel(chunk, lay, logical, HYPERS[hyper], 2)
    assert torch.equal(_bits(p_out), _bits(p))
    assert not bool(m_out.count_nonzero()) and not bool(v_out.count_nonzero())


@pytest.mark.parametrize('hyper', ['default', 'weight_decay'])
def test_kernel_inf_and_nan_gradients_stay_in_their_elements(chunk, hyper):
    """+inf inside a float4 group (element 1) and NaN in the last element (the n % 4 tail where there is one), in every tensor of 5
    elements and more, at every alignment: non-finite p, m, v in exactly these elements - where the fp64 formula has them - and every
    other element inside the allowances"""
    lay = layout(chunk)
    slots = lay[0]
    p, g, m, v = logical_inputs(lay[2][0].numel(), seed=9)
    bad, start = [], 0
    for _, n, _ in slots:
        if n >= 5:
            g[start + 1] = math.inf
            g[start + n - 1] = math.nan
            bad += [start + 1, start + n - 1]
        start += n
    expected = torch.zeros(g.numel(), dtype=torch.bool)
    expected[bad] = True
    lr, betas, eps, wd = HYPERS[hyper]
    p_out, m_out, v_out = run_kernel(chunk, lay, (p, g, m, v), HYPERS[hyper], 2)
    for name, x in (('p', p_out), ('exp_avg', m_out), ('exp_avg_sq', v_out)):
        assert torch.equal(~torch.isfinite(x), expected), f'{name}: non-finite elements are not exactly the poisoned ones'
    ratios = R.adam_ratios(p, g, m, v, p_out, m_out, v_out, 2, lr, betas, eps, wd)      # (inf for any mismatch with the fp64 formula)
    _note('kernel', f'kernel inf/nan {hyper}', ratios)
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize('n_steps', [1, 256, 257, 600])
@pytest.mark.parametrize('many_chunks', [False, True])
def test_kernel_step_counters(chunk, many_chunks, n_steps):
    """block 0 walks the counters in strides of its 256 threads - alone (n_chunks == 1) and beside the other blocks' work"""
    lay = layout(chunk) if many_chunks else layout(chunk, only=(5,), shifts=(SHIFTS[0],))      # or one tensor, one chunk
    logical = logical_inputs(lay[2][0].numel(), seed=10)
    lr, betas, eps, wd = HYPERS['default']
    p_out, m_out, v_out = run_kernel(chunk, lay, logical, HYPERS['default'], 3, n_steps=n_steps)      # asserts the counters
    ratios = R.adam_ratios(*logical, p_out, m_out, v_out, 3, lr, betas, eps, wd)
    _note('kernel', f'kernel counters n_steps={n_steps} many_chunks={many_chunks}', ratios)
    assert max(ratios) <= 1.0, ratios


# --------------------------------------------------------------------------------------------------------------- optimizer

SIZES = [(1,), (7,), (4096,), (4097,), (33, 65)]


class Bench:
    """amd.Adam on bare parameters with hand-made gradients; `step` checks everything after every optimizer step"""

    def __init__(self, amd, monkeypatch, sizes=SIZES, groups=None, persistent=True, seed=0, misaligned=2, **adam_kw):
        self.gen = torch.Generator().manual_seed(seed)
        self.persistent = persistent
        self.params = []
        for k, s in enumerate(sizes):
            n = math.prod(s)
            if k == misaligned:                       # a view one element into a larger buffer: 4 bytes off the 16-byte alignment
                buf = torch.zeros(n + 9, device=DEV)
                p = torch.nn.Parameter(buf[1:1 + n].view(s))
                assert p.data_ptr() % 16 == 4 and p.is_contiguous()
            else:
                p = torch.nn.Parameter(torch.zeros(s, device=DEV))
            p.data.copy_(R.param_values(n + k, self.gen)[k:].view(s))      # (from element k on: scalars of every scale)
            self.params.append(p)
        self.t = {p: 0 for p in self.params}
        groups = groups if groups is not None else [dict(params=[0, 1, 2]), dict(params=list(range(3, len(sizes))))]
        self.opt = amd.Adam([dict(g, params=[self.params[i] for i in g['params']]) for g in groups], **adam_kw)
        self.count = {'torch': 0, 'native': 0, 'general': 0}
        L = _mods()[1].load()
        real_fused, real_native = torch._fused_adam_, L.i3d_adam_step
        monkeypatch.setattr(torch, '_fused_adam_', lambda *a, **k: (self._hit('torch'), real_fused(*a, **k))[1])
        monkeypatch.setattr(L, 'i3d_adam_step', lambda *a: (self._hit('native'), real_native(*a))[1])
        self._wrap_general(self.opt)
        self.n = 0

    def _hit(self, what):
        self.count[what] += 1

    def _wrap_general(self, opt):
        real = opt._step_general
        opt._step_general = lambda closure=None: (self._hit('general'), real(closure))[1]

    def add(self, size):
        p = torch.nn.Parameter(R.param_values(math.prod(size), self.gen).view(size).to(DEV))
        self.params.append(p)
        self.t[p] = 0
        return p

    @staticmethod
    def _flat(ts):
        return torch.cat([t.detach().reshape(-1) for t in ts]).cpu()

    def _state(self, opt, ps, key):
        return self._flat([opt.state[p][key] if len(opt.state.get(p, {})) else torch.zeros_like(p) for p in ps])

    def give_gradients(self, without=()):
        for k, p in enumerate(self.params):
            if any(p is q for q in without):
                continue
            g = R.grad_values(p.numel() + k, self.gen, step=self.n)[k:].view(p.shape).to(DEV)
            if self.persistent and p.grad is not None:
                p.grad.copy_(g)
            else:
                p.grad = g

    def step(self, expect, fast=None, closure=None, opt=None, tag=''):
        """one optimizer step on the gradients in place; expect: 'native' or 'torch' - the kernel that must have run, alone"""
        opt = opt or self.opt
        self.n += 1
        pre = []
        for gr in opt.param_groups:
            ps = list(gr['params'])
            act, idle = [p for p in ps if p.grad is not None], [p for p in ps if p.grad is None]
            for p in act:
                self.t[p] += 1
            pre.append((gr, act, idle, [self._flat(act)] + [self._flat([p.grad for p in act])] + [self._state(opt, act, k) for k in ('exp_avg', 'exp_avg_sq')]
                        if act else None, [_bits(self._flat(idle)), _bits(self._state(opt, idle, 'exp_avg')), _bits(self._state(opt, idle, 'exp_avg_sq'))] if idle else None))
        before = dict(self.count)
        out = opt.step(closure) if closure is not None else opt.step()
        ran = {k: self.count[k] - before[k] for k in before}
        for gr, act, idle, a, b in pre:
            if act:
                T = torch.cat([torch.full((p.numel(),), float(self.t[p]), dtype=torch.float64) for p in act])
                ratios = R.adam_ratios(*a, self._flat(act), self._state(opt, act, 'exp_avg'), self._state(opt, act, 'exp_avg_sq'), T,
                                       gr['lr'], gr['betas'], gr['eps'], gr['weight_decay'])
                _note('optimizer', f'{tag} step {self.n} lr {gr["lr"]:g} wd {gr["weight_decay"]:g}', ratios)
                assert max(ratios) <= 1.0, (self.n, ratios)
                assert torch.equal(_bits(self._flat([p.grad for p in act])), _bits(a[1])), 'a gradient changed'
                if gr['lr'] == 0:
                    assert torch.equal(_bits(self._flat(act)), _bits(a[0]))
            if idle:
                after = [_bits(self._flat(idle)), _bits(self._state(opt, idle, 'exp_avg')), _bits(self._state(opt, idle, 'exp_avg_sq'))]
                assert all(torch.equal(x, y) for x, y in zip(after, b)), 'a parameter without gradient was touched'
            for p in act + idle:
                if len(opt.state.get(p, {})):
                    assert float(opt.state[p]['step']) == self.t[p], (self.n, float(opt.state[p]['step']), self.t[p])
                else:
                    assert self.t[p] == 0
        assert (ran['native'] > 0, ran['torch'] > 0) == (expect == 'native', expect == 'torch'), (self.n, expect, ran)
        if expect == 'native':
            assert ran['native'] == 1, 'ONE launch for all parameters'
        if fast is not None and opt is self.opt:
            assert (ran['general'] == 0) == fast, (self.n, 'fast path' if fast else 'general path', ran)
        return out

    def run(self, plan, after_step=None, tag=''):
        """plan: per step 'torch' / 'native' / 'fast' (native straight from `step`, without _step_general)"""
        for e in plan:
            self.give_gradients()
            self.step('native' if e == 'fast' else e, fast=(e == 'fast') if e != 'torch' else None, tag=tag)
            if after_step is not None:
                after_step(self)


def test_optimizer_persistent_gradients_reach_the_fast_path(amd, monkeypatch):
    """1. two groups, equal hyper-parameters, the same gradient tensors every step: native from step 2, straight from `step` from step 3"""
    b = Bench(amd, monkeypatch, lr=1e-3)
    b.run(['torch', 'native', 'fast', 'fast', 'fast', 'fast', 'fast'], after_step=lambda b: b.opt.zero_grad(set_to_none=False), tag='persistent')
    assert b.opt._host_step == 7


def test_optimizer_fresh_gradient_objects_every_step(amd, monkeypatch):
    """2. zero_grad() sets the gradients to None: new gradient objects every step - native through the general path, a new table"""
    b = Bench(amd, monkeypatch, persistent=False, lr=1e-3)
    b.run(['torch'] + ['native'] * 6, after_step=lambda b: b.opt.zero_grad(), tag='fresh')
    assert b.count['general'] == 7


def test_optimizer_lr_schedule(amd, monkeypatch):
    """3. the warm-up scheduler's pattern: another lr in front of every step, one of them 0 (asserted inside: parameters bit-identical)"""
    b = Bench(amd, monkeypatch, lr=1e-3)
    for k, lr in enumerate([1e-5, 2e-5, 0.0, 4e-5, 8e-5, 8e-5, 3e-3]):
        for gr in b.opt.param_groups:
            gr['lr'] = lr
        b.give_gradients()
        b.step('torch' if k == 0 else 'native', fast=(k == 5), tag='lr schedule')


def test_optimizer_uniform_weight_decay(amd, monkeypatch):
    """4. weight decay 1e-2 in both groups: native"""
    b = Bench(amd, monkeypatch, lr=1e-3, weight_decay=1e-2)
    b.run(['torch', 'native', 'fast', 'fast', 'fast', 'fast'], tag='uniform wd')


def test_optimizer_groups_with_different_weight_decay(amd, monkeypatch):
    """5. weight decay 0 and 1e-2: torch's kernel per group on every step, never ours; the counters advance by exactly one"""
    b = Bench(amd, monkeypatch, groups=[dict(params=[0, 1, 2], weight_decay=0), dict(params=[3, 4], weight_decay=1e-2)], lr=1e-3)
    b.run(['torch'] * 6, tag='mixed wd')
    assert b.count['native'] == 0


def test_optimizer_first_gradient_at_step_four(amd, monkeypatch):
    """6. a parameter without gradient for three steps: its bias corrections start at t = 1 when the others are at 4, and no native
    launch is made while the counters differ"""
    b = Bench(amd, monkeypatch, lr=1e-3)
    late = b.params[3]
    for e in ['torch', 'native', 'fast']:
        b.give_gradients(without=(late,))
        b.step('native' if e == 'fast' else e, fast=(e == 'fast'), tag='late first gradient')
    assert b.t[late] == 0
    b.run(['torch'] * 5, tag='late first gradient')
    assert b.t[late] == 5 and b.t[b.params[0]] == 8


@pytest.mark.parametrize('persistent', [True, False])
def test_optimizer_gradient_missing_for_one_step(amd, monkeypatch, persistent):
    """7. one parameter's .grad is None at step 4 and THE SAME tensor object comes back at step 5: torch skips the parameter at step 4
    (untouched), its step count is one behind from then on - per-parameter bias corrections, so torch's kernel and no native launch.
    With the host count that survived torch's step (optim.py before `_torch_step`) the persistent case launched natively at step 5 with
    the bias corrections of step 4: param error / allowance 3.4e4, observed on the MI355X."""
    b = Bench(amd, monkeypatch, persistent=persistent, lr=1e-3)
    b.run(['torch', 'native', 'fast' if persistent else 'native'], tag='grad None once')
    gone = b.params[1]
    kept, gone.grad = gone.grad, None
    b.give_gradients(without=(gone,))
    b.step('torch', tag='grad None once')
    gone.grad = kept
    b.run(['torch'] * 4, tag='grad None once')
    assert b.t[gone] == 7 and b.t[b.params[0]] == 8


@pytest.mark.parametrize('persistent', [True, False])
def test_optimizer_closure_step_between_plain_steps(amd, monkeypatch, persistent):
    """8. step(closure) at step 4 is torch's step: the host's step count must not survive it - steps 5.. are native again, at t = 5..
    (with the surviving count: t = 4 at step 5, param error / allowance 3.3e4 with persistent and with fresh gradients, observed)"""
    b = Bench(amd, monkeypatch, persistent=persistent, lr=1e-3)
    b.run(['torch', 'native', 'fast' if persistent else 'native'], tag='closure')
    b.give_gradients()
    calls = []
    assert b.step('torch', closure=lambda: (calls.append(torch.is_grad_enabled()), torch.tensor(1.5))[1], tag='closure').item() == 1.5
    assert calls == [True]
    b.run(['native'] + ['fast' if persistent else 'native'] * 3, tag='closure')
    assert b.opt._host_step == 8


def test_optimizer_add_param_group_after_three_steps(amd, monkeypatch):
    """9. the new group's parameter starts at t = 1 beside t = 4: torch's kernel from then on"""
    b = Bench(amd, monkeypatch, lr=1e-3)
    b.run(['torch', 'native', 'fast'], tag='add_param_group')
    b.opt.add_param_group(dict(params=[b.add((130,))]))
    b.run(['torch'] * 4, tag='add_param_group')
    assert b.t[b.params[-1]] == 4 and b.t[b.params[0]] == 7


def test_optimizer_state_dict_round_trip(amd, monkeypatch):
    """10. state_dict() after four steps, three of them native: the counters read 4; it loads into torch.optim.Adam and into a fresh
    amd.Adam, and both continue for two steps inside the allowances (t = 5, 6)"""
    b = Bench(amd, monkeypatch, lr=1e-3)
    b.run(['torch', 'native', 'fast', 'fast'], tag='state_dict')
    sd = b.opt.state_dict()
    assert [float(s['step']) for s in sd['state'].values()] == [4.0] * len(b.params)
    assert all(s['step'].dtype == torch.float32 for s in sd['state'].values())
    origin, t4 = list(b.params), dict(b.t)
    for cls, kw, plan in ((torch.optim.Adam, dict(fused=True), ['torch', 'torch']), (amd.Adam, {}, ['torch', 'native'])):
        clones = [torch.nn.Parameter(p.detach().clone()) for p in origin]
        opt = cls([dict(params=clones[:3]), dict(params=clones[3:])], lr=1e-3, **kw)
        opt.load_state_dict(copy.deepcopy(sd))                        # (torch shares the tensors of a state_dict it loads)
        b.params, b.t = clones, {c: t4[p] for c, p in zip(clones, origin)}
        for e in plan:
            b.give_gradients()
            b.step(e, opt=opt, tag=f'state_dict -> {cls.__module__}')
        assert [float(opt.state[c]['step']) for c in clones] == [6.0] * len(clones)


def test_optimizer_parameter_storage_replaced(amd, monkeypatch):
    """11. p.data = a copy elsewhere in memory after step 3: step 4 updates the new storage, natively, and never the old one"""
    b = Bench(amd, monkeypatch, lr=1e-3)
    b.run(['torch', 'native', 'fast'], tag='storage replaced')
    p = b.params[4]
    old = p.data
    p.data = old.clone()
    assert p.data_ptr() != old.data_ptr()
    old_bits = _bits(old).clone()
    b.run(['native', 'fast', 'fast'], tag='storage replaced')
    assert torch.equal(_bits(old), old_bits), 'the old storage was written'
    assert not torch.equal(p.data, old)


def test_optimizer_three_hundred_scalar_parameters(amd, monkeypatch):
    """12. more step counters than block 0 has threads; scalars of shape () and (1,)"""
    sizes = [() if k % 2 else (1,) for k in range(300)]
    b = Bench(amd, monkeypatch, sizes=sizes, groups=[dict(params=list(range(100))), dict(params=list(range(100, 300)))], misaligned=-1, lr=1e-3)
    b.run(['torch', 'native', 'fast', 'fast', 'fast', 'fast'], tag='300 scalars')
    assert b.opt._steps_flat.numel() == 300 and b.opt._native.n_chunks == 300
