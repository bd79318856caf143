"""The planner of a PNA layer's buffers (include/infomax3d_hip.h: i3d_pna_layer_place_fwd / _bwd) through the ctypes binding, on
fake base addresses that nothing dereferences, and the whole-model sizes that stand on it.  No GPU is needed: placement is
pointer arithmetic on the host."""
import ctypes
import importlib
import itertools

import pytest

importlib.import_module('3dinfomax_amd.build').build(verbose=False)
L = importlib.import_module('3dinfomax_amd._lib')
lib = L.load()

N, E, Q_ROWS, V_PAD, N_GROUPS, N_AGG = 5, 7, 3, 32, 2, 4
F_H, F_Q = 28, 24                       # neither is a block width: a buffer sized by the wrong one shows
WIDTHS = (8, 12, 16, 20, 4)             # the blocks' output widths in forward order: all different up to five blocks, and no two
#                                         neighbours alike in the layers of six and seven
FWD_BASE, CHAIN_BASE, SIDE_BASE = 0x10000000, 0x30000000, 0x50000000
RELU, SILU = L.ACT['relu'], L.ACT['silu']


def _leaves(obj, prefix=''):
    """{'edge.tail.mean': value, 'pre[1].x': value, 'aff[2]': value, ...} of every scalar and pointer member"""
    out = {}
    for name, _ in obj._fields_:
        v = getattr(obj, name)
        items = [(f'{prefix}{name}', v)] if not isinstance(v, ctypes.Array) else [(f'{prefix}{name}[{i}]', x) for i, x in enumerate(v)]
        for path, x in items:
            if isinstance(x, ctypes.Structure):
                out.update(_leaves(x, path + '.'))
            else:
                out[path] = x
    return out


def _fill_pointers(obj, counter):
    """a distinct non-null sentinel in every pointer member: what the planner must set to NULL or leave alone starts non-null"""
    for name, t in obj._fields_:
        v = getattr(obj, name)
        if t is ctypes.c_void_p:
            setattr(obj, name, 0x7000000 + 16 * next(counter))
        elif isinstance(v, ctypes.Structure):
            _fill_pointers(v, counter)
        elif isinstance(v, ctypes.Array):
            for i, x in enumerate(v):
                if isinstance(x, ctypes.Structure):
                    _fill_pointers(x, counter)
                elif v._type_ is ctypes.c_void_p:
                    v[i] = 0x7000000 + 16 * next(counter)


def describe(fused, merge, n_pre_extra, n_post_extra, q, act):
    a = L.PnaLayerArgs()
    _fill_pointers(a, itertools.count())
    widths = itertools.cycle(WIDTHS)
    a.fused_bn, a.merge_h, a.n_pre_extra, a.n_post_extra, a.n_aggregators = fused, merge, n_pre_extra, n_post_extra, N_AGG
    for t in [a.edge.tail, a.post.tail] + [blocks[i].tail for blocks in (a.pre, a.postx) for i in range(3)]:
        t.act, t.post_act = act, L.ACT[None]
    e = a.edge
    e.num_nodes, e.num_edges, e.f_h, e.f_out, e.ldw = N, E, F_H, next(widths), 2 * F_H + F_Q
    e.f_q, e.q_rows, e.v_pad = (0, 0, 0) if q == 'absent' else (F_Q, 0, 0) if q == 'dense' else (F_Q, Q_ROWS, V_PAD)
    if q == 'absent':
        e.q = None
    f = e.f_out
    for c in (a.pre[i] for i in range(n_pre_extra)):
        c.rows, c.f_in, c.f_out, c.ldw = E, f, next(widths), f
        f = c.f_out
    p = a.post
    p.num_nodes, p.f_h, p.f_out, p.agg_width, p.n_groups, p.n_scalers, p.m_padded = N, F_H, next(widths), N_AGG * f, N_GROUPS, 3, 128
    p.ldw = F_H + 3 * p.agg_width
    f = p.f_out
    for c in (a.postx[i] for i in range(n_post_extra)):
        c.rows, c.f_in, c.f_out, c.ldw = N, f, next(widths), f
        f = c.f_out
    return a


def expected_forward(a):
    """{member: floats, or None for a buffer this description does not have} - the sizes of the header's member comments"""
    e, p = a.edge, a.post
    fused, merged, keeps = bool(a.fused_bn), bool(a.merge_h), a.edge.tail.act == SILU
    Fo0, WL = e.f_out, 2 * e.f_out + p.f_out
    panel = lambda n, k: lib.i3d_panel_packed_bytes(n, k) // 4 if merged else None      # noqa: E731
    x = {'edge.tail.mean': Fo0, 'edge.tail.invstd': Fo0, 'edge.P': N * 2 * Fo0,
         'edge.Q': None if not e.f_q else (e.q_rows or E) * Fo0,
         'edge.xact': E * Fo0, 'edge.pre_keep': E * Fo0 if keeps else None, 'edge.y': None if fused else E * Fo0,
         'aff[0]': 3 * Fo0 if fused else None,
         'Wcat': WL * F_H if merged else None, 'bcat': WL if merged else None, 'PL': N * WL if merged else None,
         'Wcat_panel': panel(WL, F_H), 'Wcat_dgrad_panel': panel(F_H, WL)}
    for i in range(3):
        c = a.pre[i]
        if i < a.n_pre_extra:
            x.update({f'pre[{i}].tail.mean': c.f_out, f'pre[{i}].tail.invstd': c.f_out, f'pre[{i}].xact': E * c.f_out,
                      f'pre[{i}].pre_keep': E * c.f_out if keeps else None, f'pre[{i}].y': None if fused else E * c.f_out,
                      f'aff[{i + 1}]': 3 * c.f_out if fused else None,
                      f'pre[{i}].W_dgrad_panel': panel(c.f_in, c.f_out), f'pre[{i}].W_fwd_panel': panel(c.f_out, c.f_in)})
        else:
            x[f'aff[{i + 1}]'] = None
    x.update({'post.tail.mean': p.f_out, 'post.tail.invstd': p.f_out, 'post.agg': N * p.agg_width,
              'post.WD': N_GROUPS * p.f_out * p.agg_width, 'post.xact': N * p.f_out, 'post.pre_keep': N * p.f_out if keeps else None})
    if a.n_post_extra:
        x['post.y'] = N * p.f_out
    for i in range(a.n_post_extra):
        c = a.postx[i]
        x.update({f'postx[{i}].tail.mean': c.f_out, f'postx[{i}].tail.invstd': c.f_out, f'postx[{i}].xact': N * c.f_out,
                  f'postx[{i}].pre_keep': N * c.f_out if keeps else None})
        if i < a.n_post_extra - 1:
            x[f'postx[{i}].y'] = N * c.f_out
    return x


def expected_backward(a):
    """{member: (region, floats) or None}"""
    e, p = a.edge, a.post
    merged, table = bool(a.merge_h), e.q_rows > 0
    f_msg = p.agg_width // N_AGG
    x = {'post.grad_pre': ('side', N * p.f_out), 'post.grad_WD': ('side', N_GROUPS * p.f_out * p.agg_width),
         'post.grad_agg': ('chain', N * p.agg_width), 'grad_msg': ('chain', E * f_msg),
         'edge.grad_pre': ('side', E * e.f_out), 'edge.grad_P': ('side', N * 2 * e.f_out), 'edge.grad_h': ('chain', N * F_H),
         'edge.grad_Q': ('side', V_PAD * e.f_out) if table else None,
         'DL': ('side', N * (2 * e.f_out + p.f_out)) if merged else None,
         'edge_bias_partial': ('side', lib.i3d_bn_bias_partial_floats(e.f_out)) if merged else None}
    for name, blocks, n in (('pre', a.pre, a.n_pre_extra), ('postx', a.postx, a.n_post_extra)):
        for i in range(n):
            c = blocks[i]
            x[f'{name}[{i}].grad_pre'] = ('side', c.rows * c.f_out)
            x[f'{name}[{i}].grad_x'] = ('chain', c.rows * c.f_in)
    return x


def check_placed(after, expected, regions):
    """inside its region, on a 16-byte boundary, no two overlapping at their sizes; NULL where the description has no such buffer"""
    spans = []
    for path, want in expected.items():
        if want is None:
            assert after[path] is None, f'{path} must be NULL'
            continue
        region, floats = want if isinstance(want, tuple) else ('fwd', want)
        base, count = regions[region]
        p = after[path]
        assert p is not None and p % 16 == 0 and base <= p and p + 4 * floats <= base + 4 * count, (path, p, floats)
        spans.append((p, p + 4 * floats, path))
    spans.sort()
    for (_, end, one), (start, _, two) in zip(spans, spans[1:]):
        assert end <= start, f'{one} overlaps {two}'


def check_untouched(before, after, written):
    changed = {k for k in before if before[k] != after[k]} - set(written)
    assert not changed, f'the planner wrote {sorted(changed)}'


CASES = [c for c in itertools.product((0, 1), (0, 1), (0, 1, 3), (0, 2), ('absent', 'dense', 'table'), (RELU, SILU))
         if not (c[1] and not (c[0] and c[3] == 0))]      # merge_h only with fused_bn and one posttrans block


@pytest.mark.parametrize('fused,merge,n_pre_extra,n_post_extra,q,act', CASES)
def test_layer_placement(fused, merge, n_pre_extra, n_post_extra, q, act):
    a = describe(fused, merge, n_pre_extra, n_post_extra, q, act)
    ref = ctypes.byref(a)
    n_chain, n_side = ctypes.c_long(-7), ctypes.c_long(-7)
    if fused and n_post_extra:      # the fused-BatchNorm form has one posttrans block (I3dPnaLayerArgs.fused_bn): no such layer
        assert lib.i3d_pna_layer_place_fwd(ref, FWD_BASE) < 0 and lib.i3d_pna_layer_place_fwd(ref, None) < 0
        assert lib.i3d_pna_layer_place_bwd(ref, CHAIN_BASE, SIDE_BASE, ctypes.byref(n_chain), ctypes.byref(n_side)) < 0
        assert (n_chain.value, n_side.value) == (0, 0)
        return
    before = _leaves(a)
    # ---- forward
    n_saved = lib.i3d_pna_layer_place_fwd(ref, None)
    assert n_saved > 0 and lib.i3d_pna_layer_place_fwd(ref, FWD_BASE) == n_saved
    after = _leaves(a)
    want = expected_forward(a)
    check_placed(after, want, {'fwd': (FWD_BASE, n_saved)})
    last_pre = f'pre[{n_pre_extra - 1}]' if n_pre_extra else 'edge'
    out_of = lambda block: after[block + ('.xact' if fused else '.y')]      # noqa: E731
    chain = {'msg': out_of(last_pre)}
    for i in range(n_pre_extra):
        chain[f'pre[{i}].x'] = out_of(f'pre[{i - 1}]' if i else 'edge')
    for i in range(n_post_extra):
        chain[f'postx[{i}].x'] = after[f'postx[{i - 1}].y' if i else 'post.y']
    for path, value in chain.items():
        assert after[path] == value is not None, path
    # the posttrans chain ends in the caller's output (and every other member of the caller's is as it was)
    last_post = f'postx[{n_post_extra - 1}]' if n_post_extra else 'post'
    assert after[last_post + '.y'] == before[last_post + '.y']
    check_untouched(before, after, list(want) + list(chain))
    # ---- backward
    before = after
    assert lib.i3d_pna_layer_place_bwd(ref, None, None, ctypes.byref(n_chain), ctypes.byref(n_side)) == 0
    sized = (n_chain.value, n_side.value)
    assert lib.i3d_pna_layer_place_bwd(ref, CHAIN_BASE, SIDE_BASE, ctypes.byref(n_chain), ctypes.byref(n_side)) == 0
    assert sized == (n_chain.value, n_side.value) and min(sized) > 0
    after = _leaves(a)
    want = expected_backward(a)
    check_placed(after, want, {'chain': (CHAIN_BASE, sized[0]), 'side': (SIDE_BASE, sized[1])})
    # each block's grad_y is the grad_x of the block behind it (the messages' gradient for the last pretrans block), the top one grad_out
    order = ['edge'] + [f'pre[{i}]' for i in range(n_pre_extra)] + ['post'] + [f'postx[{i}]' for i in range(n_post_extra)]
    chain = {}
    for block, behind in zip(order, order[1:] + [None]):
        chain[block + '.grad_y'] = after['grad_out'] if behind is None else after['grad_msg'] if behind == 'post' else after[behind + '.grad_x']
    for path, value in chain.items():
        assert after[path] == value is not None, path
    assert after['grad_out'] == before['grad_out']
    check_untouched(before, after, list(want) + list(chain))


def _pinned_model():
    P = 0x7000000        # any non-null address: sizing dereferences nothing
    m, b = L.PnaModel(), L.PnaBatch()
    m.training, m.n_layers, m.hidden, m.n_pre, m.residual = 1, 2, 200, 1, 1
    m.n_aggregators, m.n_scalers, m.avg_d_log = 4, 3, 1.0
    for i, k in enumerate(('mean', 'max', 'min', 'std')):
        m.aggregators[i] = L.AGG[k]
    for i, k in enumerate(('identity', 'amplification', 'attenuation')):
        m.scalers[i] = L.SCALER[k]
    for layer in range(2):
        for fc, f_in, act in ((m.pre[layer][0], 600, RELU), (m.post[layer], 2600, L.ACT[None])):
            fc.f_in, fc.f_out, fc.act, fc.gamma, fc.eps, fc.momentum = f_in, 200, act, P, 1e-5, 0.1
    m.n_atom_tables, m.n_bond_tables, m.n_readout, m.n_head = 1, 1, 2, 1
    m.atom_dims[0], m.bond_dims[0] = 10, 5
    m.readout_ops[0], m.readout_ops[1] = L.AGG['mean'], L.AGG['sum']
    m.head[0].f_in, m.head[0].f_out, m.head[0].act = 400, 256, L.ACT[None]
    b.num_nodes, b.num_edges, b.num_graphs, b.n_comb, b.v_pad, b.m_padded, b.n_groups = 1000, 2100, 50, 5, 32, 1152, 3
    for g, (degree, start, count) in enumerate(((1, 0, 300), (2, 320, 400), (3, 768, 300))):
        b.group_degree[g], b.group_start[g], b.group_count[g] = degree, start, count
    return m, b


def test_model_sizes_of_a_pinned_description():
    m, b = _pinned_model()
    assert lib.i3d_pna_model_saved_floats(ctypes.byref(m), ctypes.byref(b)) == 7406780
    # 8 889 336 was the hand-kept upper bound that charged every layer's side buffers twice; the planned size is exact
    assert 0 < lib.i3d_pna_model_scratch_floats(ctypes.byref(m), ctypes.byref(b)) <= 8889336
