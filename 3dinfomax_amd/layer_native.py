"""One PNA layer through the native layer composite (csrc/composite.hip: i3d_pna_layer_fwd / i3d_pna_layer_bwd).

pna.PNALayerFn runs a layer as four block Functions back to back from Python (~20 us of Python and 5-7 allocations per
block and direction).  Here the whole layer is ONE C call per direction: Python describes the layer in one argument struct
(sizes, parameters, flags), the library's planner sizes one buffer and places the layer's saved and scratch tensors in it,
chained block to block (csrc/composite.hip: i3d_pna_layer_place_fwd / _bwd - the same planner the whole-model sequencer
uses), and Python allocates that buffer and what autograd hands out (the layer output, dL/dh, dL/dq and the parameter
gradients).  Same kernels, same order, same bits as the block path - it is eligible when every block is a BatchNorm block
in training mode with local statistics (the pre-training configuration) and the posttrans is degree-grouped; anything else
stays on the block path.
"""
import ctypes

import torch

from . import _lib, ops, tape
from . import layers as _layers
from .layers import _set_workspaces

_SIMPLE_ACTS = (None, 'relu', 'leakyrelu')
# the in-degree groups / (group, scaler) coefficients that the per-degree tables of I3dGroupedFcArgs hold
_MAX_GROUPS, _MAX_COEF = _lib.array_len(_lib.GroupedFcArgs, 'group_start'), _lib.array_len(_lib.GroupedFcArgs, 'coef')
KEEP_LAST_ARGS = None


def fused_bn_ok(plan, params, n_pre, n_post):
    """Can the layer take the fused-BatchNorm form (statistics in the producers' epilogues, BatchNorm-apply in the consumers'
    loads: csrc/fused_bn.hip)?  Otherwise: a statistics pass + an apply pass per block.  Same arithmetic up to summation order."""
    if n_post != 1:
        return False
    for spec in plan.pre_specs + plan.post_specs[:1]:
        if spec.act not in _SIMPLE_ACTS:
            return False
    for spec in plan.pre_specs:
        if spec.post_act is not None:
            return False
    for i in range(1, n_pre):          # BatchNorm prologue of the GEMM: K <= 1024
        if params[4 * i].shape[1] > 1024:
            return False
    return True


def _al(n):
    return (n + 3) & ~3


class _Arena:
    """bump allocator over one float32 tensor: take(n) -> device pointer (16-byte aligned)"""

    def __init__(self, nfloats, device):
        self.buf = torch.empty(nfloats, dtype=torch.float32, device=device)
        self.base = self.buf.data_ptr()
        self.cap = nfloats
        self.used = 0

    def take(self, n):
        p = self.base + 4 * self.used
        self.used += _al(n)
        assert self.used <= self.cap
        return p


def eligible(h, q, index, qmap, plan, params):
    if not (plan.grouped and h.is_cuda and index.num_edges > 0):
        return False
    n_pre, n_post = len(plan.pre_specs), len(plan.post_specs)
    if n_pre - 1 > 3 or n_post - 1 > 3 or h.shape[1] % 4:
        return False
    for spec in plan.pre_specs + plan.post_specs:
        if not _layers._composite_ok(spec, h):
            return False
    for i in range(n_pre + n_post):
        W = params[4 * i]
        if not W.is_contiguous() or W.shape[0] % 4 or W.shape[1] % 4:
            return False
    groups = index.degree_groups()[2]
    if len(groups) > _MAX_GROUPS or len(groups) * len(plan.coef[0]) > _MAX_COEF:
        return False
    if q is not None and (not q.is_contiguous() or (qmap is not None and q.shape[0] != qmap.rows)):
        return False
    return True


def _tail(tail, spec, gamma, beta, mean_ptr, invstd_ptr, feat, device):
    bn = spec.bn
    tail.act, tail.post_act = ops.ACT[spec.act], ops.ACT[spec.post_act]
    tail.eps, tail.momentum = bn.eps, bn.momentum
    tail.gamma, tail.beta = gamma.data_ptr(), beta.data_ptr()
    tail.running_mean, tail.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
    tail.mean, tail.invstd = mean_ptr, invstd_ptr
    nbt = bn.num_batches_tracked           # bumped by the statistics kernel
    tail.num_batches_tracked = nbt.data_ptr() if nbt is not None else None
    _set_workspaces(tail, feat, device)


def _fc(c, rows, f_in, W, b, ga, be, spec, dev):
    """describes a plain block; -> its output width"""
    Fo = W.shape[0]
    _tail(c.tail, spec, ga, be, None, None, Fo, dev)
    c.rows, c.f_in, c.f_out, c.ldw = rows, f_in, Fo, W.stride(0)
    c.W, c.bias = W.data_ptr(), b.data_ptr()
    return Fo


def forward(ctx, h, q, index, qmap, plan, params):
    h = h.contiguous()
    dev = h.device
    N, Fh = h.shape
    E = index.num_edges
    n_pre, n_post = len(plan.pre_specs), len(plan.post_specs)
    pre_p = [params[4 * i:4 * i + 4] for i in range(n_pre)]
    post_p = [params[4 * (n_pre + i):4 * (n_pre + i) + 4] for i in range(n_post)]
    rows_d, tiles_d, groups = index.degree_groups()
    L = _lib.load()
    y_out = torch.empty(N, post_p[-1][0].shape[0], dtype=torch.float32, device=dev)

    # ---- describe the layer: sizes, parameters, tails, flags, the caller's tensors
    a = _lib.PnaLayerArgs()
    a.fused_bn = int(fused_bn_ok(plan, params, n_pre, n_post))
    # the products that read h as one GEMM per direction (include/infomax3d_hip.h: I3dPnaLayerArgs.merge_h)
    a.merge_h = int(a.fused_bn and post_p[0][0].shape[0] % 4 == 0)
    e = a.edge
    W, b, ga, be = pre_p[0]
    Fo0 = W.shape[0]
    _tail(e.tail, plan.pre_specs[0], ga, be, None, None, Fo0, dev)
    e.num_nodes, e.num_edges, e.f_h, e.f_out, e.ldw = N, E, Fh, Fo0, W.stride(0)
    e.h, e.W, e.bias = h.data_ptr(), W.data_ptr(), b.data_ptr()
    if q is not None:
        e.q, e.f_q = q.data_ptr(), q.shape[1]
        if qmap is not None:
            e.q_rows, e.v_pad, e.q_code, e.onehot = qmap.rows, qmap.v_pad, qmap.codes.data_ptr(), qmap.onehot.data_ptr()
    e.src_s, e.dst_s, e.in_ptr = index.src_s.data_ptr(), index.dst_s.data_ptr(), index.in_ptr.data_ptr()
    e.out_ptr, e.out_epos = index.out_ptr.data_ptr(), index.out_epos.data_ptr()
    a.n_pre_extra = n_pre - 1
    f_max = Fmsg = Fo0
    for i in range(1, n_pre):
        Fmsg = _fc(a.pre[i - 1], E, Fmsg, *pre_p[i], plan.pre_specs[i], dev)
        f_max = max(f_max, Fmsg)
    a.n_aggregators, a.n_scalers, a.force_scalers, a.avg_d_log = len(plan.aggregators), len(plan.agg_scalers), 0, plan.avg
    for i, v in enumerate(plan.aggregators):
        a.aggregators[i] = v
    for i, v in enumerate(plan.agg_scalers):
        a.scalers[i] = v
    p = a.post          # degree-grouped
    W, b, ga, be = post_p[0]
    Fp0 = W.shape[0]
    _tail(p.tail, plan.post_specs[0], ga, be, None, None, Fp0, dev)
    p.num_nodes, p.f_h, p.f_out, p.agg_width, p.ldw = N, Fh, Fp0, len(plan.aggregators) * Fmsg, W.stride(0)
    p.n_groups, p.n_scalers, p.m_padded = len(groups), len(plan.coef[0]), rows_d.shape[0]
    for gi, (_, start, count) in enumerate(groups):
        p.group_start[gi], p.group_count[gi] = start, count
    for k, v in enumerate(c_ for g_ in plan.coef for c_ in g_):
        p.coef[k] = v
    p.h, p.W, p.bias = h.data_ptr(), W.data_ptr(), b.data_ptr()
    p.deg_rows, p.deg_tile_group = rows_d.data_ptr(), tiles_d.data_ptr()
    a.n_post_extra = n_post - 1
    f_in = Fp0
    for i in range(1, n_post):
        f_in = _fc(a.postx[i - 1], N, f_in, *post_p[i], plan.post_specs[i], dev)
    last = a.postx[n_post - 2] if n_post > 1 else p        # its y is the layer output
    last.y = y_out.data_ptr()
    a.residual = 1 if plan.residual else 0
    if plan.residual:
        last.residual = h.data_ptr()

    # ---- size, allocate once, place (csrc/composite.hip: i3d_pna_layer_place_fwd); the statistics scratch rides at the end
    n_saved = L.i3d_pna_layer_place_fwd(ctypes.byref(a), None)
    if n_saved < 0:
        _lib.check(n_saved, 'i3d_pna_layer_place_fwd')
    n_stats = int(L.i3d_pna_layer_stats_floats(N, E, rows_d.shape[0], max(f_max, Fp0))) if a.fused_bn else 0
    ar = _Arena(n_saved + n_stats, dev)
    L.i3d_pna_layer_place_fwd(ctypes.byref(a), ar.take(n_saved))      # (the sizing call has accepted this description)
    if a.fused_bn:
        a.stats_ws = ar.take(n_stats)
    if ops.KERNEL_TIMERS is not None:   # bench.py: HIP events on the launch stream around the roofline kernel
        t0, t1 = ops.RawEvent(), ops.RawEvent()
        a.agg_event_start, a.agg_event_stop = t0.handle, t1.handle
        ops.KERNEL_TIMERS.setdefault('pna_aggregate_fwd', []).append(
            (t0, t1, N, E, Fmsg, len(plan.aggregators) * len(plan.agg_scalers) * Fmsg))
    _lib.check(L.i3d_pna_layer_fwd(ctypes.byref(a), ops._stream()), 'i3d_pna_layer_fwd')
    a.agg_event_start = a.agg_event_stop = None
    ctx.native = (a, ar, h, q, qmap, index, plan, params)
    if KEEP_LAST_ARGS is not None:      # tools/launch_floor.py: replay the C call without the Python around it
        KEEP_LAST_ARGS.append((a, ctx.native))
    return y_out


def backward(ctx, grad):
    a, ar_fwd, h, q, qmap, index, plan, params = ctx.native
    dev = h.device
    grad = grad.contiguous()
    blocks = [a.edge] + [a.pre[i] for i in range(a.n_pre_extra)] + [a.post] + [a.postx[i] for i in range(a.n_post_extra)]
    grads = []          # (gW, gbias, ggamma, gbeta) per block, forward order: the model's persistent gradient buffers when it has them
    for k, c in enumerate(blocks):
        _set_workspaces(c.tail, c.f_out, dev)      # per thread and stream: autograd's thread here
        g4 = tuple(tape.grad_like(params[4 * k + j]) for j in range(4))
        c.grad_W, c.grad_bias, c.grad_gamma, c.grad_beta = (t.data_ptr() for t in g4)
        grads.extend(g4)
    gh = torch.empty_like(h)
    gq = torch.empty_like(q) if (q is not None and ctx.needs_input_grad[1]) else None
    a.grad_out, a.post.grad_h = grad.data_ptr(), gh.data_ptr()
    a.edge.grad_q = gq.data_ptr() if gq is not None else None
    # ---- size, allocate once, place (i3d_pna_layer_place_bwd): the chain's buffers, then the weight-gradient stream's
    L = _lib.load()
    n_chain, n_side = ctypes.c_long(), ctypes.c_long()
    _lib.check(L.i3d_pna_layer_place_bwd(ctypes.byref(a), None, None, ctypes.byref(n_chain), ctypes.byref(n_side)), 'i3d_pna_layer_place_bwd')
    ar = _Arena(n_chain.value + n_side.value, dev)
    # (accepted by the sizing call: no second check of the return)
    L.i3d_pna_layer_place_bwd(ctypes.byref(a), ar.take(n_chain.value), ar.take(n_side.value), ctypes.byref(n_chain), ctypes.byref(n_side))
    _lib.check(L.i3d_pna_layer_bwd(ctypes.byref(a), ops._stream()), 'i3d_pna_layer_bwd')
    return (gh, gq, None, None, None) + tuple(grads)
