"""Tensor-level wrappers over the C ABI (include/infomax3d_hip.h).

torch is plumbing here: it owns device memory (caching allocator) and the current HIP stream; every
computation below is one of the hand-written gfx950 kernels in csrc/.  No autograd in this file - the
autograd.Functions in layers.py / pna.py / net3d.py / losses.py chain these calls explicitly.
"""
import ctypes
import os
import threading

import torch

from . import _lib
from ._lib import ACT, AGG, SCALER, check, int_array, ptr_array

_tls = threading.local()
KERNEL_TIMERS = None      # set to a dict by bench.py to collect (start, end) HIP events of the roofline kernel


# The wrappers below are on the host's critical path (~210 calls per training step): pointers and the stream are
# passed to ctypes as plain ints (argtypes are c_void_p), the raw current stream comes from one C call.
_raw_stream = torch._C._cuda_getCurrentRawStream


def _stream():
    return _raw_stream(torch.cuda.current_device())


def _p(t):
    return t.data_ptr() if t is not None else None


def _chk(t, dtype=torch.float32):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise AssertionError(f'expected a contiguous {dtype} HIP tensor, got {t.device} {t.dtype} '
                             f'contiguous={t.is_contiguous()} (there is no CPU fallback)')
    return t


_ws_need = {}


def _workspace(feat, device):
    """Thread-local scratch for the two-stage column reductions (stream-ordered reuse), one per stream (the raw stream
    handle is the key: torch.cuda.current_stream() builds a Python object, ~10 us, and this runs ~60 times per step)."""
    need = _ws_need.get(feat)
    if need is None:
        need = _ws_need[feat] = _lib.load().i3d_colreduce_workspace_bytes(0, feat)
    key = (device.index, _raw_stream(device.index))
    ws = getattr(_tls, 'ws', None)
    if ws is None:
        ws = _tls.ws = {}
    buf = ws.get(key)
    if buf is None or buf.numel() < need:
        # zero-initialised: the arrival counters of the in-kernel finalisation live at its head (include/infomax3d_hip.h)
        buf = ws[key] = torch.zeros(max(need, 1 << 22), dtype=torch.uint8, device=device)
    return buf


def _gemm_workspace(device):
    """Thread-local scratch of the weight-gradient GEMMs (split-K / row-segment slices, include/infomax3d_hip.h
    i3d_gemm_f32_ws), one per stream."""
    key = (device.index, _raw_stream(device.index))
    ws = getattr(_tls, 'gws', None)
    if ws is None:
        ws = _tls.gws = {}
    buf = ws.get(key)
    if buf is None:
        buf = ws[key] = torch.empty(max(GEMM_WORKSPACE_BYTES, 16), dtype=torch.uint8, device=device)
    return buf


# I3D_GEMM_SCRATCH=0: fp32 atomics on top of a zero-fill instead of the two-stage reduction (A/B switch)
GEMM_WORKSPACE_BYTES = (160 << 20) if os.environ.get('I3D_GEMM_SCRATCH', '1') != '0' else 0


class RawEvent:
    """hipEvent_t created through the C ABI (for measurements around a kernel that a composite launches)"""

    def __init__(self):
        h = ctypes.c_void_p()
        check(_lib.load().i3d_event_create(ctypes.byref(h)), 'i3d_event_create')
        self.handle = h.value

    def record(self):
        """on the current stream"""
        check(_lib.load().i3d_event_record(self.handle, _stream()), 'i3d_event_record')

    def elapsed_time(self, stop):
        ms = ctypes.c_float()
        check(_lib.load().i3d_event_elapsed_ms(self.handle, stop.handle, ctypes.byref(ms)), 'i3d_event_elapsed_ms')
        return ms.value

    def __del__(self):
        try:
            _lib.load().i3d_event_destroy(self.handle)
        except Exception:
            pass


def agg_codes(names):
    return [AGG[n] for n in names]


def scaler_codes(names):
    return [SCALER[n] for n in names]


# ---- K1 --------------------------------------------------------------------------------------------------
def embedding_sum_fwd(idx, tables, row_perm=None):
    _chk(idx, torch.int64)
    rows, n_cols = idx.shape
    feat = tables[0].shape[1]
    out = torch.empty(rows, feat, dtype=torch.float32, device=idx.device)
    L = _lib.load()
    check(L.i3d_embedding_sum_fwd(_p(idx), _p(row_perm), rows, n_cols, ptr_array([_chk(t).data_ptr() for t in tables]), feat,
                                  _p(out), _stream()), 'i3d_embedding_sum_fwd')
    return out


def embedding_sum_bwd(idx, grad_out, dims, row_perm=None):
    _chk(idx, torch.int64)
    _chk(grad_out)
    rows, n_cols = idx.shape
    feat = grad_out.shape[1]
    total = sum(dims)
    L = _lib.load()
    if MULTIHOT_EMB_BWD and rows > 0 and total <= 1024 and n_cols <= 16:
        # all tables at once: multi-hot^T dY, split-K through the scratch (deterministic; the LDS-atomics kernel below
        # needs ~115 us for the 9 atom tables of a 512-molecule batch), at any width (the tower variant's 90 / 70 too)
        v_pad = (total + 31) // 32 * 32
        offsets, o = [], 0
        for d in dims:
            offsets.append(o)
            o += d
        hot = torch.empty(rows, v_pad, dtype=torch.float32, device=idx.device)
        check(L.i3d_multihot(_p(idx), _p(row_perm), rows, n_cols, int_array(offsets), v_pad, _p(hot), _stream()), 'i3d_multihot')
        flat = gemm(hot, grad_out, trans_a=True)
    else:
        flat = torch.zeros(total, feat, dtype=torch.float32, device=idx.device)     # one fill for all tables
        ptrs, o = [], 0
        for d in dims:
            ptrs.append(flat.data_ptr() + 4 * o * feat)
            o += d
        check(L.i3d_embedding_sum_bwd(_p(idx), _p(row_perm), rows, n_cols, _p(grad_out), feat, ptr_array(ptrs),
                                      int_array(list(dims)), _stream()), 'i3d_embedding_sum_bwd')
    grads, o = [], 0
    for d in dims:
        grads.append(flat[o:o + d])
        o += d
    return grads


# I3D_MULTIHOT_EMB_BWD=0: embedding-table gradients by LDS-privatised atomics instead of the multi-hot GEMM
MULTIHOT_EMB_BWD = True


# ---- K4 / K6 ---------------------------------------------------------------------------------------------
def pna_aggregate_fwd(e, in_ptr, num_nodes, aggregators, scalers, avg_d_log=1.0, force_scalers=False, tower_feat=0):
    """tower_feat > 0: the output row is [tower][block][feature of the tower] (include/infomax3d_hip.h: i3d_pna_aggregate_fwd_towers)"""
    _chk(e)
    _chk(in_ptr, torch.int32)
    feat = e.shape[1]
    n_sc = len(scalers) if (len(scalers) > 1 or force_scalers) else 1
    out = torch.empty(num_nodes, n_sc * len(aggregators) * feat, dtype=torch.float32, device=e.device)
    L = _lib.load()
    if tower_feat:
        check(L.i3d_pna_aggregate_fwd_towers(_p(e), _p(in_ptr), num_nodes, feat, tower_feat, int_array(aggregators), len(aggregators),
                                             int_array(scalers), len(scalers), int(force_scalers), float(avg_d_log), _p(out), _stream()),
              'i3d_pna_aggregate_fwd_towers')
        return out
    timed = KERNEL_TIMERS is not None
    if timed:   # bench.py: HIP events on the launch stream around the roofline kernel
        t0, t1 = RawEvent(), RawEvent()
        t0.record()
    check(L.i3d_pna_aggregate_fwd(_p(e), _p(in_ptr), num_nodes, feat, int_array(aggregators), len(aggregators),
                                  int_array(scalers), len(scalers), int(force_scalers), float(avg_d_log), _p(out), _stream()),
          'i3d_pna_aggregate_fwd')
    if timed:
        t1.record()
        KERNEL_TIMERS.setdefault('pna_aggregate_fwd', []).append((t0, t1, num_nodes, e.shape[0], feat, out.shape[1]))
    return out


def pna_aggregate_bwd(grad_out, e, in_ptr, num_nodes, aggregators, scalers, avg_d_log=1.0, force_scalers=False, tower_feat=0):
    _chk(grad_out)
    _chk(e)
    grad_e = torch.empty_like(e)
    L = _lib.load()
    if tower_feat:
        check(L.i3d_pna_aggregate_bwd_towers(_p(grad_out), _p(e), _p(in_ptr), num_nodes, e.shape[1], tower_feat, int_array(aggregators),
                                             len(aggregators), int_array(scalers), len(scalers), int(force_scalers), float(avg_d_log),
                                             _p(grad_e), _stream()), 'i3d_pna_aggregate_bwd_towers')
        return grad_e
    check(L.i3d_pna_aggregate_bwd(_p(grad_out), _p(e), _p(in_ptr), num_nodes, e.shape[1], int_array(aggregators),
                                  len(aggregators), int_array(scalers), len(scalers), int(force_scalers), float(avg_d_log),
                                  _p(grad_e), _stream()), 'i3d_pna_aggregate_bwd')
    return grad_e


def segment_readout_fwd(x, graph_ptr, num_graphs, ops):
    _chk(x)
    _chk(graph_ptr, torch.int32)
    feat = x.shape[1]
    out = torch.empty(num_graphs, len(ops) * feat, dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.i3d_segment_readout_fwd(_p(x), _p(graph_ptr), num_graphs, feat, int_array(ops), len(ops), _p(out), _stream()),
          'i3d_segment_readout_fwd')
    return out


def segment_readout_bwd(grad_out, x, graph_ptr, num_graphs, ops):
    _chk(grad_out)
    _chk(x)
    grad_x = torch.empty_like(x)
    L = _lib.load()
    check(L.i3d_segment_readout_bwd(_p(grad_out), _p(x), _p(graph_ptr), num_graphs, x.shape[1], int_array(ops), len(ops),
                                    _p(grad_x), _stream()), 'i3d_segment_readout_bwd')
    return grad_x


# ---- GEMM ------------------------------------------------------------------------------------------------
def _ld(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1, (t.shape, t.stride())
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def set_matmul_precision(dtype):
    """'fp32' (default): exact fp32 products; 'bf16': bf16-rounded operands on the bf16 matrix pipe, fp32 accumulation
    (every GEMM of the library, process-level).  Returns the previous setting."""
    L = _lib.load()
    prev = 'bf16' if L.i3d_get_matmul_precision() else 'fp32'
    name = {torch.float32: 'fp32', torch.bfloat16: 'bf16'}.get(dtype, dtype)
    if name not in ('fp32', 'bf16'):
        raise ValueError(f'matmul precision {dtype!r}: fp32 or bf16')
    check(L.i3d_set_matmul_precision(int(name == 'bf16')), 'i3d_set_matmul_precision')
    return prev


def get_matmul_precision():
    return 'bf16' if _lib.load().i3d_get_matmul_precision() else 'fp32'


def set_fp32_products(mode):
    """'native': v_mfma_f32_32x32x2_f32; 'split': three-part bf16 split of both operands, six part products on the bf16 pipe
    (include/infomax3d_hip.h: i3d_set_fp32_products).  fp32 mode only.  Returns the previous setting."""
    L = _lib.load()
    prev = 'split' if L.i3d_get_fp32_products() else 'native'
    if mode not in ('native', 'split'):
        raise ValueError(f'fp32 products {mode!r}: native or split')
    check(L.i3d_set_fp32_products(int(mode == 'split')), 'i3d_set_fp32_products')
    return prev


def get_fp32_products():
    return 'split' if _lib.load().i3d_get_fp32_products() else 'native'


def gemm(A, B, trans_a=False, trans_b=False, out=None, bias=None, accumulate=False):
    """out[M,N] = (accumulate ? out : 0) + op(A) op(B) + bias.  A, B, out: 2-D fp32, unit inner stride
    (row slices / column slices of a contiguous tensor are fine: the row stride is the leading dimension)."""
    M, K = (A.shape[1], A.shape[0]) if trans_a else A.shape
    K2, N = (B.shape[1], B.shape[0]) if trans_b else B.shape
    assert K == K2, (A.shape, B.shape, trans_a, trans_b)
    if out is None:
        assert not accumulate
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    L = _lib.load()
    if trans_a and K >= 1024:     # weight gradient: the split-K slices are combined through the scratch (deterministic)
        check(L.i3d_gemm_f32_ws(int(trans_a), int(trans_b), M, N, K, _p(A), _ld(A), _p(B), _ld(B), _p(out), _ld(out),
                                _p(bias), int(accumulate), _p(_gemm_workspace(A.device)), GEMM_WORKSPACE_BYTES, _stream()),
              'i3d_gemm_f32_ws')
        return out
    check(L.i3d_gemm_f32(int(trans_a), int(trans_b), M, N, K, _p(A), _ld(A), _p(B), _ld(B), _p(out), _ld(out),
                         _p(bias), int(accumulate), _stream()), 'i3d_gemm_f32')
    return out


# ---- BatchNorm / activations -----------------------------------------------------------------------------
def act_stats_fwd(pre, act, eps, momentum, running_mean=None, running_var=None, sums_out=None, out=None):
    """x = act(pre) (in place unless `out` is given), returns (x, mean, invstd)."""
    _chk(pre)
    rows, feat = pre.shape
    x = pre if out is None else out
    mean = torch.empty(feat, dtype=torch.float32, device=pre.device)
    invstd = torch.empty(feat, dtype=torch.float32, device=pre.device)
    L = _lib.load()
    check(L.i3d_act_stats_fwd(_p(pre), rows, feat, ACT[act], _p(x), float(eps), float(momentum), _p(mean), _p(invstd),
                              _p(running_mean), _p(running_var), _p(sums_out), _p(_workspace(feat, pre.device)),
                              _stream()), 'i3d_act_stats_fwd')
    return x, mean, invstd


def bn_finalize_stats(sums, feat, eps, momentum, running_mean=None, running_var=None):
    mean = torch.empty(feat, dtype=torch.float32, device=sums.device)
    invstd = torch.empty(feat, dtype=torch.float32, device=sums.device)
    L = _lib.load()
    check(L.i3d_bn_finalize_stats(_p(sums), feat, float(eps), float(momentum), _p(mean), _p(invstd), _p(running_mean),
                                  _p(running_var), _stream()), 'i3d_bn_finalize_stats')
    return mean, invstd


def bn_apply_fwd(x, mean, invstd, gamma, beta, post_act=None, residual=None, out=None):
    _chk(x)
    rows, feat = x.shape
    y = torch.empty_like(x) if out is None else out
    L = _lib.load()
    check(L.i3d_bn_apply_fwd(_p(x), rows, feat, _p(mean), _p(invstd), _p(gamma), _p(beta), ACT[post_act], _p(residual),
                             _p(y), _stream()), 'i3d_bn_apply_fwd')
    return y


def bn_eval_fwd(x, running_mean, running_var, eps, gamma, beta, post_act=None, residual=None, out=None):
    _chk(x)
    rows, feat = x.shape
    y = torch.empty_like(x) if out is None else out
    L = _lib.load()
    check(L.i3d_bn_eval_fwd(_p(x), rows, feat, _p(running_mean), _p(running_var), float(eps), _p(gamma), _p(beta),
                            ACT[post_act], _p(residual), _p(y), _stream()), 'i3d_bn_eval_fwd')
    return y


def bn_bwd(grad_y, x, pre, act, post_act, mean, invstd, gamma, beta, sums_out=None, sums_in=None, total_rows=0,
           grad_gamma=None, grad_beta=None, out=None, grad_bias=None):
    """Returns (grad_pre, grad_gamma, grad_beta).  grad_pre may alias grad_y (out=grad_y); grad_bias (optional, [feat])
    receives the column sums of grad_pre from the same pass."""
    _chk(grad_y)
    _chk(x)
    rows, feat = x.shape
    if grad_gamma is None:
        grad_gamma = torch.empty(feat, dtype=torch.float32, device=x.device)
        grad_beta = torch.empty(feat, dtype=torch.float32, device=x.device)
    grad_pre = torch.empty_like(x) if out is None else out
    L = _lib.load()
    check(L.i3d_bn_bwd(_p(grad_y), _p(x), _p(pre), rows, feat, ACT[act], ACT[post_act], _p(mean), _p(invstd), _p(gamma),
                       _p(beta), _p(grad_gamma), _p(grad_beta), _p(grad_pre), _p(grad_bias), _p(sums_out), _p(sums_in),
                       int(total_rows), _p(_workspace(feat, x.device)), _stream()), 'i3d_bn_bwd')
    return grad_pre, grad_gamma, grad_beta


def bn_eval_bwd(grad_y, x, pre, act, post_act, running_mean, running_var, eps, gamma, beta, out=None):
    _chk(grad_y)
    _chk(x)
    rows, feat = x.shape
    grad_gamma = torch.empty(feat, dtype=torch.float32, device=x.device)
    grad_beta = torch.empty(feat, dtype=torch.float32, device=x.device)
    grad_pre = torch.empty_like(x) if out is None else out
    L = _lib.load()
    check(L.i3d_bn_eval_bwd(_p(grad_y), _p(x), _p(pre), rows, feat, ACT[act], ACT[post_act], _p(running_mean),
                            _p(running_var), float(eps), _p(gamma), _p(beta), _p(grad_gamma), _p(grad_beta), _p(grad_pre),
                            _p(_workspace(feat, x.device)), _stream()), 'i3d_bn_eval_bwd')
    return grad_pre, grad_gamma, grad_beta


def set_bn_bwd_one_launch(on):
    """The BatchNorm backward as one launch (reduction, finalisation and data gradient; csrc/bn.hip: bn_bwd_fused_kernel) - process
    wide, on by default; off = the two-pass kernels (what larger tensors take anyway).  Switch it off when several processes share
    one GPU (include/infomax3d_hip.h: i3d_set_bn_bwd_one_launch).  Returns the previous setting."""
    return bool(_lib.load().i3d_set_bn_bwd_one_launch(int(bool(on))))


def colsum(x, w=None, out=None):
    _chk(x)
    rows, feat = x.shape
    if out is None:
        out = torch.empty(feat, dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.i3d_colsum(_p(x), _p(w), rows, feat, _p(out), _p(_workspace(feat, x.device)), _stream()), 'i3d_colsum')
    return out


def act_fwd(x, act, out=None):
    _chk(x)
    y = torch.empty_like(x) if out is None else out
    check(_lib.load().i3d_act_fwd(_p(x), x.numel(), ACT[act], _p(y), _stream()), 'i3d_act_fwd')
    return y


def act_bwd(grad_y, x, act, out=None):
    _chk(x)
    g = torch.empty_like(x) if out is None else out
    check(_lib.load().i3d_act_bwd(_p(grad_y), _p(x), x.numel(), ACT[act], _p(g), _stream()), 'i3d_act_bwd')
    return g


def add_inplace(dst, src):
    _chk(dst)
    _chk(src)
    assert dst.numel() == src.numel()
    check(_lib.load().i3d_add_inplace(_p(dst), _p(src), dst.numel(), _stream()), 'i3d_add_inplace')
    return dst


def mul(a, b, out=None):
    """out = a * b elementwise (same shape; out may be a)"""
    _chk(a)
    _chk(b)
    assert a.numel() == b.numel()
    if out is None:
        out = torch.empty_like(a)
    check(_lib.load().i3d_mul(_p(a), _p(b), a.numel(), _p(out), _stream()), 'i3d_mul')
    return out


def dropout_mask(like, p):
    """the scaled keep-mask nn.Dropout(p) would apply to a tensor shaped like `like` at this point of torch's generator
    stream: torch's own dropout kernel on a tensor of ones (same shape -> same Philox offsets -> the SAME mask the reference's
    module draws on this device with this seed), values 0 or 1 / (1 - p)"""
    return torch.nn.functional.dropout(torch.ones_like(like), float(p), True)


# ---- edge kernels ----------------------------------------------------------------------------------------
def edge_combine_fwd(P, Q, bias, src_s, dst_s, q_code=None):
    _chk(P)
    E, feat = src_s.shape[0], P.shape[1] // 2
    pre = torch.empty(E, feat, dtype=torch.float32, device=P.device)
    check(_lib.load().i3d_edge_combine_fwd(_p(P), P.shape[1], _p(Q), _p(q_code), _p(bias), _p(src_s), _p(dst_s), E, feat,
                                           _p(pre), _stream()), 'i3d_edge_combine_fwd')
    return pre


def edge_codes(idx, row_perm, dims, v_pad):
    """codes[j] = joint category of row (row_perm[j] if given else j) of idx [rows, C]; onehot [rows, v_pad]."""
    _chk(idx, torch.int64)
    rows, n_cols = idx.shape
    strides, s = [], 1
    for d in dims:
        strides.append(s)
        s *= d
    assert s <= v_pad and v_pad % 4 == 0 and len(dims) == n_cols
    codes = torch.empty(rows, dtype=torch.int32, device=idx.device)
    onehot = torch.empty(rows, v_pad, dtype=torch.float32, device=idx.device)
    check(_lib.load().i3d_edge_codes(_p(idx), _p(row_perm), rows, n_cols, int_array(strides), v_pad, _p(codes), _p(onehot),
                                     _stream()), 'i3d_edge_codes')
    return codes, onehot


def segment_sum(x, ptr, idx, num_segments, mean=False, out=None):
    """out[v] = sum_{j in [ptr[v],ptr[v+1])} x[idx[j] if idx is not None else j]  (x, out may be column slices)."""
    feat = x.shape[1]
    if out is None:
        out = torch.empty(num_segments, feat, dtype=torch.float32, device=x.device)
    check(_lib.load().i3d_segment_sum(_p(x), _ld(x), _p(ptr), _p(idx), num_segments, feat, int(mean), _p(out), _ld(out),
                                      _stream()), 'i3d_segment_sum')
    return out


def segment_bcast(g, ptr, seg_of_row, rows, mean=False):
    _chk(g)
    feat = g.shape[1]
    out = torch.empty(rows, feat, dtype=torch.float32, device=g.device)
    check(_lib.load().i3d_segment_bcast(_p(g), _p(ptr), _p(seg_of_row), rows, feat, int(mean), _p(out), _stream()),
          'i3d_segment_bcast')
    return out


def gather_rows(x, idx):
    _chk(x)
    _chk(idx, torch.int32)
    out = torch.empty(idx.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
    check(_lib.load().i3d_gather_rows(_p(x), _p(idx), idx.shape[0], x.shape[1], _p(out), _stream()), 'i3d_gather_rows')
    return out


def fourier_encode(d, n_enc):
    _chk(d)
    E = d.shape[0]
    out = torch.empty(E, 2 * n_enc + 1, dtype=torch.float32, device=d.device)
    check(_lib.load().i3d_fourier_encode(_p(d), E, n_enc, _p(out), _stream()), 'i3d_fourier_encode')
    return out


def soft_edge_fwd(m, ws, bs):
    _chk(m)
    E, feat = m.shape
    msg = torch.empty_like(m)
    w = torch.empty(E, dtype=torch.float32, device=m.device)
    check(_lib.load().i3d_soft_edge_fwd(_p(m), _p(ws), _p(bs), E, feat, _p(msg), _p(w), _stream()), 'i3d_soft_edge_fwd')
    return msg, w


def soft_edge_bwd(grad_msg, m, w, ws):
    _chk(grad_msg)
    E, feat = m.shape
    gm = torch.empty_like(m)
    gg = torch.empty(E, dtype=torch.float32, device=m.device)
    check(_lib.load().i3d_soft_edge_bwd(_p(grad_msg), _p(m), _p(w), _p(ws), E, feat, _p(gm), _p(gg), _stream()),
          'i3d_soft_edge_bwd')
    return gm, gg


# ---- NT-Xent ---------------------------------------------------------------------------------------------
def row_norms(z):
    _chk(z)
    n = torch.empty(z.shape[0], dtype=torch.float32, device=z.device)
    check(_lib.load().i3d_row_norms(_p(z), z.shape[0], z.shape[1], _p(n), _stream()), 'i3d_row_norms')
    return n


def ntxent_fwd(sim, n1, n2, b1, b2, conf, pos_offset, tau, eps, loss_scale=1.0):
    row_sum = torch.empty(b1, dtype=torch.float32, device=sim.device)
    row_pos = torch.empty(b1, dtype=torch.float32, device=sim.device)
    loss_sum = torch.empty(1, dtype=torch.float32, device=sim.device)
    check(_lib.load().i3d_ntxent_fwd(_p(sim), _p(n1), _p(n2), b1, b2, conf, pos_offset, float(tau), float(eps),
                                     float(loss_scale), _p(row_sum), _p(row_pos), _p(loss_sum), _stream()), 'i3d_ntxent_fwd')
    return row_sum, row_pos, loss_sum


def ntxent_bwd(sim, n1, n2, row_sum, row_pos, b1, b2, conf, pos_offset, tau, eps, grad_scale, grad_scale_dev=None):
    dsim = torch.empty_like(sim)
    ca = torch.empty(b1, dtype=torch.float32, device=sim.device)
    cb = torch.empty(b2 * conf, dtype=torch.float32, device=sim.device)
    check(_lib.load().i3d_ntxent_bwd(_p(sim), _p(n1), _p(n2), _p(row_sum), _p(row_pos), b1, b2, conf, pos_offset,
                                     float(tau), float(eps), float(grad_scale), _p(grad_scale_dev), _p(dsim), _p(ca), _p(cb),
                                     _stream()),
          'i3d_ntxent_bwd')
    return dsim, ca, cb


def add(a, b):
    """a + b (new tensor) without a torch op: clone-free"""
    out = torch.empty_like(a)
    check(_lib.load().i3d_add(_p(a), _p(b), a.numel(), _p(out), _stream()), 'i3d_add')
    return out


def broadcast_row(row, rows):
    """[rows, F] with every row = `row` [F]"""
    out = torch.empty(rows, row.shape[0], dtype=torch.float32, device=row.device)
    check(_lib.load().i3d_broadcast_row(_p(row), rows, row.shape[0], _p(out), _stream()), 'i3d_broadcast_row')
    return out


def row_axpy(z, coef, out):
    _chk(z)
    _chk(out)
    check(_lib.load().i3d_row_axpy(_p(z), _p(coef), z.shape[0], z.shape[1], _p(out), _stream()), 'i3d_row_axpy')
    return out


def row_scale(z, coef):
    _chk(z)
    out = torch.empty_like(z)
    check(_lib.load().i3d_row_scale(_p(z), _p(coef), z.shape[0], z.shape[1], _p(out), _stream()), 'i3d_row_scale')
    return out


# ---- degree-grouped posttrans ------------------------------------------------------------------------------
def _float_array(values):
    from ctypes import c_float
    return (c_float * len(values))(*values)


def combine_weights_fwd(W, f_in, agg_width, coef, n_groups, n_scalers):
    """WD[g] = sum_s coef[g][s] * W[:, f_in + s*agg_width : f_in + (s+1)*agg_width]  -> [n_groups, f_out, agg_width]."""
    _chk(W)
    f_out = W.shape[0]
    WD = torch.empty(n_groups, f_out, agg_width, dtype=torch.float32, device=W.device)
    check(_lib.load().i3d_pna_combine_weights_fwd(_p(W), W.shape[1], f_in, f_out, agg_width, n_groups, n_scalers,
                                                  _float_array(coef), _p(WD), _stream()), 'i3d_pna_combine_weights_fwd')
    return WD


def combine_weights_bwd(dWD, dW, f_in, agg_width, coef, n_groups, n_scalers):
    """dW[:, f_in + s*agg_width ...] = sum_g coef[g][s] * dWD[g]   (writes the aggregate blocks of dW in place)."""
    _chk(dWD)
    _chk(dW)
    check(_lib.load().i3d_pna_combine_weights_bwd(_p(dWD), dW.shape[1], f_in, dW.shape[0], agg_width, n_groups,
                                                  n_scalers, _float_array(coef), _p(dW), _stream()),
          'i3d_pna_combine_weights_bwd')
    return dW


def gemm_grouped(A, m_rows, tile_group, Bg, out, trans_b, accumulate):
    """out[r] (+)= A[r] @ op(Bg[group of r])  for the rows listed in m_rows (64-padded per group, -1 = padding)."""
    _chk(A)
    _chk(Bg)
    K = A.shape[1]
    N = Bg.shape[1] if trans_b else Bg.shape[2]
    assert (Bg.shape[2] if trans_b else Bg.shape[1]) == K and out.shape[1] == N
    check(_lib.load().i3d_gemm_f32_grouped(int(trans_b), m_rows.shape[0], N, K, _p(A), A.shape[1], A.shape[0], _p(m_rows),
                                           _p(tile_group), _p(Bg), Bg.shape[2], Bg.shape[1] * Bg.shape[2], _p(out),
                                           _ld(out), int(accumulate), _stream()), 'i3d_gemm_f32_grouped')
    return out


def gemm_rowsubset_multi(A, B, k_rows, group_start, group_count, out, accumulate=False, tile_cfg=-1, seg_rows=0,
                         use_workspace=True):
    """out[g] = sum over j in [group_start[g], +group_count[g]) of A[k_rows[j],:]^T B[k_rows[j],:]; out: [G, M, N]."""
    _chk(A)
    _chk(B)
    _chk(out)
    G = len(group_start)
    assert out.shape == (G, A.shape[1], B.shape[1])
    check(_lib.load().i3d_gemm_f32_rowsubset_multi(A.shape[1], B.shape[1], G, int_array(list(group_start)),
                                                   int_array(list(group_count)), _p(A), A.shape[1], _p(B), B.shape[1],
                                                   _p(k_rows), A.shape[0], _p(out), out.shape[1] * out.shape[2],
                                                   out.shape[2], int(accumulate), tile_cfg, seg_rows,
                                                   _p(_gemm_workspace(A.device)) if use_workspace else None,
                                                   GEMM_WORKSPACE_BYTES if use_workspace else 0, _stream()),
          'i3d_gemm_f32_rowsubset_multi')
    return out


def gemm_rowsubset(A, B, k_rows, out):
    """out[M,N] = sum over rows r in k_rows of A[r,:M]^T B[r,:N]."""
    _chk(A)
    _chk(B)
    check(_lib.load().i3d_gemm_f32_rowsubset(A.shape[1], B.shape[1], k_rows.shape[0], _p(A), A.shape[1], _p(B), B.shape[1],
                                             _p(k_rows), A.shape[0], _p(out), _ld(out), 0, _stream()),
          'i3d_gemm_f32_rowsubset')
    return out


# ---- BatchNorm out of the memory path (csrc/fused_bn.hip) --------------------------------------------------
def bn_finalize_partials(partial, n_tiles, feat, eps, momentum, gamma=None, beta=None, running_mean=None, running_var=None,
                         num_batches_tracked=None, want_aff=True):
    """per-tile partials [n_tiles, 3, feat] -> (mean, invstd, aff [3, feat] = mean | gamma invstd | beta or None)"""
    _chk(partial)
    dev = partial.device
    mean = torch.empty(feat, dtype=torch.float32, device=dev)
    invstd = torch.empty(feat, dtype=torch.float32, device=dev)
    aff = torch.empty(3, feat, dtype=torch.float32, device=dev) if want_aff else None
    check(_lib.load().i3d_bn_finalize_partials(_p(partial), n_tiles, feat, float(eps), float(momentum), _p(gamma), _p(beta),
                                               _p(mean), _p(invstd), _p(running_mean), _p(running_var),
                                               _p(num_batches_tracked), _p(aff), _stream()), 'i3d_bn_finalize_partials')
    return mean, invstd, aff


def edge_combine_act_stats(P, Q, bias, src_s, dst_s, act=None, q_code=None):
    """x = act(P[src,:F] + P[dst,F:] + Q[code or row] + bias) [E, F] and its per-tile statistics -> (x, partial, n_tiles)"""
    _chk(P)
    E, feat = src_s.shape[0], P.shape[1] // 2
    L = _lib.load()
    rpt = L.i3d_edge_stats_rows_per_tile(feat)
    n_tiles = (E + rpt - 1) // rpt
    x = torch.empty(E, feat, dtype=torch.float32, device=P.device)
    partial = torch.empty(n_tiles, 3, feat, dtype=torch.float32, device=P.device)
    check(L.i3d_edge_combine_act_stats(_p(P), P.shape[1], _p(Q), _p(q_code), _p(bias), _p(src_s), _p(dst_s), E, feat, ACT[act],
                                       _p(x), _p(partial), _stream()), 'i3d_edge_combine_act_stats')
    return x, partial, n_tiles


def gemm_fused(A, W, bias=None, a_aff=None, act=None, want_stats=True, out=None, accumulate=False, m_rows=None,
               tile_group=None):
    """out = act(A' W^T + bias (+ out)), A' = (A - mean) * scale + shift per column when a_aff [3, K] is given;
    -> (out, partial [tiles, 3, N] or None, tiles).  W: [N, K], or [G, N, K] with m_rows / tile_group (grouped).
    act: None, 'relu' or 'leakyrelu' only (since round 4 the fused epilogue carries the ReLU class; SiLU / Sigmoid / Tanh ... run as a
    pass of their own behind a plain product - the C entry point refuses their codes)."""
    _chk(A)
    K = A.shape[1]
    if m_rows is not None:
        M, N, stride, rows_total = m_rows.shape[0], W.shape[1], W.shape[1] * W.shape[2], A.shape[0]
    else:
        M, N, stride, rows_total = A.shape[0], W.shape[0], 0, A.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty(rows_total, N, dtype=torch.float32, device=A.device)
    tiles = (M + 63) // 64
    partial = torch.empty(tiles, 3, N, dtype=torch.float32, device=A.device) if want_stats else None
    check(_lib.load().i3d_gemm_f32_fused(M, N, K, _p(A), K, rows_total, _p(W), K, _p(out), N, _p(bias), int(accumulate),
                                         _p(a_aff), ACT[act], _p(partial), _p(m_rows), _p(tile_group), stride, _stream()),
          'i3d_gemm_f32_fused')
    return out, partial, tiles


def panel_pack(W, trans):
    """The weight of a Linear packed for the row-panel products (csrc/panel.hip): its three bf16 images in the LDS layout of the product
    kernel.  trans=True: B[n][k] = W[n, k] (forward, W stored [out, in]); False: B[n][k] = W[k, n] (data gradient).  -> uint8 tensor"""
    _chk(W)
    N, K = (W.shape[0], W.shape[1]) if trans else (W.shape[1], W.shape[0])
    L = _lib.load()
    packed = torch.empty(L.i3d_panel_packed_bytes(N, K), dtype=torch.uint8, device=W.device)
    check(L.i3d_panel_pack(_p(W), W.stride(0), N, K, int(bool(trans)), _p(packed), _stream()), 'i3d_panel_pack')
    return packed, N, K


def panel_gemm(A, packed, N, bias=None, out=None, accumulate=False):
    """out (+)= A B^T (+ bias) with B packed by panel_pack: every 64-row (or 32-row) slab of A read and split once per 208 columns"""
    _chk(A)
    M, K = A.shape
    if out is None:
        assert not accumulate
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    check(_lib.load().i3d_panel_gemm(M, N, K, _p(A), A.stride(0), _p(packed), _p(out), out.stride(0), _p(bias), int(accumulate), _stream()),
          'i3d_panel_gemm')
    return out


def panel_gemm_fused(A, packed, N, bias=None, a_aff=None, act=None, want_stats=True):
    """gemm_fused in row-panel form -> (out, partial [tiles, 3, N] of 32-row tiles or None, tiles)"""
    _chk(A)
    M, K = A.shape
    L = _lib.load()
    out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    tiles = L.i3d_panel_stats_tiles(M)
    partial = torch.empty(tiles, 3, N, dtype=torch.float32, device=A.device) if want_stats else None
    check(L.i3d_panel_gemm_fused(M, N, K, _p(A), A.stride(0), _p(packed), _p(out), N, _p(bias), _p(a_aff), ACT[act], _p(partial), _stream()),
          'i3d_panel_gemm_fused')
    return out, partial, tiles


def gemm_wgrad_bn(dY, x, grad_bias, aff):
    """dW = dY^T ((x - mean) * scale + shift) from the raw x (aff [3, f_in]); grad_bias = column sums of dY"""
    _chk(dY), _chk(x)
    dW = torch.empty(dY.shape[1], x.shape[1], dtype=torch.float32, device=x.device)
    check(_lib.load().i3d_gemm_f32_wgrad_bn(dY.shape[1], x.shape[1], x.shape[0], _p(dY), dY.shape[1], _p(x), x.shape[1], _p(dW),
                                            x.shape[1], _p(grad_bias), _p(aff), _p(_gemm_workspace(x.device)),
                                            GEMM_WORKSPACE_BYTES, _stream()), 'i3d_gemm_f32_wgrad_bn')
    return dW


def pna_aggregate_fwd_aff(e, aff, in_ptr, num_nodes, aggregators, scalers, avg_d_log, force_scalers=False):
    if e.dtype == torch.bfloat16:      # messages stored as bf16 (the bf16 mode's storage form): i3d_pna_aggregate_fwd_ex
        n_s = len(scalers) if (len(scalers) > 1 or force_scalers) else 1
        out = torch.empty(num_nodes, n_s * len(aggregators) * e.shape[1], dtype=torch.float32, device=e.device)
        check(_lib.load().i3d_pna_aggregate_fwd_ex(e.data_ptr(), 1, _p(aff), _p(in_ptr), num_nodes, e.shape[1], int_array(aggregators),
                                                   len(aggregators), int_array(scalers), len(scalers), int(force_scalers),
                                                   float(avg_d_log), _p(out), _stream()), 'i3d_pna_aggregate_fwd_ex')
        return out
    _chk(e)
    n_s = len(scalers) if (len(scalers) > 1 or force_scalers) else 1
    out = torch.empty(num_nodes, n_s * len(aggregators) * e.shape[1], dtype=torch.float32, device=e.device)
    check(_lib.load().i3d_pna_aggregate_fwd_aff(_p(e), _p(aff), _p(in_ptr), num_nodes, e.shape[1], int_array(aggregators),
                                                len(aggregators), int_array(scalers), len(scalers), int(force_scalers),
                                                float(avg_d_log), _p(out), _stream()), 'i3d_pna_aggregate_fwd_aff')
    return out


def pna_aggregate_bwd_aff(grad_out, e, aff, in_ptr, num_nodes, aggregators, scalers, avg_d_log, force_scalers=False):
    if e.dtype == torch.bfloat16:
        _chk(grad_out)
        ge = torch.empty(e.shape, dtype=torch.float32, device=e.device)      # (every edge row has a destination: all rows are written)
        check(_lib.load().i3d_pna_aggregate_bwd_ex(_p(grad_out), e.data_ptr(), 1, _p(aff), _p(in_ptr), num_nodes, e.shape[1],
                                                   int_array(aggregators), len(aggregators), int_array(scalers), len(scalers),
                                                   int(force_scalers), float(avg_d_log), _p(ge), _stream()), 'i3d_pna_aggregate_bwd_ex')
        return ge
    _chk(grad_out), _chk(e)
    ge = torch.empty_like(e)
    check(_lib.load().i3d_pna_aggregate_bwd_aff(_p(grad_out), _p(e), _p(aff), _p(in_ptr), num_nodes, e.shape[1],
                                                int_array(aggregators), len(aggregators), int_array(scalers), len(scalers),
                                                int(force_scalers), float(avg_d_log), _p(ge), _stream()),
          'i3d_pna_aggregate_bwd_aff')
    return ge


def pna_messages_normalized(e, aff):
    """test entry (i3d_pna_messages_normalized_ex): the messages exactly as the aggregation kernels see them, fp32 [E, F] -
    (e - mean) * scale + shift of a fp32 or bf16 e, aff [3, F] or None"""
    bf16 = e.dtype == torch.bfloat16
    _chk(e, torch.bfloat16 if bf16 else torch.float32)
    out = torch.empty(e.shape, dtype=torch.float32, device=e.device)
    check(_lib.load().i3d_pna_messages_normalized_ex(e.data_ptr(), int(bf16), _p(aff), e.shape[0], e.shape[1], _p(out), _stream()),
          'i3d_pna_messages_normalized_ex')
    return out


WGRAD_PLAIN, WGRAD_BN, WGRAD_COMBINE = (_lib.DEFINES[f'I3D_WGRAD_{k}'] for k in ('PLAIN', 'BN', 'COMBINE'))


def wgrad_multi(problems, outputs):
    """All weight gradients of a layer from one launch + one fixed-order reduction (csrc/wgrad.hip).

    problems: dicts {A [rows, M], B [rows, N], rows (int32 index or None), k_begin, k_count};
    outputs: dicts {kind, first_problem, n_groups, C (tensor, written in place), ldc, c_split, c_delta, aff, row, coef
    (list of n_groups * n_scalers floats), n_scalers, scaler_stride}."""
    L = _lib.load()
    pa = (_lib.WgradProblem * len(problems))()
    keep = []
    for d, p in zip(problems, pa):
        A, B = _chk(d['A']), _chk(d['B'])
        p.A, p.B = A.data_ptr(), B.data_ptr()
        p.rows = d['rows'].data_ptr() if d.get('rows') is not None else None
        p.rows_total = A.shape[0]
        p.lda, p.ldb = d.get('lda', A.shape[1]), d.get('ldb', B.shape[1])
        p.M, p.N = d.get('M', A.shape[1]), d.get('N', B.shape[1])
        p.k_begin = d.get('k_begin', 0)
        p.k_count = d.get('k_count', A.shape[0] if d.get('rows') is None else d['rows'].shape[0])
    oa = (_lib.WgradOutput * len(outputs))()
    for d, o in zip(outputs, oa):
        o.kind, o.n_groups, o.first_problem = d.get('kind', WGRAD_PLAIN), d.get('n_groups', 1), d['first_problem']
        C = _chk(d['C'])
        o.C, o.ldc = C.data_ptr() + 4 * d.get('c_offset', 0), d.get('ldc', C.shape[-1])
        o.c_split, o.c_delta = d.get('c_split', 0), d.get('c_delta', 0)
        o.n_scalers, o.scaler_stride = d.get('n_scalers', 1), d.get('scaler_stride', 0)
        o.aff = d['aff'].data_ptr() if d.get('aff') is not None else None
        o.row = d['row'].data_ptr() if d.get('row') is not None else None
        if d.get('coef') is not None:
            arr = _float_array(d['coef'])
            keep.append(arr)
            o.coef = ctypes.addressof(arr)
    dev = problems[0]['A'].device
    check(L.i3d_wgrad_multi(pa, len(problems), oa, len(outputs), _p(_gemm_workspace(dev)), GEMM_WORKSPACE_BYTES, _stream()),
          'i3d_wgrad_multi')


# ---- distance-prediction baseline (csrc/distance.hip) ----------------------------------------------------------------
def mha_fwd(qkv, graph_ptr, num_graphs, nhead, scale):
    """per-molecule multi-head self-attention: qkv [N, 3H] (in_proj output) -> (out [N, H], lse [N, nhead])"""
    _chk(qkv)
    _chk(graph_ptr, torch.int32)
    N, H = qkv.shape[0], qkv.shape[1] // 3
    out = torch.empty(N, H, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(N, nhead, dtype=torch.float32, device=qkv.device)
    check(_lib.load().i3d_mha_fwd(_p(qkv), _p(graph_ptr), num_graphs, N, H, nhead, float(scale), _p(out), _p(lse), _stream()),
          'i3d_mha_fwd')
    return out, lse


def mha_bwd(qkv, out, grad_out, lse, graph_ptr, num_graphs, nhead, scale):
    """-> grad_qkv [N, 3H]"""
    for t in (qkv, out, grad_out, lse):
        _chk(t)
    N, H = out.shape
    delta = torch.empty(N, nhead, dtype=torch.float32, device=qkv.device)
    grad_qkv = torch.empty_like(qkv)
    check(_lib.load().i3d_mha_bwd(_p(qkv), _p(out), _p(grad_out), _p(lse), _p(graph_ptr), num_graphs, N, H, nhead, float(scale),
                                  _p(delta), _p(grad_qkv), _stream()), 'i3d_mha_bwd')
    return grad_qkv


def ln_res_fwd(x, r, gamma, beta, eps):
    """y = LayerNorm(x + r) -> (y, mean [rows], rstd [rows])"""
    for t in (x, r, gamma, beta):
        _chk(t)
    rows, feat = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(_lib.load().i3d_ln_res_fwd(_p(x), _p(r), _p(gamma), _p(beta), rows, feat, float(eps), _p(y), _p(mean), _p(rstd),
                                     _stream()), 'i3d_ln_res_fwd')
    return y, mean, rstd


def ln_res_bwd(grad_y, x, r, gamma, mean, rstd):
    """-> (grad of x + r [rows, feat], grad_gamma [feat], grad_beta [feat])"""
    _chk(grad_y)
    rows, feat = x.shape
    L = _lib.load()
    gx = torch.empty_like(x)
    gg = torch.empty(feat, dtype=torch.float32, device=x.device)
    gb = torch.empty(feat, dtype=torch.float32, device=x.device)
    if rows == 0:
        return gx, gg.zero_(), gb.zero_()
    partial = torch.empty(L.i3d_ln_res_partial_floats(rows, feat), dtype=torch.float32, device=x.device)
    check(L.i3d_ln_res_bwd(_p(grad_y), _p(x), _p(r), _p(gamma), _p(mean), _p(rstd), rows, feat, _p(gx), _p(partial), _p(gg),
                           _p(gb), _stream()), 'i3d_ln_res_bwd')
    return gx, gg, gb


def pair_sum_fwd(u, bias, pidx):
    """softplus(u_i + u_j + 2 bias) over the pairs of the pair graph index `pidx` -> [pairs, feat] in pair-id order"""
    _chk(u)
    _chk(bias)
    P, feat = pidx.num_edges, u.shape[1]
    out = torch.empty(P, feat, dtype=torch.float32, device=u.device)
    check(_lib.load().i3d_pair_sum_fwd(_p(u), _p(bias), _p(pidx.src_s), _p(pidx.dst_s), _p(pidx.perm), P, feat, _p(out),
                                       _stream()), 'i3d_pair_sum_fwd')
    return out


def pair_sum_bwd(grad_out, u, bias, pidx):
    """-> grad_u [N, feat]: the per-pair gradients summed per node over both ends (fixed order: segment sums)"""
    _chk(grad_out)
    P, feat = pidx.num_edges, u.shape[1]
    gp = torch.empty(P, feat, dtype=torch.float32, device=u.device)
    check(_lib.load().i3d_pair_sum_bwd(_p(grad_out), _p(u), _p(bias), _p(pidx.src_s), _p(pidx.dst_s), _p(pidx.perm), P, feat,
                                       _p(gp), _stream()), 'i3d_pair_sum_bwd')
    return _pair_node_sums(gp, gp, pidx)


def pair_norm_fwd(p, pidx):
    """||p_i - p_j|| over the pairs of `pidx` -> [pairs, 1] in pair-id order"""
    _chk(p)
    P = pidx.num_edges
    out = torch.empty(P, 1, dtype=torch.float32, device=p.device)
    check(_lib.load().i3d_pair_norm_fwd(_p(p), _p(pidx.src_s), _p(pidx.dst_s), _p(pidx.perm), P, p.shape[1], _p(out),
                                        _stream()), 'i3d_pair_norm_fwd')
    return out


def pair_norm_bwd(grad_out, p, dist, pidx):
    """-> grad_p [N, feat]"""
    _chk(grad_out)
    P, feat = pidx.num_edges, p.shape[1]
    gp = torch.empty(P, 2 * feat, dtype=torch.float32, device=p.device)
    check(_lib.load().i3d_pair_norm_bwd(_p(grad_out), _p(p), _p(dist), _p(pidx.src_s), _p(pidx.dst_s), _p(pidx.perm), P, feat,
                                        _p(gp), _stream()), 'i3d_pair_norm_bwd')
    return _pair_node_sums(gp[:, :feat], gp[:, feat:], pidx)


def _pair_node_sums(g_src, g_dst, pidx):
    """node v: sum of g_src over the pairs that start at v (out_ptr / out_epos) + sum of g_dst over those that end at v (in_ptr);
    both [pairs, feat] in the pair graph's epos order"""
    N = pidx.num_nodes
    out = segment_sum(g_src, pidx.out_ptr, pidx.out_epos, N)
    return add_inplace(out, segment_sum(g_dst, pidx.in_ptr, None, N))


# ---- 3D autoencoder: fused two-layer pair head, mean squared error (csrc/pairmlp.hip) -----------------------------------------
PAIR_MLP_MAX_WIDTH = 128


def pair_mlp_supported(width):
    """hidden widths of the two-layer distance_net the fused pair head is built for"""
    return 1 <= width <= PAIR_MLP_MAX_WIDTH


def _pair_mlp_workspace(P, D, device):
    return torch.empty(_lib.load().i3d_pair_mlp_workspace_floats(P, D), dtype=torch.float32, device=device)


def pair_mlp_fwd(AB, b1, gamma, beta, w2, b2, pidx, training, eps, momentum, running_mean=None, running_var=None,
                 num_batches_tracked=None):
    """softplus(f([h_s | h_d]) + f([h_d | h_s])) for f = Linear -> ReLU -> BatchNorm -> Linear(D -> 1) from AB = h [W1a | W1b]^T
    [N, 2D] over the pairs of `pidx` -> (out [P, 1] in pair-id order, stats [4, D] = mean1 | rstd1 | mean2 | rstd2 and coef [2D + 1], both fp64).  Training mode
    updates the running statistics twice (s->d first) and adds 2 to num_batches_tracked, on the device."""
    for t in (AB, b1, gamma, beta, w2, b2):
        _chk(t)
    P, D = pidx.num_edges, AB.shape[1] // 2
    dev = AB.device
    out = torch.empty(P, 1, dtype=torch.float32, device=dev)
    stats = torch.empty(4, D, dtype=torch.float64, device=dev)
    coef = torch.empty(2 * D + 1, dtype=torch.float64, device=dev)
    if P == 0:
        return out, stats, coef
    ws = _pair_mlp_workspace(P, D, dev) if training else None
    nbt = num_batches_tracked if (num_batches_tracked is not None and num_batches_tracked.is_cuda) else None
    check(_lib.load().i3d_pair_mlp_fwd(_p(AB), _p(b1), _p(gamma), _p(beta), _p(w2), _p(b2), _p(pidx.src_s), _p(pidx.dst_s),
                                       _p(pidx.perm), P, D, int(bool(training)), float(eps), float(momentum), _p(running_mean),
                                       _p(running_var), _p(nbt), _p(stats), _p(coef), _p(ws), _p(out), _stream()),
          'i3d_pair_mlp_fwd')
    return out, stats, coef


def pair_mlp_bwd(grad_out, AB, b1, gamma, beta, w2, stats, coef, pidx, training):
    """-> (grad_AB [N, 2D], grad_gamma [D], grad_beta [D], grad_w2 [D], grad_b2 [1])"""
    _chk(grad_out)
    P, D, N = pidx.num_edges, AB.shape[1] // 2, AB.shape[0]
    dev = AB.device
    gAB = torch.empty(N, 2 * D, dtype=torch.float32, device=dev)
    small = torch.empty(3 * D + 1, dtype=torch.float32, device=dev)
    gg, gb, gw2, gb2 = small[:D], small[D:2 * D], small[2 * D:3 * D], small[3 * D:]
    grad_pair = torch.empty(P, dtype=torch.float32, device=dev)
    bcoef = torch.empty(6 * D + 1, dtype=torch.float64, device=dev)
    check(_lib.load().i3d_pair_mlp_bwd(_p(grad_out), _p(coef), _p(AB), _p(b1), _p(gamma), _p(beta), _p(w2), _p(pidx.src_s),
                                       _p(pidx.dst_s), _p(pidx.perm), _p(pidx.in_ptr), _p(pidx.out_ptr), _p(pidx.out_epos), N, P,
                                       D, int(bool(training)), _p(stats), _p(_pair_mlp_workspace(P, D, dev)), _p(grad_pair),
                                       _p(bcoef), _p(gAB), _p(gg), _p(gb), _p(gw2), _p(gb2), _stream()),
          'i3d_pair_mlp_bwd')
    return gAB, gg, gb, gw2, gb2


def mse_fwd(a, b, scale):
    """scale * sum((a - b)^2) -> [1]; deterministic (block partials summed in order), no host read-back"""
    _chk(a)
    _chk(b)
    n = a.numel()
    assert b.numel() == n
    L = _lib.load()
    partial = torch.empty(L.i3d_mse_partial_floats(n), dtype=torch.float32, device=a.device)
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    check(L.i3d_mse_fwd(_p(a), _p(b), n, float(scale), _p(partial), _p(loss), _stream()), 'i3d_mse_fwd')
    return loss


def mse_bwd(a, b, scale, grad_scale_dev, need_a=True, need_b=True):
    """-> (grad_a, grad_b) = (2 scale g (a - b), its negation), g = grad_scale_dev[0] multiplied in on the device"""
    n = a.numel()
    ga = torch.empty_like(a) if need_a else None
    gb = torch.empty_like(b) if need_b else None
    if need_a or need_b:
        check(_lib.load().i3d_mse_bwd(_p(a), _p(b), n, float(scale), _p(grad_scale_dev), _p(ga), _p(gb), _stream()), 'i3d_mse_bwd')
    return ga, gb


# ---- multi-conformer losses with one 2D embedding per conformer (csrc/sep2d.hip) ------------------------------------------------------
SEP2D_MAX_CONFORMERS = 8


def row_normalize_fwd(x):
    """-> (x / max(|x|, 1e-12) per row, the row norms): torch F.normalize"""
    _chk(x)
    y = torch.empty_like(x)
    n = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    check(_lib.load().i3d_row_normalize_fwd(_p(x), x.shape[0], x.shape[1], _p(y), _p(n), _stream()), 'i3d_row_normalize_fwd')
    return y, n


def row_normalize_bwd(x, norms, grad_y):
    _chk(x)
    _chk(grad_y)
    gx = torch.empty_like(x)
    check(_lib.load().i3d_row_normalize_bwd(_p(x), _p(norms), _p(grad_y), x.shape[0], x.shape[1], _p(gx), _stream()),
          'i3d_row_normalize_bwd')
    return gx


def sep2d_fwd(sim, n1, n2, batch, conf, tau):
    """sim [B C, B C] (rows: 2D view, columns: 3D view) -> (row_den [B], row_pos [B], both fp64, loss [1])"""
    _chk(sim)
    row_den = torch.empty(batch, dtype=torch.float64, device=sim.device)
    row_pos = torch.empty(batch, dtype=torch.float64, device=sim.device)
    loss = torch.empty(1, dtype=torch.float32, device=sim.device)
    check(_lib.load().i3d_sep2d_fwd(_p(sim), _p(n1), _p(n2), batch, conf, float(tau), _p(row_den), _p(row_pos), _p(loss), _stream()),
          'i3d_sep2d_fwd')
    return row_den, row_pos, loss


def sep2d_bwd(sim, n1, n2, row_den, row_pos, batch, conf, tau, grad_scale_dev):
    """-> (dsim, ca [B C], cb [B C]); the upstream scalar gradient grad_scale_dev[0] is multiplied in on the device"""
    dsim = torch.empty_like(sim)
    ca = torch.empty(batch * conf, dtype=torch.float32, device=sim.device)
    cb = torch.empty(batch * conf, dtype=torch.float32, device=sim.device)
    check(_lib.load().i3d_sep2d_bwd(_p(sim), _p(n1), _p(n2), _p(row_den), _p(row_pos), batch, conf, float(tau), _p(grad_scale_dev),
                                    _p(dsim), _p(ca), _p(cb), _stream()), 'i3d_sep2d_bwd')
    return dsim, ca, cb


def mmd_pair_fwd(X, Y, batch, conf, kernel_num, kernel_mul):
    """X (2D view), Y (3D view) [B C, D] -> (sim [B, B], bandwidth [B, B], cross [B C, B C], intra [2, B, C, C]); entry [a, b]
    compares the conformers of X[b] with those of Y[a]"""
    _chk(X)
    _chk(Y)
    N, D = X.shape
    dev = X.device
    cross = torch.empty(N, N, dtype=torch.float32, device=dev)
    intra = torch.empty(2, batch, conf, conf, dtype=torch.float32, device=dev)
    bandwidth = torch.empty(batch, batch, dtype=torch.float32, device=dev)
    sim = torch.empty(batch, batch, dtype=torch.float32, device=dev)
    check(_lib.load().i3d_mmd_pair_fwd(_p(X), _p(Y), batch, conf, D, int(kernel_num), float(kernel_mul), _p(cross), _p(intra),
                                       _p(bandwidth), _p(sim), _stream()), 'i3d_mmd_pair_fwd')
    return sim, bandwidth, cross, intra


def mmd_pair_bwd(X, Y, cross, intra, bandwidth, sim, dsim, batch, conf, kernel_num, kernel_mul):
    """-> (dX, dY) from dsim [B, B]; the bandwidth is a constant"""
    _chk(dsim)
    N, D = X.shape
    gcross = torch.empty_like(cross)
    gintra = torch.empty_like(intra)
    dX, dY = torch.empty_like(X), torch.empty_like(Y)
    check(_lib.load().i3d_mmd_pair_bwd(_p(X), _p(Y), _p(cross), _p(intra), _p(bandwidth), _p(sim), _p(dsim), batch, conf, D,
                                       int(kernel_num), float(kernel_mul), _p(gcross), _p(gintra), _p(dX), _p(dY), _stream()),
          'i3d_mmd_pair_bwd')
    return dX, dY


# ---- set-matching and per-conformer NT-Xent (csrc/confmatch.hip) -------------------------------------------------------------------------
PER_CONF_MAX_CONFORMERS = 64
CONF_MATCH_MODES = {'min': 0, 'max': 1}
PER_CONF_MODES = {'v2': 0, 'v3': 1}


def conf_match_fwd(sim, n1, n2, batch, conf, mode, tau):
    """sim [B C, B C] (rows: the conformer-wise 2D view, columns: the 3D view) -> (sel [B, B] uint8: l C + u of the selected entry of
    every molecule pair, row_den [B] fp64, pos_j / pos_lu [B] int32: where the positive sits, loss [1])"""
    _chk(sim)
    dev = sim.device
    sel = torch.empty(batch, batch, dtype=torch.uint8, device=dev)
    dsel = torch.empty(batch, batch, dtype=torch.uint8, device=dev) if mode == CONF_MATCH_MODES['min'] else None
    row_den = torch.empty(batch, dtype=torch.float64, device=dev)
    row_pos = torch.empty(batch, dtype=torch.float64, device=dev)
    pos_j = torch.empty(batch, dtype=torch.int32, device=dev)
    pos_lu = torch.empty(batch, dtype=torch.int32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    check(_lib.load().i3d_conf_match_fwd(_p(sim), _p(n1), _p(n2), batch, conf, int(mode), float(tau), _p(sel), _p(dsel), _p(row_den),
                                         _p(row_pos), _p(pos_j), _p(pos_lu), _p(loss), _stream()), 'i3d_conf_match_fwd')
    return sel, row_den, pos_j, pos_lu, loss


def conf_match_bwd(sim, z1v, z2, n1, n2, sel, row_den, pos_j, pos_lu, batch, conf, mode, norm, tau, grad_scale_dev):
    """-> (dz1v, dz2) from one selected entry per molecule pair; the upstream scalar gradient grad_scale_dev[0] is multiplied in on the
    device"""
    _chk(z1v)
    _chk(z2)
    L = _lib.load()
    work = torch.empty(L.i3d_conf_match_work_floats(batch), dtype=torch.float32, device=sim.device)
    dz1, dz2 = torch.empty_like(z1v), torch.empty_like(z2)
    check(L.i3d_conf_match_bwd(_p(sim), _p(z1v), _p(z2), _p(n1), _p(n2), _p(sel), _p(row_den), _p(pos_j), _p(pos_lu), batch, conf,
                               z2.shape[1], int(mode), int(bool(norm)), float(tau), _p(grad_scale_dev), _p(work), _p(dz1), _p(dz2),
                               _stream()), 'i3d_conf_match_bwd')
    return dz1, dz2


def per_conf_fwd(sim, n1, n2, batch, conf, mode, tau):
    """sim [B, B C] -> (den, pos: [B] (V2) or [B C] (V3), fp64; loss [1])"""
    _chk(sim)
    terms = batch * conf if mode == PER_CONF_MODES['v3'] else batch
    den = torch.empty(terms, dtype=torch.float64, device=sim.device)
    pos = torch.empty(terms, dtype=torch.float64, device=sim.device)
    loss = torch.empty(1, dtype=torch.float32, device=sim.device)
    check(_lib.load().i3d_per_conf_fwd(_p(sim), _p(n1), _p(n2), batch, conf, int(mode), float(tau), _p(den), _p(pos), _p(loss),
                                       _stream()), 'i3d_per_conf_fwd')
    return den, pos, loss


def per_conf_bwd(sim, n1, n2, den, pos, batch, conf, mode, tau, grad_scale_dev):
    """-> (dsim [B, B C], ca [B], cb [B C]); the upstream scalar gradient grad_scale_dev[0] is multiplied in on the device"""
    dsim = torch.empty_like(sim)
    ca = torch.empty(batch, dtype=torch.float32, device=sim.device)
    cb = torch.empty(batch * conf, dtype=torch.float32, device=sim.device)
    check(_lib.load().i3d_per_conf_bwd(_p(sim), _p(n1), _p(n2), _p(den), _p(pos), batch, conf, int(mode), float(tau),
                                       _p(grad_scale_dev), _p(dsim), _p(ca), _p(cb), _stream()), 'i3d_per_conf_bwd')
    return dsim, ca, cb


# ---- InfoNCE / NTXentHard / InfoNCEHard / NTXentExtraNegatives (csrc/hardneg.hip) --------------------------------------------------------
HARDNEG_MODES = {'infonce': 0, 'ntxent_hard': 1, 'infonce_hard': 2, 'extra_negatives': 3}
HARDNEG_MAX_EXTRA = 256


def hardneg_norms(z1, z2, extra=None, norm=True):
    """-> (n1 [b1], n2 [b2], xdot, xn [b1 U]): the row norms (ones without normalisation) and, one wave per extra negative (i, u) of
    extra [b1 U, dim], <z1_i, x_iu> and |x_iu| (None without extras)"""
    _chk(z1)
    _chk(z2)
    b1, b2, dev = z1.shape[0], z2.shape[0], z1.device
    n_extra = 0 if extra is None else _chk(extra).shape[0] // b1
    n1 = torch.empty(b1, dtype=torch.float32, device=dev)
    n2 = torch.empty(b2, dtype=torch.float32, device=dev)
    xdot = torch.empty(b1 * n_extra, dtype=torch.float32, device=dev) if n_extra else None
    xn = torch.empty(b1 * n_extra, dtype=torch.float32, device=dev) if n_extra else None
    check(_lib.load().i3d_hardneg_norms(_p(z1), _p(z2), _p(extra) if n_extra else None, b1, b2, n_extra, z1.shape[1], int(bool(norm)),
                                        _p(n1), _p(n2), _p(xdot), _p(xn), _stream()), 'i3d_hardneg_norms')
    return n1, n2, xdot, xn


def hardneg_fwd(mode, sim, n1, n2, pos_offset, tau, tau_plus=0.0, beta=0.0, extra_weight=1.0, loss_scale=1.0, xdot=None, xn=None):
    """sim [b1, b2] -> (stats [b1, 5] fp64: pos, S, A, C, l; coef [b1, 4]: cp, c1, c2, cq; loss [1] = loss_scale sum_i l_i)"""
    _chk(sim)
    b1, b2 = sim.shape
    n_extra = 0 if xdot is None else xdot.shape[0] // b1
    stats = torch.empty(b1, 5, dtype=torch.float64, device=sim.device)
    coef = torch.empty(b1, 4, dtype=torch.float32, device=sim.device)
    loss = torch.empty(1, dtype=torch.float32, device=sim.device)
    check(_lib.load().i3d_hardneg_fwd(int(mode), _p(sim), _p(n1), _p(n2), _p(xdot), _p(xn), b1, b2, n_extra, int(pos_offset), float(tau),
                                      float(tau_plus), float(beta), float(extra_weight), float(loss_scale), _p(stats), _p(coef),
                                      _p(loss), _stream()), 'i3d_hardneg_fwd')
    return stats, coef, loss


def hardneg_bwd(mode, sim, n1, n2, coef, z1, z2, pos_offset, tau, beta=0.0, grad_scale=1.0, grad_scale_dev=None, norm=True, extra=None,
                xdot=None, xn=None):
    """-> (dsim [b1, b2], ca [b1], cb [b2], dz1 = ca z1 + the extras' part, dz2 = cb z2, dx or None) from one launch; dz1 += dsim z2 and
    dz2 += dsim^T z1 complete the gradients"""
    _chk(sim)
    _chk(z1)
    _chk(z2)
    b1, b2 = sim.shape
    n_extra = 0 if extra is None else _chk(extra).shape[0] // b1
    dsim = torch.empty_like(sim)
    ca = torch.empty(b1, dtype=torch.float32, device=sim.device)
    cb = torch.empty(b2, dtype=torch.float32, device=sim.device)
    dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
    dx = torch.empty_like(extra) if n_extra else None
    check(_lib.load().i3d_hardneg_bwd(int(mode), _p(sim), _p(n1), _p(n2), _p(coef), _p(xdot), _p(xn), _p(z1), _p(z2),
                                      _p(extra) if n_extra else None, b1, b2, n_extra, z1.shape[1], int(pos_offset), int(bool(norm)),
                                      float(tau), float(beta), float(grad_scale), _p(grad_scale_dev), _p(dsim), _p(ca), _p(cb), _p(dz1),
                                      _p(dz2), _p(dx), _stream()), 'i3d_hardneg_bwd')
    return dsim, ca, cb, dz1, dz2, dx


# ---- BarlowTwinsLoss / CosineSimilarityLoss / RegularizationLoss / CriticLoss (csrc/batchstat.hip) ---------------------------------------
BATCHSTAT_MAX_REPEATS = 32


def bs_moments(z1, z2=None, standardised=False, centred=False):
    """z [n, dim] -> (mom [views, 2, dim] fp64: column mean and unbiased variance from centred values, [a1, a2] = (z - mean) / std or
    None, [c1, c2] = z - mean or None); both views in one launch"""
    views = [_chk(z1)] + ([_chk(z2)] if z2 is not None else [])
    n, dim = z1.shape
    mom = torch.empty(len(views), 2, dim, dtype=torch.float64, device=z1.device)
    a = [torch.empty_like(z) for z in views] if standardised else None
    c = [torch.empty_like(z) for z in views] if centred else None
    second = lambda ts: _p(ts[1]) if ts is not None and len(ts) > 1 else None
    check(_lib.load().i3d_bs_moments(_p(z1), _p(z2), n, dim, _p(a[0]) if a else None, second(a), _p(c[0]) if c else None, second(c),
                                     _p(mom), _stream()), 'i3d_bs_moments')
    return mom, a, c


def bs_pass_blocks(dim):
    return _lib.load().i3d_bs_pass_blocks(int(dim))


def bs_matrix_pass(m, inv_n, target, w_diag, w_off, partial=None):
    """m [count, dim, dim] or [dim, dim], C = m inv_n -> partial [count, blocks] fp64, the workgroups' shares of w_diag sum_i
    (C_ii - target)^2 + w_off sum_{i != j} C_ij^2; m is overwritten with the gradient of that sum with respect to C"""
    _chk(m)
    dim = m.shape[-1]
    count = m.shape[0] if m.dim() == 3 else 1
    if partial is None:
        partial = torch.empty(count, bs_pass_blocks(dim), dtype=torch.float64, device=m.device)
    check(_lib.load().i3d_bs_matrix_pass(_p(m), count, dim, float(inv_n), float(target), float(w_diag), float(w_off), _p(partial),
                                         _stream()), 'i3d_bs_matrix_pass')
    return partial


def bs_finish(partial, scale=1.0, mom=None, var_w=0.0):
    """-> loss [1] = scale sum(partial) + var_w * mean over the columns of relu(1 - sqrt(var + 1e-4)), summed over the views of mom"""
    dev = partial.device if partial is not None else mom.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    views, dim = (mom.shape[0], mom.shape[2]) if mom is not None else (0, 0)
    check(_lib.load().i3d_bs_finish(_p(partial), partial.numel() if partial is not None else 0, float(scale), _p(mom), views, dim,
                                    float(var_w) if mom is not None else 0.0, _p(loss), _stream()), 'i3d_bs_finish')
    return loss


def bs_col_bwd(z, mom, a=None, da=None, dc=None, sa=0.0, sc=0.0, var_w=0.0, grad_scale=1.0, grad_scale_dev=None):
    """z, a, da, dc: lists of one tensor per view ([n, dim]; a / da / dc None: the term is absent) -> [dz per view], the backward of the
    standardisation, of the centring and of the variance hinge in one launch"""
    n, dim = z[0].shape
    dz = [torch.empty_like(_chk(t)) for t in z]
    at = lambda ts, k: _p(ts[k]) if ts is not None and len(ts) > k else None
    check(_lib.load().i3d_bs_col_bwd(at(z, 0), at(z, 1), at(a, 0), at(a, 1), at(da, 0), at(da, 1), at(dc, 0), at(dc, 1), n, dim, _p(mom),
                                     float(sa), float(sc), float(var_w), float(grad_scale), _p(grad_scale_dev), at(dz, 0), at(dz, 1),
                                     _stream()), 'i3d_bs_col_bwd')
    return dz


def bs_rows_fwd(x, y):
    """x [rows, dim], y [rows, dim] or [rows, dim, reps] (normalised over dim) -> (rowloss [rows] fp64 = sum_r |x_hat - y_hat_r|^2,
    stats [rows, 1 + 2 reps] fp64: |x|, |y_r|, <x, y_r>)"""
    _chk(x)
    _chk(y)
    rows, dim = x.shape
    reps = y.shape[2] if y.dim() == 3 else 1
    stats = torch.empty(rows, 1 + 2 * reps, dtype=torch.float64, device=x.device)
    rowloss = torch.empty(rows, dtype=torch.float64, device=x.device)
    check(_lib.load().i3d_bs_rows_fwd(_p(x), _p(y), rows, dim, reps, _p(stats), _p(rowloss), _stream()), 'i3d_bs_rows_fwd')
    return rowloss, stats


def bs_rows_bwd(x, y, stats, grad_scale, grad_scale_dev=None):
    """-> (dx, dy) of grad_scale * grad_scale_dev[0] * sum(rowloss) from one launch"""
    rows, dim = x.shape
    reps = y.shape[2] if y.dim() == 3 else 1
    dx, dy = torch.empty_like(x), torch.empty_like(y)
    check(_lib.load().i3d_bs_rows_bwd(_p(x), _p(y), rows, dim, reps, _p(stats), float(grad_scale), _p(grad_scale_dev), _p(dx), _p(dy),
                                      _stream()), 'i3d_bs_rows_bwd')
    return dx, dy


# ---- KLDivergenceMultiplePositives (csrc/klmp.hip) -------------------------------------------------------------------------------------
def kl_mp_fwd(z1, z2, batch, conf, inv_global_batch, want_loss=True):
    """z1 [B, 2 D] (mean | log-variance), z2 [B C, D] -> (stats [B, 3] fp64: kl_b, sum_d var(z2_b), sum_d exp(s1_b); loss [1] =
    inv_global_batch sum_b kl_b, or None)"""
    _chk(z1)
    _chk(z2)
    stats = torch.empty(batch, 3, dtype=torch.float64, device=z1.device)
    loss = torch.empty(1, dtype=torch.float32, device=z1.device) if want_loss else None
    check(_lib.load().i3d_kl_mp_fwd(_p(z1), _p(z2), batch, conf, z2.shape[1], float(inv_global_batch), _p(stats), _p(loss), _stream()),
          'i3d_kl_mp_fwd')
    return stats, loss


def kl_mp_bwd(z1, z2, batch, conf, inv_global_batch, grad_scale_dev):
    """-> (dz1, dz2); the upstream scalar gradient grad_scale_dev[0] is multiplied in on the device"""
    _chk(z1)
    _chk(z2)
    dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
    check(_lib.load().i3d_kl_mp_bwd(_p(z1), _p(z2), batch, conf, z2.shape[1], float(inv_global_batch), _p(grad_scale_dev), _p(dz1),
                                    _p(dz2), _stream()), 'i3d_kl_mp_bwd')
    return dz1, dz2


# ---- NTXentLikelihoodLoss / PositiveProb / NegativeProb / JSDMultiplePositivesLoss (csrc/gausspair.hip) -----------------------------------
def gauss_z2_strides(batch, conf, dim, conformer_major=False):
    """(molecule stride, conformer stride) in floats of z2 [B C, D]: row j C + c (the losses) or row c B + j (the metrics)"""
    return (dim, batch * dim) if conformer_major else (conf * dim, dim)


def gauss_lik_fwd(z1, z2, batch, conf, conformer_major=False):
    """z1 [B, 2 D] (mean | log-variance), z2 [B C, D] -> lik [B, B] fp64: the mean over conformers and features of the densities of
    molecule j's conformers under molecule i's Gaussian"""
    _chk(z1)
    _chk(z2)
    dim = z2.shape[1]
    ms, cs = gauss_z2_strides(batch, conf, dim, conformer_major)
    lik = torch.empty(batch, batch, dtype=torch.float64, device=z1.device)
    check(_lib.load().i3d_gauss_lik_fwd(_p(z1), _p(z2), batch, conf, dim, ms, cs, _p(lik), _stream()), 'i3d_gauss_lik_fwd')
    return lik


def gauss_lik_loss(lik, tau):
    """-> (rows [B, 2] fp64: log den_i, l_i; loss [1] = mean_i l_i)"""
    batch = lik.shape[0]
    rows = torch.empty(batch, 2, dtype=torch.float64, device=lik.device)
    loss = torch.empty(1, dtype=torch.float32, device=lik.device)
    check(_lib.load().i3d_gauss_lik_loss(_p(lik), batch, float(tau), _p(rows), _p(loss), _stream()), 'i3d_gauss_lik_loss')
    return rows, loss


def gauss_lik_probs(lik):
    """-> [2] fp64: mean_i lik_ii, mean_i sum_{j != i} lik_ij"""
    out = torch.empty(2, dtype=torch.float64, device=lik.device)
    check(_lib.load().i3d_gauss_lik_probs(_p(lik), lik.shape[0], _p(out), _stream()), 'i3d_gauss_lik_probs')
    return out


def gauss_lik_bwd(z1, z2, batch, conf, lik, rows, tau, grad_scale_dev):
    """-> (dz1, dz2), z2 molecule major; the upstream scalar gradient grad_scale_dev[0] is multiplied in on the device"""
    _chk(z1)
    _chk(z2)
    dim = z2.shape[1]
    ms, cs = gauss_z2_strides(batch, conf, dim)
    grad_lik = torch.empty_like(lik)
    dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
    check(_lib.load().i3d_gauss_lik_bwd(_p(z1), _p(z2), batch, conf, dim, ms, cs, _p(lik), _p(rows), float(tau), _p(grad_scale_dev),
                                        _p(grad_lik), _p(dz1), _p(dz2), _stream()), 'i3d_gauss_lik_bwd')
    return dz1, dz2


def gauss_jsd_fwd(z1, z2, batch, conf):
    """-> (astat [B, 2], rows [B, 3] fp64, loss [1]); the [B, B] similarity is scratch of the forward pass"""
    _chk(z1)
    _chk(z2)
    dev = z1.device
    astat = torch.empty(batch, 2, dtype=torch.float64, device=dev)
    sim = torch.empty(batch, batch, dtype=torch.float64, device=dev)
    rows = torch.empty(batch, 3, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    check(_lib.load().i3d_gauss_jsd_fwd(_p(z1), _p(z2), batch, conf, z2.shape[1], _p(astat), _p(sim), _p(rows), _p(loss), _stream()),
          'i3d_gauss_jsd_fwd')
    return astat, rows, loss


def gauss_jsd_bwd(z1, z2, batch, conf, astat, rows, grad_scale_dev):
    """-> (dz1, dz2); the upstream scalar gradient grad_scale_dev[0] is multiplied in on the device"""
    _chk(z1)
    _chk(z2)
    dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
    check(_lib.load().i3d_gauss_jsd_bwd(_p(z1), _p(z2), batch, conf, z2.shape[1], _p(astat), _p(rows), _p(grad_scale_dev), _p(dz1),
                                        _p(dz2), _stream()), 'i3d_gauss_jsd_bwd')
    return dz1, dz2


# ---- fine-tuning: NaN-label losses and task moments (csrc/task.hip) -----------------------------------------------------------------------
MASKED_LOSS_KINDS = {'bce_with_logits': 0, 'mse': 1}


def masked_loss_fwd(pred, target, kind):
    """pred, target [B, T] -> out [3] fp64: the mean over the elements whose target is not NaN, their count, and (first four bytes of
    out[2]) the mean in fp32 - out.view(torch.float32)[4] is the loss tensor"""
    _chk(pred)
    _chk(target)
    L = _lib.load()
    B, T = pred.shape
    partials = torch.empty(L.i3d_masked_loss_partial_floats(B, T) // 2, dtype=torch.float64, device=pred.device)
    out = torch.empty(3, dtype=torch.float64, device=pred.device)
    check(L.i3d_masked_loss_fwd(_p(pred), _p(target), B, T, int(kind), _p(partials), _p(out), _stream()), 'i3d_masked_loss_fwd')
    return out


def masked_loss_bwd(pred, target, kind, out, grad_out_dev):
    """-> grad_pred [B, T]; the upstream scalar gradient grad_out_dev[0] and the labelled count out[1] are read on the device"""
    _chk(pred)
    _chk(target)
    _chk(grad_out_dev)
    B, T = pred.shape
    grad = torch.empty_like(pred)
    check(_lib.load().i3d_masked_loss_bwd(_p(pred), _p(target), B, T, int(kind), _p(out), _p(grad_out_dev), _p(grad), _stream()),
          'i3d_masked_loss_bwd')
    return grad


def task_moments(pred, target):
    """pred, target [B, T] -> table [T + 1, 10] fp64 on the device (include/infomax3d_hip.h: i3d_task_moments)"""
    _chk(pred)
    _chk(target)
    L = _lib.load()
    B, T = pred.shape
    partials = torch.empty(L.i3d_task_moments_partial_floats(B, T) // 2, dtype=torch.float64, device=pred.device)
    table = torch.empty(T + 1, 10, dtype=torch.float64, device=pred.device)
    check(L.i3d_task_moments(_p(pred), _p(target), B, T, _p(partials), _p(table), _stream()), 'i3d_task_moments')
    return table


# ---- GIN message step (csrc/gin.hip) -------------------------------------------------------------------------
def code_sorted_index(codes, num_codes):
    """(order [E], code_ptr [V + 1]) int32: the edge positions sorted by code (stable) and where every code's run starts in that
    list - what i3d_gin_conv_bwd reduces the table gradient over.  Built once per batch, beside edge_codes; index plumbing in
    torch (a stable sort and a count), on whatever device `codes` lives on."""
    c = codes.long()
    order = torch.sort(c, stable=True)[1].to(torch.int32)
    ptr = torch.zeros(num_codes + 1, dtype=torch.int64, device=codes.device)
    if c.numel():
        torch.cumsum(torch.bincount(c, minlength=num_codes)[:num_codes], 0, out=ptr[1:])
    return order, ptr.to(torch.int32)


def gin_conv_fwd(h, vn, graph_ptr, num_graphs, T, codes, in_ptr, src_s, eps):
    """-> (x, z): x = h + vn[graph of the node] (x is h itself when vn is None), z = (1 + eps) x + sum over the in-edges of
    relu(x[src] + T[code]).  One launch (include/infomax3d_hip.h: i3d_gin_conv_fwd)."""
    _chk(h)
    _chk(T)
    _chk(eps)
    N, H = h.shape
    E = 0 if codes is None else codes.shape[0]
    x = h
    if vn is not None:
        _chk(vn)
        x = torch.empty_like(h)
    z = torch.empty_like(h)
    check(_lib.load().i3d_gin_conv_fwd(_p(h), _p(vn), _p(graph_ptr), num_graphs, _p(T), T.shape[0], _p(codes), _p(in_ptr), _p(src_s),
                                       _p(eps), N, E, H, _p(x) if vn is not None else None, _p(z), _stream()), 'i3d_gin_conv_fwd')
    return x, z


def gin_conv_bwd(g, x, T, codes, src_s, dst_s, out_ptr, out_epos, code_order, code_ptr, eps, dT_out=None):
    """-> (dx [N, H], dT [V, H], deps [1]) from g = dL/dz (include/infomax3d_hip.h: i3d_gin_conv_bwd)"""
    _chk(g)
    _chk(x)
    _chk(T)
    N, H = x.shape
    V = T.shape[0]
    E = 0 if codes is None else codes.shape[0]
    L = _lib.load()
    partials = torch.empty(max(L.i3d_gin_conv_bwd_partial_floats(N, E, H, V), 2), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    dT = torch.empty_like(T) if dT_out is None else dT_out
    deps = torch.empty(1, dtype=torch.float32, device=x.device)
    check(L.i3d_gin_conv_bwd(_p(g), _p(x), _p(T), V, _p(codes), _p(src_s), _p(dst_s), _p(out_ptr), _p(out_epos), _p(code_order),
                             _p(code_ptr), _p(eps), N, E, H, _p(partials), _p(dx), _p(dT), _p(deps), _stream()), 'i3d_gin_conv_bwd')
    return dx, dT, deps


# ---- EGNN: gate, in-edge reduction, residual add (csrc/egnn.hip) -----------------------------------------------------------------
def gate_reduce_max_feat():
    return _lib.load().i3d_gate_reduce_max_feat()


def gate_reduce_fwd(m, ws, bs, in_ptr, h, mean=False):
    """-> (u [N, H], w [E]) with u[v] = h[v] + sum (mean) over the in-edges j of v of m[j] sigmoid(<ws, m[j]> + bs), w the gates; one
    launch.  None when the kernel does not take the shape (include/infomax3d_hip.h: I3D_NOT_TAKEN): the caller composes the step."""
    _chk(m)
    _chk(h)
    _chk(ws)
    _chk(bs)
    _chk(in_ptr, torch.int32)
    E, H = m.shape
    N = h.shape[0]
    assert h.shape[1] == H and ws.numel() == H and bs.numel() == 1 and in_ptr.shape[0] == N + 1
    u = torch.empty_like(h)
    w = torch.empty(E, dtype=torch.float32, device=m.device)
    rc = _lib.load().i3d_gate_reduce_fwd(_p(m), _p(ws), _p(bs), _p(in_ptr), _p(h), N, E, H, int(mean), _p(u), _p(w), _stream())
    if rc == _lib.NOT_TAKEN:
        return None
    check(rc, 'i3d_gate_reduce_fwd')
    return u, w


def gate_reduce_bwd(gu, m, w, ws, in_ptr, mean=False):
    """-> (gm [E, H], gws [H], gbs [1]) from gu = dL/du; dL/dh is gu itself.  One launch and the two column sums over the per-node
    partial rows.  None when the kernel does not take the shape."""
    _chk(gu)
    _chk(m)
    _chk(w)
    _chk(ws)
    E, H = m.shape
    N = gu.shape[0]
    gm = torch.empty_like(m)
    part_ws = torch.empty(N, H, dtype=torch.float32, device=m.device)
    part_bs = torch.empty(N, 1, dtype=torch.float32, device=m.device)
    rc = _lib.load().i3d_gate_reduce_bwd(_p(gu), _p(m), _p(w), _p(ws), _p(in_ptr), N, E, H, int(mean), _p(gm), _p(part_ws),
                                         _p(part_bs), _stream())
    if rc == _lib.NOT_TAKEN:
        return None
    check(rc, 'i3d_gate_reduce_bwd')
    return gm, colsum(part_ws), colsum(part_bs)


# ---- SAN's edge attention (csrc/san.hip) -------------------------------------------------------------------------------------------
def san_attn_takes(feat, heads, num_codes):
    """whether the kernels' lane map covers the shape (include/infomax3d_hip.h: i3d_san_attn_fwd); ValueError on impossible sizes"""
    rc = _lib.load().i3d_san_attn_takes(feat, heads, num_codes)
    if rc == _lib.NOT_TAKEN:
        return False
    check(rc, 'i3d_san_attn_takes')
    return True


def san_edge_codes(bond_idx, real_in, perm, dims):
    """-> (codes [E] int32, real [E] uint8 or None): the joint bond code (first column fastest, as edge_codes) and the real flag of
    every edge position of the destination-sorted order, from bond_idx [E, C] and real_in [E] int64 in edge-id order.  One launch."""
    _chk(bond_idx, torch.int64)
    _chk(perm, torch.int32)
    E, n_cols = bond_idx.shape
    strides, s = [], 1
    for d in dims:
        strides.append(s)
        s *= d
    assert len(dims) == n_cols and perm.shape[0] == E
    codes = torch.empty(E, dtype=torch.int32, device=bond_idx.device)
    real = None
    if real_in is not None:
        real_in = _chk(real_in.contiguous(), torch.int64)
        assert real_in.shape[0] == E
        real = torch.empty(E, dtype=torch.uint8, device=bond_idx.device)
    check(_lib.load().i3d_san_edge_codes(_p(bond_idx), _p(real_in), _p(perm), E, n_cols, int_array(strides), _p(codes), _p(real),
                                         _stream()), 'i3d_san_edge_codes')
    return codes, real


def _san_blocks(Y, H, full_graph):
    """the column blocks Q | K | V (| Q_2 | K_2) of the stacked product Y [N, 3H or 5H]"""
    n = 5 if full_graph else 3
    assert Y.dim() == 2 and Y.shape[1] == n * H and Y.stride(1) == 1, (Y.shape, Y.stride(), H)
    blocks = [Y[:, b * H:(b + 1) * H] for b in range(n)]
    return blocks + [None] * (5 - n)


def san_attn_fwd(Y, te, te2, codes, real, in_ptr, src_s, heads, gamma, full_graph):
    """-> (out [N, H], s [E, nh], z [N, nh]) from the stacked projections Y = Q | K | V (| Q_2 | K_2) [N, 3H or 5H] and the tables
    te, te2 [V, H]; None when the kernel does not take the shape.  One launch; none at all for N = 0 or E = 0 (zero rows)."""
    _chk(Y)
    _chk(te)
    H = te.shape[1]
    q, k, v, q2, k2 = _san_blocks(Y, H, full_graph)
    N, V = Y.shape[0], te.shape[0]
    E = 0 if codes is None else codes.shape[0]
    if not san_attn_takes(H, heads, V) or (E and (codes.dtype != torch.int32 or (full_graph and real.dtype != torch.uint8))):
        return None
    if full_graph:
        _chk(te2)
    out = torch.empty(N, H, dtype=torch.float32, device=Y.device)
    s = torch.empty(E, heads, dtype=torch.float32, device=Y.device)
    z = torch.empty(N, heads, dtype=torch.float32, device=Y.device)
    if N == 0 or E == 0:
        return out.zero_(), s, z.zero_()
    assert in_ptr.shape[0] == N + 1 and src_s.shape[0] == E
    check(_lib.load().i3d_san_attn_fwd(_p(q), _p(k), _p(v), _p(q2), _p(k2), Y.stride(0), _p(te), _p(te2), V, _p(codes), _p(real),
                                       _p(in_ptr), _p(src_s), N, E, H, heads, int(full_graph), float(gamma), _p(out), _p(s), _p(z),
                                       _stream()), 'i3d_san_attn_fwd')
    return out, s, z


def san_attn_bwd(g, out, z, s, Y, te, te2, codes, real, index, code_order, code_ptr, heads, gamma, full_graph):
    """-> (dY [N, 3H or 5H], dte [V, H], dte2 [V, H] or None) from g = dL/dout and what san_attn_fwd returned; `index`: the batch's
    graph.GraphIndex.  Four launches; none for N = 0 or E = 0 (zero gradients)."""
    _chk(g)
    H, V = te.shape[1], te.shape[0]
    q, k, v, q2, k2 = _san_blocks(Y, H, full_graph)
    N, E = Y.shape[0], s.shape[0]
    dY = torch.empty_like(Y)
    dte = torch.empty_like(te)
    dte2 = torch.empty_like(te2) if full_graph else None
    if N == 0 or E == 0:
        return dY.zero_(), dte.zero_(), dte2.zero_() if full_graph else None
    dq, dk, dv, dq2, dk2 = _san_blocks(dY, H, full_graph)
    L = _lib.load()
    gn = torch.empty(N, H, dtype=torch.float32, device=Y.device)
    ds = torch.empty(E, heads, dtype=torch.float32, device=Y.device)
    partials = torch.empty(max(L.i3d_san_attn_bwd_partial_floats(E, H, V), 2), dtype=torch.float32, device=Y.device)
    check(L.i3d_san_attn_bwd(_p(g), _p(out), _p(z), _p(s), _p(q), _p(k), _p(v), _p(q2), _p(k2), Y.stride(0), _p(te), _p(te2), V, _p(codes),
                             _p(real), _p(index.in_ptr), _p(index.src_s), _p(index.dst_s), _p(index.out_ptr), _p(index.out_epos),
                             _p(code_order), _p(code_ptr), N, E, H, heads, int(full_graph), float(gamma), _p(gn), _p(ds), _p(partials),
                             _p(dq), _p(dk), _p(dv), _p(dq2), _p(dk2), dY.stride(0), _p(dte), _p(dte2), _stream()), 'i3d_san_attn_bwd')
    return dY, dte, dte2


# ---- SMP / SphereNet: geometry, raw bases, triplet interaction (csrc/smp.hip) ---------------------------------------------------------
class SmpGeometry:
    """the radius graph and the triplet lists of one batch (include/infomax3d_hip.h: i3d_smp_radius_fill, i3d_smp_triplet_fill):
    src, dst, dist [E]; in_ptr [N + 1]; trip_ptr [E + 1], idx_kj, idx_ji [T] grouped by ji; kj_ptr [E + 1], kj_order [T] the same
    list grouped by kj (a stable sort, so every group keeps the triplet order)"""
    __slots__ = ('N', 'E', 'T', 'src', 'dst', 'dist', 'in_ptr', 'trip_ptr', 'idx_kj', 'idx_ji', 'kj_ptr', 'kj_order')


def _ptr_of(counts):
    ptr = torch.zeros(counts.shape[0] + 1, dtype=torch.int32, device=counts.device)
    ptr[1:] = torch.cumsum(counts, 0)
    return ptr


def smp_geometry(pos, batch, num_graphs, cutoff):
    """-> SmpGeometry of pos [N, 3] with the non-decreasing molecule index batch [N].  Count launch, cumsum, fill launch, twice; the
    host reads the two totals E and T and nothing else.  N = 0, E = 0 and T = 0 launch nothing further and give empties."""
    _chk(pos)
    N, dev = pos.shape[0], pos.device
    assert pos.shape == (N, 3) and batch.shape == (N,)
    L = _lib.load()
    i32 = dict(dtype=torch.int32, device=dev)
    mol = batch.to(torch.int32).contiguous()
    graph_ptr = torch.searchsorted(mol, torch.arange(num_graphs + 1, **i32)).to(torch.int32)
    geo = SmpGeometry()
    deg = torch.zeros(N, **i32)
    check(L.i3d_smp_radius_count(_p(pos), _p(mol), _p(graph_ptr), N, num_graphs, float(cutoff), _p(deg), _stream()), 'i3d_smp_radius_count')
    geo.in_ptr = _ptr_of(deg)
    geo.N, geo.E = N, int(geo.in_ptr[-1])
    geo.src, geo.dst = torch.empty(geo.E, **i32), torch.empty(geo.E, **i32)
    geo.dist = torch.empty(geo.E, dtype=torch.float32, device=dev)
    check(L.i3d_smp_radius_fill(_p(pos), _p(mol), _p(graph_ptr), _p(geo.in_ptr), N, num_graphs, geo.E, float(cutoff), _p(geo.src),
                                _p(geo.dst), _p(geo.dist), _stream()), 'i3d_smp_radius_fill')
    count = torch.zeros(geo.E, **i32)
    check(L.i3d_smp_triplet_count(_p(geo.src), _p(geo.dst), _p(geo.in_ptr), geo.E, _p(count), _stream()), 'i3d_smp_triplet_count')
    geo.trip_ptr = _ptr_of(count)
    geo.T = int(geo.trip_ptr[-1])
    geo.idx_kj, geo.idx_ji = torch.empty(geo.T, **i32), torch.empty(geo.T, **i32)
    check(L.i3d_smp_triplet_fill(_p(geo.src), _p(geo.dst), _p(geo.in_ptr), _p(geo.trip_ptr), geo.E, geo.T, _p(geo.idx_kj), _p(geo.idx_ji),
                                 _stream()), 'i3d_smp_triplet_fill')
    if geo.T:
        order = torch.sort(geo.idx_kj, stable=True)[1]
        geo.kj_order = order.to(torch.int32)
        geo.kj_ptr = _ptr_of(torch.bincount(geo.idx_kj, minlength=geo.E))
    else:
        geo.kj_order, geo.kj_ptr = torch.empty(0, **i32), torch.zeros(geo.E + 1, **i32)
    return geo


def smp_bases(pos, geo, num_spherical, num_radial, cutoff, zeros, norm, pref):
    """-> (angle [T], torsion [T], sbf [T, n k], t [T, n n k]) fp32 from the fp64 device tables zeros, norm [n, k] and pref [n n] (smp.py
    builds them).  Three launches, none for T = 0."""
    _chk(pos)
    n, k = num_spherical, num_radial
    for tab, size in ((zeros, n * k), (norm, n * k), (pref, n * n)):
        _chk(tab, torch.float64)
        assert tab.numel() == size
    f32 = dict(dtype=torch.float32, device=pos.device)
    angle, torsion = torch.empty(geo.T, **f32), torch.empty(geo.T, **f32)
    sbf, t = torch.empty(geo.T, n * k, **f32), torch.empty(geo.T, n * n * k, **f32)
    if geo.T:
        rbf_ws = torch.empty(geo.E, n * k, dtype=torch.float64, device=pos.device)
        cbf_ws = torch.empty(geo.T, n * n, dtype=torch.float64, device=pos.device)
        check(_lib.load().i3d_smp_bases(_p(pos), _p(geo.dist), _p(geo.src), _p(geo.dst), _p(geo.in_ptr), _p(geo.idx_kj), _p(geo.idx_ji),
                                        geo.E, geo.T, n, k, float(cutoff), _p(zeros), _p(norm), _p(pref), _p(rbf_ws), _p(cbf_ws),
                                        _p(angle), _p(torsion), _p(sbf), _p(t), _stream()), 'i3d_smp_bases')
    return angle, torsion, sbf, t


def smp_triplets_takes(int_emb, basis_emb):
    """whether the kernels' lane map covers the shape: int_emb <= 256 (lane c owns the columns c + 64 r, r < 1, 2 or 4) and
    basis_emb <= 8 (a lane keeps its rows of both weights in registers; 16 columns would spill them); ValueError on impossible sizes"""
    if int_emb < 1 or basis_emb < 1:
        raise ValueError(f'smp_triplets_takes: int_emb {int_emb} / basis_emb {basis_emb} below 1')
    rc = _lib.load().i3d_smp_triplets_takes(int_emb, basis_emb)
    if rc == _lib.NOT_TAKEN:
        return False
    check(rc, 'i3d_smp_triplets_takes')
    return True


def smp_triplets_fwd(x, s8, t8, w1, w2, geo):
    """out [E, I] = sum over the triplets of every ji edge of x[idx_kj] * (s8 w1^T) * (t8 w2^T); None when the kernels do not take
    (I, Bs).  One launch; none for E = 0, and T = 0 gives zeros."""
    for a in (x, s8, t8, w1, w2):
        _chk(a)
    (E, I), Bs = x.shape, w1.shape[1]
    assert E == geo.E and s8.shape == (geo.T, Bs) and t8.shape == (geo.T, Bs) and w1.shape == (I, Bs) and w2.shape == (I, Bs)
    if not smp_triplets_takes(I, Bs):
        return None
    if E == 0 or geo.T == 0:
        return torch.zeros(E, I, dtype=torch.float32, device=x.device)
    out = torch.empty(E, I, dtype=torch.float32, device=x.device)
    check(_lib.load().i3d_smp_triplets_fwd(_p(x), _p(s8), _p(t8), _p(w1), _p(w2), _p(geo.trip_ptr), _p(geo.idx_kj), E, geo.T, I, Bs,
                                           _p(out), _stream()), 'i3d_smp_triplets_fwd')
    return out


def smp_triplets_bwd(g, x, s8, t8, w1, w2, geo):
    """-> (dx [E, I], ds8 [T, Bs], dt8 [T, Bs], dw1 [I, Bs], dw2 [I, Bs]) from g = dL/dout.  Four launches; zeros for E = 0 or T = 0."""
    for a in (g, x, s8, t8, w1, w2):
        _chk(a)
    (E, I), Bs = x.shape, w1.shape[1]
    assert g.shape == x.shape
    if E == 0 or geo.T == 0:
        return tuple(torch.zeros_like(a) for a in (x, s8, t8, w1, w2))
    dx, ds8, dt8, dw1, dw2 = (torch.empty_like(a) for a in (x, s8, t8, w1, w2))
    L = _lib.load()
    partials = torch.empty(L.i3d_smp_triplets_bwd_partial_floats(geo.T, I, Bs), dtype=torch.float32, device=x.device)
    check(L.i3d_smp_triplets_bwd(_p(g), _p(x), _p(s8), _p(t8), _p(w1), _p(w2), _p(geo.trip_ptr), _p(geo.idx_kj), _p(geo.idx_ji),
                                 _p(geo.kj_ptr), _p(geo.kj_order), E, geo.T, I, Bs, _p(partials), _p(dx), _p(ds8), _p(dt8), _p(dw1),
                                 _p(dw2), _stream()), 'i3d_smp_triplets_bwd')
    return dx, ds8, dt8, dw1, dw2


# ---- GeoMol's message-passing step (csrc/geomol.hip) -----------------------------------------------------------------------------
GEOMOL_PARTIAL_FLOATS = _lib.DEFINES['I3D_GEOMOL_PARTIAL_FLOATS']


def geomol_edge_fwd(F, PQ, src_s, dst_s):
    """h [E, H] = relu(F + P[src] + Q[dst]); PQ [N, 2H] holds P | Q.  One launch."""
    _chk(F)
    _chk(PQ)
    E, H = F.shape
    N = PQ.shape[0]
    assert PQ.shape[1] == 2 * H and src_s.shape[0] == E and dst_s.shape[0] == E
    h = torch.empty_like(F)
    check(_lib.load().i3d_geomol_edge_fwd(_p(F), _p(PQ), _p(src_s), _p(dst_s), N, E, H, _p(h), _stream()), 'i3d_geomol_edge_fwd')
    return h


def geomol_edge_bwd(g, h, in_ptr, out_ptr, out_epos):
    """-> (dF [E, H], dPQ [N, 2H] = dP | dQ) from g = dL/dh and the forward's h.  One launch."""
    _chk(g)
    _chk(h)
    _chk(in_ptr, torch.int32)
    _chk(out_ptr, torch.int32)
    E, H = h.shape
    N = in_ptr.shape[0] - 1
    assert g.shape == h.shape and out_ptr.shape[0] == N + 1 and out_epos.shape[0] == E
    dF = torch.empty_like(h)
    dPQ = torch.empty(N, 2 * H, dtype=torch.float32, device=h.device)
    check(_lib.load().i3d_geomol_edge_bwd(_p(g), _p(h), _p(in_ptr), _p(out_ptr), _p(out_epos), N, E, H, _p(dF), _p(dPQ), _stream()),
          'i3d_geomol_edge_bwd')
    return dF, dPQ


def geomol_residual_fwd(a, b, eps):
    """(1 + eps) a + b on [R, H]; eps a device tensor [1]: no host synchronisation"""
    _chk(a)
    _chk(b)
    _chk(eps)
    assert a.shape == b.shape and eps.numel() == 1
    out = torch.empty_like(a)
    check(_lib.load().i3d_geomol_residual_fwd(_p(a), _p(b), _p(eps), a.shape[0], a.shape[1], _p(out), _stream()),
          'i3d_geomol_residual_fwd')
    return out


def geomol_residual_bwd(g, a, eps):
    """-> (da = (1 + eps) g, deps [1] = <g, a>, fp64 accumulation rounded once).  dL/db is g itself."""
    _chk(g)
    _chk(a)
    _chk(eps)
    assert g.shape == a.shape and eps.numel() == 1
    da = torch.empty_like(g)
    deps = torch.empty(1, dtype=torch.float32, device=g.device)
    partials = torch.empty(GEOMOL_PARTIAL_FLOATS, dtype=torch.float32, device=g.device)
    check(_lib.load().i3d_geomol_residual_bwd(_p(g), _p(a), _p(eps), a.shape[0], a.shape[1], _p(partials), _p(da), _p(deps),
                                              _stream()), 'i3d_geomol_residual_bwd')
    return da, deps


# ---- local-global NT-Xent (csrc/localglobal.hip; called from losses._LocalGlobalFn) ---------------------------------------------------
LG_ROW_CHUNK = 256      # rows per first-stage workgroup of the column reduction of the backward pass (i3d_lg_row_chunk)
