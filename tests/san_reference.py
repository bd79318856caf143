"""SAN's edge attention (reference models/san.py:111-177) as a torch composition in any dtype, with autograd for the gradients, and
the seeded batches tests/test_gpu_san.py runs the kernels of csrc/san.hip on.  Edge tensors are in destination-sorted order."""
import importlib
import math

import numpy as np
import torch

graph = importlib.import_module('3dinfomax_amd.graph')
synth = importlib.import_module('3dinfomax_amd.synth')

NAMES = ('Q', 'K', 'V', 'Q2', 'K2', 'TE', 'TE2')
ABSENT_CODE = 37
NUM_CODES = 60


def attention(t, idx, nh, gamma, full_graph):
    """t: {'Q','K','V','Q2','K2' [N, H], 'TE','TE2' [V, H]} -> (out [N, H], s [E, nh]); idx: {'src','dst','code' int64, 'real' bool}"""
    src, dst, code, real = idx['src'], idx['dst'], idx['code'], idx['real']
    N, H = t['Q'].shape
    E, dh = src.shape[0], H // nh
    if full_graph:
        sel = real[:, None]
        prod = torch.where(sel, t['K'][src] * t['Q'][dst] * t['TE'][code], t['K2'][src] * t['Q2'][dst] * t['TE2'][code])
        coef = torch.where(real, 1.0 / (gamma + 1.0), gamma / (gamma + 1.0)).to(prod.dtype)[:, None]
    else:
        prod = t['K'][src] * t['Q'][dst] * t['TE'][code]
        coef = 1.0
    s = prod.view(E, nh, dh).sum(-1) / math.sqrt(dh)
    w = torch.exp(s.clamp(-5, 5)) * coef
    wV = torch.zeros(N, nh, dh, dtype=prod.dtype).index_add_(0, dst, t['V'][src].view(E, nh, dh) * w[:, :, None])
    z = torch.zeros(N, nh, dtype=prod.dtype).index_add_(0, dst, w)
    return (wV / (z[:, :, None] + 1e-6)).reshape(N, H), s


def run(t, g, idx, nh, gamma, full_graph, dtype):
    """-> {'out', 's', 'dQ', ..., 'dTE2'} of the composition in `dtype` (CPU)"""
    names = NAMES if full_graph else ('Q', 'K', 'V', 'TE')
    x = {k: t[k].detach().to(dtype).requires_grad_() for k in names}
    out, s = attention(x, idx, nh, gamma, full_graph)
    out.backward(g.to(dtype))
    res = {'out': out.detach(), 's': s.detach()}
    res.update({'d' + k: x[k].grad for k in names})
    return res


def complete_batch(sizes):
    """complete graphs without self loops, block-diagonal -> (src, dst, num_nodes) in edge-id order"""
    srcs, dsts, off = [], [], 0
    for n in sizes:
        s, d = synth.complete_graph_edges(n)
        srcs.append(s + off)
        dsts.append(d + off)
        off += n
    return np.concatenate(srcs), np.concatenate(dsts), off


def chain_batch(sizes):
    """bond-like: chains with both directions and a ring closure on the longer ones; a size-1 entry is an isolated node"""
    srcs, dsts, off = [], [], 0
    for n in sizes:
        a = np.arange(n - 1)
        s, d = np.concatenate([a, a + 1]), np.concatenate([a + 1, a])
        if n > 4:
            s, d = np.concatenate([s, [0, n - 1, 2, n - 2]]), np.concatenate([d, [n - 1, 0, n - 2, 2]])
        srcs.append(s + off)
        dsts.append(d + off)
        off += n
    return np.concatenate(srcs).astype(np.int64), np.concatenate(dsts).astype(np.int64), off


def make_case(H, nh, full_graph, seed, scale):
    """-> (tensors fp32 {Q..TE2}, g [N, H], idx (CPU, destination-sorted), index (graph.GraphIndex, CPU), N).  60 codes: ABSENT_CODE on
    no edge, code 0 on 95 % of the fake edges; the real edges are those between consecutive nodes of a molecule (complete batch).
    `scale` multiplies Q, K and the tables: the share of saturated scores."""
    rng = np.random.default_rng(seed)
    if full_graph:
        src, dst, N = complete_batch((1, 2, 3, 17, 33, 70))
        real = np.abs(src - dst) == 1
    else:
        src, dst, N = chain_batch((1, 2, 5, 9, 30))
        real = np.ones(src.shape[0], bool)
    index = graph.build_index(src, dst, N, [N])
    perm = index.perm.long().numpy()
    E = src.shape[0]
    allowed = np.array([c for c in range(NUM_CODES) if c != ABSENT_CODE])
    code = rng.choice(allowed, size=E)
    if full_graph:
        code = np.where(~real & (rng.random(E) < 0.95), 0, code)
    idx = {'src': torch.from_numpy(src[perm]), 'dst': torch.from_numpy(dst[perm]), 'code': torch.from_numpy(code[perm]),
           'real': torch.from_numpy(real[perm])}
    g = torch.Generator().manual_seed(seed)
    t = {k: torch.randn(N, H, generator=g) * (scale if k in ('Q', 'K', 'Q2', 'K2') else 1.0) for k in ('Q', 'K', 'V', 'Q2', 'K2')}
    t['TE'] = torch.randn(NUM_CODES, H, generator=g) * scale
    t['TE2'] = torch.randn(NUM_CODES, H, generator=g) * scale
    grad = torch.randn(N, H, generator=g)
    _clear_clamp_edges(t, idx, nh, full_graph)
    return t, grad, idx, index, N


def _clear_clamp_edges(t, idx, nh, full_graph, margin=2e-3):
    """With tens of thousands of scores some always land within 1e-3 of +-5, where the clamp's gradient is implementation-defined:
    the source's K (K2) slice of that head is stretched by 1 % until none is left within `margin` (a stretch moves the source's
    other scores of the head as well, so the pass repeats; it ends after a few rounds)."""
    dh = t['Q'].shape[1] // nh
    for _ in range(100):
        with torch.no_grad():
            s = attention({k: v.double() for k, v in t.items()}, idx, nh, 0.5, full_graph)[1]
        bad = ((s.abs() - 5).abs() <= margin).nonzero()
        if bad.shape[0] == 0:
            return
        for e, a in bad.tolist():
            name = 'K' if (not full_graph or bool(idx['real'][e])) else 'K2'
            t[name][int(idx['src'][e]), a * dh:(a + 1) * dh] *= 1.01
    raise AssertionError('scores on the clamp edge remain')


# (H, heads) -> the scale at which 10-40 % of the scores saturate and none lies within 1e-3 of +-5, with the seed that gives it
# (checked on the host by tests/test_san_cpu.py::test_kernel_cases_saturate_as_stated, asserted again on the device's fp64 reference)
SHAPES = ((64, 4), (24, 3), (8, 1), (200, 10))
