"""The pair heads of the distance models (DistancePredictor, Net3DAE): autograd functions over the ordered atom pairs of a pair
graph, described by its kernel index (graph.GraphIndex; destination-sorted order, per-node sums as segment sums - fixed order,
no atomics).

  _PairSumHeadFn          distance_net of one Linear: u = (W_a + W_b) h per node, then softplus(u_i + u_j + 2b) per pair
  _PairNormFn             ||p_i - p_j||
  _PairConcatFn, _SoftplusSumToPairsFn   the composed form of a deeper distance_net: the [P, 2H] concatenations of both orders,
                          the MLP on each, softplus of the sum
  _PairMLPHeadFn          distance_net of two layers (Linear -> ReLU -> BatchNorm -> Linear(D -> 1)) fused: csrc/pairmlp.hip
"""
import torch

from . import ops
from .graph import as_batched_graph, build_index


def pair_index(pairwise_indices, graph):
    """The kernel index (graph.GraphIndex) of the pair graph whose edges are `pairwise_indices` [2, P] over the nodes of `graph`.
    A batch assembled on the device (dataset.FlatMolDataset.assemble_distance) carries it; otherwise it is built once on the
    host and kept on the tensor."""
    idx = getattr(pairwise_indices, '_i3d_pair_index', None)
    if idx is None:
        g = as_batched_graph(graph)
        pi = pairwise_indices.detach().cpu().numpy()
        idx = build_index(pi[0], pi[1], g.number_of_nodes(), g.batch_num_nodes().cpu().numpy()).to(pairwise_indices.device)
        pairwise_indices._i3d_pair_index = idx
    return idx


class _PairSumHeadFn(torch.autograd.Function):
    """softplus(f([h_i|h_j]) + f([h_j|h_i])) for f = Linear(2H -> T), W = [W_a | W_b]: u = h W_a^T + h W_b^T, then the pair kernel"""

    @staticmethod
    def forward(ctx, h, W, b, pidx):
        h = h.contiguous()
        H = h.shape[1]
        u = ops.gemm(h, W[:, :H], trans_b=True)
        ops.gemm(h, W[:, H:], trans_b=True, out=u, accumulate=True)
        ctx.pidx = pidx
        ctx.save_for_backward(h, W, b, u)
        return ops.pair_sum_fwd(u, b, pidx)

    @staticmethod
    def backward(ctx, grad_out):
        h, W, b, u = ctx.saved_tensors
        H = h.shape[1]
        du = ops.pair_sum_bwd(grad_out.contiguous(), u, b, ctx.pidx)
        gW = torch.empty_like(W)
        ops.gemm(du, h, trans_a=True, out=gW[:, :H])
        ops.gemm(du, h, trans_a=True, out=gW[:, H:])
        gb = ops.colsum(du)           # sum over nodes of du = 2 x sum over pairs: d(2b)/db
        gh = ops.gemm(du, W[:, :H])
        ops.gemm(du, W[:, H:], out=gh, accumulate=True)
        return gh, gW, gb, None


class _PairNormFn(torch.autograd.Function):
    """||p_i - p_j||_2 per pair, [P, 1]"""

    @staticmethod
    def forward(ctx, p, pidx):
        p = p.contiguous()
        d = ops.pair_norm_fwd(p, pidx)
        ctx.pidx = pidx
        ctx.save_for_backward(p, d)
        return d

    @staticmethod
    def backward(ctx, grad_out):
        p, d = ctx.saved_tensors
        return ops.pair_norm_bwd(grad_out.contiguous(), p, d, ctx.pidx), None


class _PairConcatFn(torch.autograd.Function):
    """[h_a | h_b] per pair in the pair graph's epos order: (a, b) = (src, dst), or (dst, src) with `swap` (segment sums of one row)"""

    @staticmethod
    def forward(ctx, h, pidx, swap):
        h = h.contiguous()
        P, H = pidx.num_edges, h.shape[1]
        one = _ranges(P, h.device)
        out = torch.empty(P, 2 * H, dtype=torch.float32, device=h.device)
        first, second = (pidx.dst_s, pidx.src_s) if swap else (pidx.src_s, pidx.dst_s)
        ops.segment_sum(h, one, first, P, out=out[:, :H])
        ops.segment_sum(h, one, second, P, out=out[:, H:])
        ctx.cfg = (pidx, swap, H)
        return out

    @staticmethod
    def backward(ctx, g):
        pidx, swap, H = ctx.cfg
        g = g.contiguous()
        gs, gd = (g[:, H:], g[:, :H]) if swap else (g[:, :H], g[:, H:])
        return ops._pair_node_sums(gs, gd, pidx), None, None


class _SoftplusSumToPairsFn(torch.autograd.Function):
    """softplus(a + b), rows permuted from the pair graph's epos order to pair-id order"""

    @staticmethod
    def forward(ctx, a, b, pidx):
        x = ops.add(a.contiguous(), b.contiguous())
        ctx.pidx = pidx
        ctx.save_for_backward(x)
        return ops.gather_rows(ops.act_fwd(x, 'softplus'), pidx.inv_perm)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        ge = ops.act_bwd(ops.gather_rows(g.contiguous(), ctx.pidx.perm), x, 'softplus')
        return ge, ge, None


_ranges_cache = {}


def _ranges(n, device):
    """int32 [0, 1, ..., n]: the row pointer of n one-row segments"""
    key = (n, str(device))
    t = _ranges_cache.get(key)
    if t is None:
        if len(_ranges_cache) > 64:
            _ranges_cache.clear()
        t = _ranges_cache[key] = torch.arange(n + 1, dtype=torch.int32, device=device)
    return t


class _PairMLPHeadFn(torch.autograd.Function):
    """softplus(f([h_s | h_d]) + f([h_d | h_s])) for f = FCLayer(2H -> D, ReLU, BatchNorm) -> FCLayer(D -> 1), each call with its own
    batch statistics (reference models/net3d_VAE.py:116-119).  W1 = [W1a | W1b]: A = h W1a^T and B = h W1b^T on the GEMM, the rest in
    the pair kernels of csrc/pairmlp.hip, which write [P, 1] and never a [P, 2H] or [P, D] tensor.  `bn` is the first layer's
    layers.BNSpec: training mode updates the running statistics twice (s->d first) and adds 2 to num_batches_tracked."""

    @staticmethod
    def forward(ctx, h, W1, b1, gamma, beta, W2, b2, pidx, bn):
        h = h.contiguous()
        H, D = h.shape[1], W1.shape[0]
        if bn.training and pidx.num_edges == 1:
            raise ValueError('distance_net: BatchNorm in training mode needs more than one pair')
        AB = torch.empty(h.shape[0], 2 * D, dtype=torch.float32, device=h.device)
        ops.gemm(h, W1[:, :H], trans_b=True, out=AB[:, :D])
        ops.gemm(h, W1[:, H:], trans_b=True, out=AB[:, D:])
        w2 = W2.reshape(-1)
        nbt = bn.num_batches_tracked
        out, stats, coef = ops.pair_mlp_fwd(AB, b1, gamma, beta, w2, b2, pidx, bn.training, bn.eps, bn.momentum, bn.running_mean,
                                      bn.running_var, nbt)
        if bn.training and nbt is not None and not nbt.is_cuda:
            nbt.add_(2)
        ctx.cfg = (pidx, bn.training)
        ctx.save_for_backward(h, W1, b1, gamma, beta, W2, AB, stats, coef)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, W1, b1, gamma, beta, W2, AB, stats, coef = ctx.saved_tensors
        pidx, training = ctx.cfg
        H, D = h.shape[1], W1.shape[0]
        if pidx.num_edges == 0:
            z = torch.zeros
            return (z(h.shape, device=h.device), z(W1.shape, device=h.device), z(D, device=h.device), z(D, device=h.device),
                    z(D, device=h.device), z(W2.shape, device=h.device), z(1, device=h.device), None, None)
        gAB, gg, gb, gw2, gb2 = ops.pair_mlp_bwd(grad_out.contiguous(), AB, b1, gamma, beta, W2.reshape(-1), stats, coef,
                                                 pidx, training)
        gW1 = torch.empty_like(W1)
        ops.gemm(gAB[:, :D], h, trans_a=True, out=gW1[:, :H])
        ops.gemm(gAB[:, D:], h, trans_a=True, out=gW1[:, H:])
        gb1 = ops.colsum(gAB)[:D]          # sum over nodes of dA = sum over pairs of (d pre1 + d pre2)
        gh = ops.gemm(gAB[:, :D], W1[:, :H])
        ops.gemm(gAB[:, D:], W1[:, H:], out=gh, accumulate=True)
        return gh, gW1, gb1, gg, gb, gw2.view_as(W2), gb2, None, None
