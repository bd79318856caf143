"""NT-Xent losses on the MI355X kernels - drop-in for `NTXent` / `NTXentMultiplePositives` of reference
commons/losses.py:126-163, 206-258 (same constructor kwargs, `forward(z1, z2, **kwargs) -> 0-dim tensor`).

Data parallel (absent in the reference, required by BASELINE.json:north_star): when a process group is
attached (`loss.attach_group(group)` or 3dinfomax_amd.dist.setup), z2 - the 3D-view embeddings - is
all-gathered over RCCL so each local 2D row sees the FULL negative set; the backward of the gather is a
reduce-scatter of dz2.  The returned value is this rank's share  sum_local(l_i) / B_global; the shares sum to
the reference's loss (dist.global_loss all-reduces it for logging).
"""
import torch
from torch import Tensor
from torch.nn.modules.loss import _Loss

import os

from . import _lib, ops

# I3D_LOSS_COMPOSITE=0: the loss as ~5 C calls per direction sequenced from Python (same kernels, same bits)
LOSS_COMPOSITE = os.environ.get('I3D_LOSS_COMPOSITE', '1') != '0'


class _AllGatherRowsFn(torch.autograd.Function):
    """all_gather along dim 0; backward = reduce_scatter(sum) of the gathered gradient.  `counts` (rows per rank, known on
    every rank) allows shards of different sizes (dist.shard_plan does not drop the remainder of a batch)."""

    @staticmethod
    def forward(ctx, x, group, counts=None):
        from . import dist as adist
        ctx.group, ctx.counts = group, counts
        if counts is not None:
            return adist.all_gather_rows_var(x, counts, group)
        return adist.all_gather_rows(x, group)

    @staticmethod
    def backward(ctx, g):
        from . import dist as adist
        if ctx.counts is not None:
            return adist.reduce_scatter_rows_var(g, ctx.counts, ctx.group), None, None
        return adist.reduce_scatter_rows(g, ctx.group), None, None


class NTXentFn(torch.autograd.Function):
    """loss_share = sum_i -log(pos_i / (rowsum_i - pos_i)) / global_batch  over the local rows of z1."""

    @staticmethod
    def forward(ctx, z1, z2, tau, eps, conf, pos_offset, global_batch, norm=True):
        z1, z2 = z1.contiguous(), z2.contiguous()
        b1, b2 = z1.shape[0], z2.shape[0] // conf
        ctx.norm = norm
        if not norm:
            # reference commons/losses.py:147-150 / :236-239 skipped: the same kernels with unit norms and no epsilon;
            # the backward then has no norm term (the row_axpy corrections)
            n1 = torch.ones(z1.shape[0], dtype=torch.float32, device=z1.device)
            n2 = torch.ones(z2.shape[0], dtype=torch.float32, device=z2.device)
            sim = ops.gemm(z1, z2, trans_b=True)
            row_sum, row_pos, loss = ops.ntxent_fwd(sim, n1, n2, b1, b2, conf, pos_offset, tau, 0.0, 1.0 / global_batch)
            ctx.cfg = (tau, 0.0, conf, pos_offset, global_batch, b1, b2)
            ctx.composite = False
            ctx.save_for_backward(z1, z2, n1, n2, sim, row_sum, row_pos)
            return loss.reshape(())
        if LOSS_COMPOSITE and z1.is_cuda and z1.dtype == torch.float32 and z2.dtype == torch.float32:
            # row norms, similarity GEMM (MFMA) and the fused exp / row-sum / log kernel from ONE C call (csrc/ntxent.hip)
            L = _lib.load()
            scratch = torch.empty(L.i3d_ntxent_loss_scratch_floats(b1, b2 * conf), dtype=torch.float32, device=z1.device)
            loss = torch.empty(1, dtype=torch.float32, device=z1.device)
            _lib.check(L.i3d_ntxent_loss_fwd(z1.data_ptr(), z2.data_ptr(), b1, b2, conf, z1.shape[1], pos_offset, float(tau),
                                             float(eps), 1.0 / global_batch, scratch.data_ptr(), loss.data_ptr(), ops._stream()),
                       'i3d_ntxent_loss_fwd')
            ctx.cfg = (tau, eps, conf, pos_offset, global_batch, b1, b2)
            ctx.composite = True
            ctx.save_for_backward(z1, z2, scratch)
            return loss.reshape(())
        n1, n2 = ops.row_norms(z1), ops.row_norms(z2)
        sim = ops.gemm(z1, z2, trans_b=True)                      # [b1, b2*conf] on the MFMA GEMM
        row_sum, row_pos, loss = ops.ntxent_fwd(sim, n1, n2, b1, b2, conf, pos_offset, tau, eps, 1.0 / global_batch)
        ctx.cfg = (tau, eps, conf, pos_offset, global_batch, b1, b2)
        ctx.composite = False
        ctx.save_for_backward(z1, z2, n1, n2, sim, row_sum, row_pos)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        tau, eps, conf, pos_offset, global_batch, b1, b2 = ctx.cfg
        if ctx.composite:
            z1, z2, scratch = ctx.saved_tensors
            L = _lib.load()
            b2c = b2 * conf
            work = torch.empty(b1 * b2c + b1 + b2c + 12, dtype=torch.float32, device=z1.device)
            dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
            gs = grad_out.contiguous().float()
            _lib.check(L.i3d_ntxent_loss_bwd(z1.data_ptr(), z2.data_ptr(), b1, b2, conf, z1.shape[1], pos_offset, float(tau),
                                             float(eps), 1.0 / global_batch, scratch.data_ptr(), gs.data_ptr(), work.data_ptr(),
                                             dz1.data_ptr(), dz2.data_ptr(), ops._stream()), 'i3d_ntxent_loss_bwd')
            return dz1, dz2, None, None, None, None, None, None
        z1, z2, n1, n2, sim, row_sum, row_pos = ctx.saved_tensors
        # the upstream scalar gradient is multiplied in on the device (no host read-back, no extra elementwise op)
        dsim, ca, cb = ops.ntxent_bwd(sim, n1, n2, row_sum, row_pos, b1, b2, conf, pos_offset, tau, eps,
                                      1.0 / global_batch, grad_out.contiguous().float())
        dz1 = ops.gemm(dsim, z2)                                  # dS z2
        dz2 = ops.gemm(dsim, z1, trans_a=True)                    # dS^T z1
        if ctx.norm:
            ops.row_axpy(z1, ca, dz1)
            ops.row_axpy(z2, cb, dz2)
        return dz1, dz2, None, None, None, None, None, None


class _GramFn(torch.autograd.Function):
    """x x^T (rows=True: [n, n]) or x^T x ([d, d]) through the library's GEMM (csrc/gemm.hip) - the matrix products of the
    regularisers below stay on the hand-written kernels; d(G)/dx = (dG + dG^T) x  resp.  x (dG + dG^T)."""

    @staticmethod
    def forward(ctx, x, rows):
        x = x.contiguous()
        ctx.rows = rows
        ctx.save_for_backward(x)
        return ops.gemm(x, x, trans_b=True) if rows else ops.gemm(x, x, trans_a=True)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gs = (g + g.transpose(0, 1)).contiguous()
        return (ops.gemm(gs, x) if ctx.rows else ops.gemm(x, gs)), None


def _gram(x, rows):
    if x.is_cuda and x.dtype == torch.float32 and x.dim() == 2:
        return _GramFn.apply(x, rows)
    return x @ x.T if rows else x.T @ x          # (CPU tensors: the host-logic tests)


# Optional regularisers (weights 0 in every BASELINE config): differentiable torch expressions around the library's GEMM for
# their matrix products.  Semantics of reference commons/losses.py:946-964.
def _log_mean_gaussian_potential(x, t):
    """log of the mean of exp(-t |x_i - x_j|^2) over all unordered pairs i < j.  The distances come from the Gram matrix of the rows
    with the column mean removed: they do not depend on a common translation, but g_ii + g_jj - 2 g_ij of the raw rows loses every
    digit once the mean exceeds the spread (embeddings with an offset, a collapsing batch).  The centring is part of the graph, so
    autograd carries its adjoint (g - mean(g))."""
    n = x.shape[0]
    x = x - x.mean(dim=0, keepdim=True)
    sq = (x * x).sum(dim=1)
    d2 = (sq[:, None] + sq[None, :] - 2.0 * _gram(x, True)).clamp_min(0.0)
    iu = torch.triu_indices(n, n, offset=1, device=x.device)
    return torch.exp(-t * d2[iu[0], iu[1]]).mean().log()


def uniformity_loss(x1: Tensor, x2: Tensor, t=2) -> Tensor:
    """mean of the two views' uniformity terms (Wang & Isola), reference :946-951"""
    return 0.5 * (_log_mean_gaussian_potential(x1, t) + _log_mean_gaussian_potential(x2, t))


def cov_loss(x):
    """sum of squared off-diagonal entries of the feature covariance, divided by the feature count (reference :954-959)"""
    n, dim = x.shape
    centred = x - x.mean(dim=0, keepdim=True)
    cov = _gram(centred, False) / (n - 1)
    off = cov - torch.diag_embed(torch.diagonal(cov))
    return (off * off).sum() / dim


def std_loss(x):
    """hinge on the per-feature standard deviation: mean(relu(1 - sqrt(var + 1e-4))) (reference :962-964)"""
    return torch.relu(1.0 - (x.var(dim=0) + 1e-4).sqrt()).mean()


class _NTXentBase(_Loss):
    _eps = 1e-8

    def __init__(self, norm: bool = True, tau: float = 0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0):
        super().__init__()
        self.norm, self.tau = norm, tau
        self.uniformity_reg, self.variance_reg, self.covariance_reg = uniformity_reg, variance_reg, covariance_reg
        self.group = None
        self.shard_counts = None
        self._equal_checked = {}       # local row count -> True once this rank has READ a check of that count (see _check_equal_shards)
        self._pending = None           # (result of the last equal-shard all-reduce, event of its pinned copy, local rows)
        self._pinned = None

    def attach_group(self, group):
        """Enable the data-parallel form (all-gathered negatives) on a torch.distributed process group."""
        self.group = group
        return self

    def set_shard_counts(self, counts):
        """molecules per rank of the current global batch when they differ (dist.shard_counts / shard_plan); None: equal"""
        self.shard_counts = list(counts) if counts is not None else None
        return self

    def _check_equal_shards(self, z1, dist):
        """Equal shards are ASSUMED when no counts were given (all_gather_into_tensor / reduce_scatter_tensor with different row
        counts per rank hang or corrupt silently) - e.g. the last partial batch of an epoch sharded with the remainder kept.
        EVERY call issues the same 2-element MAX all-reduce on every rank (whether a collective runs must never depend on
        rank-local state: a rank that has seen this row count before and one that has not would otherwise issue different
        collectives).  What IS rank-local is only when the result is read: at once for a row count this rank has not verified
        yet and on host-side backends (gloo: the result is already there), otherwise - the steady state, no host
        synchronisation in the step - through a pinned copy examined at the start of the next call.  A rank whose count is new
        raises before its gather; a rank whose count it knew raises one call later."""
        self._raise_if_unequal(block=True)          # the previous call's result: long finished, costs no wait
        rows = z1.shape[0]
        host_side = dist.get_backend(self.group) == 'gloo'
        n = torch.tensor([rows, -rows], dtype=torch.float64, device='cpu' if host_side else z1.device)
        dist.all_reduce(n, op=dist.ReduceOp.MAX, group=self.group)
        if host_side:
            self._pending = (n, None, rows)
        else:
            if self._pinned is None:
                self._pinned = torch.empty(2, dtype=torch.float64).pin_memory()
            self._pinned.copy_(n, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending = (self._pinned, ev, rows)
        if host_side or rows not in self._equal_checked:
            self._raise_if_unequal(block=True)
            self._equal_checked[rows] = True

    def _raise_if_unequal(self, block):
        if self._pending is None:
            return
        n, ev, rows = self._pending
        if ev is not None:
            if not block and not ev.query():
                return
            ev.synchronize()
        self._pending = None
        if float(n[0]) != -float(n[1]):
            raise ValueError(f'ranks hold different numbers of molecules ({rows} here, {int(-float(n[1]))}..'
                             f'{int(float(n[0]))} over the group): pass them with loss.set_shard_counts(dist.shard_counts(...))')

    def _valid_shard_counts(self, rows, world, rank):
        """the counts of set_shard_counts (None: equal shards), refused when they do not describe this rank's batch"""
        counts = self.shard_counts
        if counts is not None and (len(counts) != world or counts[rank] != rows):
            raise ValueError(f'shard counts {counts} do not describe this batch ({rows} rows on rank {rank})')
        return counts

    def _contrastive(self, z1, z2, conf):
        z2, pos_offset, global_batch = self._gathered(z1, z2, conf)
        return NTXentFn.apply(z1, z2, float(self.tau), float(self._eps), conf, pos_offset, global_batch, bool(self.norm))

    def _gathered(self, z1, z2, conf):
        """(z2 of the global batch, the column of this rank's first positive, the global batch size)"""
        pos_offset, global_batch = 0, z1.shape[0]
        if self.group is not None:
            import torch.distributed as dist
            world, rank = dist.get_world_size(self.group), dist.get_rank(self.group)
            if world > 1:
                counts = self._valid_shard_counts(z1.shape[0], world, rank)
                if counts is not None and max(counts) != min(counts):
                    z2 = _AllGatherRowsFn.apply(z2, self.group, [c * conf for c in counts])
                    pos_offset, global_batch = sum(counts[:rank]), sum(counts)
                else:
                    if counts is None:
                        self._check_equal_shards(z1, dist)
                    z2 = _AllGatherRowsFn.apply(z2, self.group)
                    pos_offset, global_batch = rank * z1.shape[0], world * z1.shape[0]
        return z2, pos_offset, global_batch

    def _regularisers(self, loss, z1, z2):
        if self.variance_reg > 0:
            loss = loss + self.variance_reg * (std_loss(z1) + std_loss(z2))
        if self.covariance_reg > 0:
            loss = loss + self.covariance_reg * (cov_loss(z1) + cov_loss(z2))
        if self.uniformity_reg > 0:
            loss = loss + self.uniformity_reg * uniformity_loss(z1, z2)
        return loss


class NTXent(_NTXentBase):
    """Normalized Temperature-scaled Cross Entropy Loss (reference commons/losses.py:126-163)."""
    _eps = 1e-8        # reference :150

    def forward(self, z1, z2, **kwargs) -> Tensor:
        return self._regularisers(self._contrastive(z1, z2, 1), z1, z2)


class NTXentMultiplePositives(_NTXentBase):
    """reference commons/losses.py:206-258; z2 is [batch*num_conformers, dim], conformer-minor; no epsilon (:239)."""
    _eps = 0.0

    def __init__(self, norm: bool = True, tau: float = 0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0,
                 conformer_variance_reg=0) -> None:
        super().__init__(norm, tau, uniformity_reg, variance_reg, covariance_reg)
        self.conformer_variance_reg = conformer_variance_reg

    def forward(self, z1, z2, **kwargs) -> Tensor:
        batch_size, metric_dim = z1.size()
        conf = z2.shape[0] // batch_size
        loss = self._contrastive(z1, z2, conf)
        z2v = z2.view(batch_size, -1, metric_dim)
        if self.variance_reg > 0:
            loss = loss + self.variance_reg * (std_loss(z1) + std_loss(z2v))
        if self.conformer_variance_reg > 0:       # the same hinge over the conformer axis
            loss = loss + self.conformer_variance_reg * torch.relu(1.0 - (z2v.var(dim=1) + 1e-4).sqrt()).mean()
        if self.covariance_reg > 0:
            loss = loss + self.covariance_reg * (cov_loss(z1) + cov_loss(z2v))
        if self.uniformity_reg > 0:
            loss = loss + self.uniformity_reg * uniformity_loss(z1, z2v)
        return loss


class _MSEFn(torch.autograd.Function):
    """weight * mean((a - b)^2) as a 0-dim tensor (csrc/pairmlp.hip: block partials summed in a fixed order; the upstream scalar
    gradient is multiplied in on the device)"""

    @staticmethod
    def forward(ctx, a, b, weight):
        a, b = a.contiguous().float(), b.contiguous().float()
        if a.shape != b.shape:
            raise ValueError(f'mean squared error of tensors shaped {tuple(a.shape)} and {tuple(b.shape)}')
        n = a.numel()
        ctx.scale = float(weight) / n if n else float('nan')
        ctx.save_for_backward(a, b)
        return ops.mse_fwd(a, b, ctx.scale).reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        a, b = ctx.saved_tensors
        ga, gb = ops.mse_bwd(a, b, ctx.scale, grad_out.contiguous().float(), ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return ga, gb, None


class NTXentAE(_NTXentBase):
    """reference commons/losses.py:165-204: forward(z1, z2, distances, distance_pred) -> (contrastive term with the regularisers,
    reconstruction_reg * mean squared error of the predicted pair distances).  Single process only: the global mean over pairs
    would need the global pair count."""
    _eps = 1e-8        # reference :191

    def __init__(self, norm: bool = True, tau: float = 0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0,
                 reconstruction_reg=1) -> None:
        super().__init__(norm, tau, uniformity_reg, variance_reg, covariance_reg)
        self.reconstruction_reg = reconstruction_reg

    def forward(self, z1, z2, distances, distance_pred, **kwargs):
        if self.group is not None:
            import torch.distributed as dist
            if dist.get_world_size(self.group) > 1:
                raise NotImplementedError('NTXentAE on a process group of more than one rank: the reconstruction term is a mean over '
                                          'the pairs of the global batch, which needs the global pair count')
        loss = self._regularisers(self._contrastive(z1, z2, 1), z1, z2)
        return loss, _MSEFn.apply(distances, distance_pred, self.reconstruction_reg)


# ---- one 2D embedding per conformer (csrc/sep2d.hip) ---------------------------------------------------------------------------------
def _separate2d_shapes(name, z1, z2):
    """(B, C, D) of z1 [B, C D] and z2 [B C, D]; everything that cannot be viewed that way is refused before any device work"""
    if z1.dim() != 2 or z2.dim() != 2:
        raise ValueError(f'{name}: z1 [batch, conformers * dim] and z2 [batch * conformers, dim] expected, got '
                         f'{tuple(z1.shape)} and {tuple(z2.shape)}')
    B, D = z1.shape[0], z2.shape[1]
    if B < 1 or z2.shape[0] % B != 0:
        raise ValueError(f'{name}: the {z2.shape[0]} rows of z2 are not a multiple of the batch size {B}')
    C = z2.shape[0] // B
    if z1.shape[1] != C * D:
        raise ValueError(f'{name}: z1 has {z1.shape[1]} columns, {C} conformers of dimension {D} need {C * D}')
    if C < 1 or C > ops.SEP2D_MAX_CONFORMERS:
        raise NotImplementedError(f'{name}: {C} conformers per molecule, the kernels are built for 1..{ops.SEP2D_MAX_CONFORMERS}')
    if B < 2:
        raise ValueError(f'{name}: a batch of {B} has no negatives')
    if z1.dtype != torch.float32 or z2.dtype != torch.float32:
        raise NotImplementedError(f'{name}: fp32 only, got {z1.dtype} and {z2.dtype}')
    return B, C, D


class _RowNormalizeFn(torch.autograd.Function):
    """F.normalize(x, dim=1) of a [rows, dim] matrix, 1e-12 clamp included"""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y, n = ops.row_normalize_fwd(x)
        ctx.save_for_backward(x, n)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, n = ctx.saved_tensors
        return ops.row_normalize_bwd(x, n, grad_y.contiguous())


class _Separate2DFn(torch.autograd.Function):
    """-mean_i log(pos_i / den_i) from the [B C, B C] similarity of the conformer-wise 2D embeddings z1v and the 3D embeddings z2"""

    @staticmethod
    def forward(ctx, z1v, z2, batch, conf, tau, norm):
        z1v, z2 = z1v.contiguous(), z2.contiguous()
        if norm:
            n1, n2 = ops.row_norms(z1v), ops.row_norms(z2)
        else:
            n1 = n2 = torch.ones(z1v.shape[0], dtype=torch.float32, device=z1v.device)
        sim = ops.gemm(z1v, z2, trans_b=True)
        row_den, row_pos, loss = ops.sep2d_fwd(sim, n1, n2, batch, conf, tau)
        ctx.cfg = (batch, conf, tau, norm)
        ctx.save_for_backward(z1v, z2, n1, n2, sim, row_den, row_pos)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        batch, conf, tau, norm = ctx.cfg
        z1v, z2, n1, n2, sim, row_den, row_pos = ctx.saved_tensors
        dsim, ca, cb = ops.sep2d_bwd(sim, n1, n2, row_den, row_pos, batch, conf, tau, grad_out.contiguous().float())
        dz1 = ops.gemm(dsim, z2)
        dz2 = ops.gemm(dsim, z1v, trans_a=True)
        if norm:
            ops.row_axpy(z1v, ca, dz1)
            ops.row_axpy(z2, cb, dz2)
        return dz1, dz2, None, None, None, None


class _MMDNTXentFn(torch.autograd.Function):
    """NT-Xent over sim[a, b] = 1 / (mmd(conformers of x[b], conformers of y[a]) + 1); x the 2D view, y the 3D view, both [B C, D].
    The kernel bandwidths are constants of the backward pass, as in the reference (computed from .data)."""

    @staticmethod
    def forward(ctx, x, y, batch, conf, tau, kernel_num, kernel_mul):
        x, y = x.contiguous(), y.contiguous()
        sim, bandwidth, cross, intra = ops.mmd_pair_fwd(x, y, batch, conf, kernel_num, kernel_mul)
        ones = torch.ones(batch, dtype=torch.float32, device=x.device)
        row_sum, row_pos, loss = ops.ntxent_fwd(sim, ones, ones, batch, batch, 1, 0, tau, 0.0, 1.0 / batch)
        ctx.cfg = (batch, conf, tau, kernel_num, kernel_mul)
        ctx.save_for_backward(x, y, sim, bandwidth, cross, intra, ones, row_sum, row_pos)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        batch, conf, tau, kernel_num, kernel_mul = ctx.cfg
        x, y, sim, bandwidth, cross, intra, ones, row_sum, row_pos = ctx.saved_tensors
        dsim, _, _ = ops.ntxent_bwd(sim, ones, ones, row_sum, row_pos, batch, batch, 1, 0, tau, 0.0, 1.0 / batch,
                                    grad_out.contiguous().float())
        dx, dy = ops.mmd_pair_bwd(x, y, cross, intra, bandwidth, sim, dsim, batch, conf, kernel_num, kernel_mul)
        return dx, dy, None, None, None, None, None


class _Separate2DBase(_NTXentBase):
    _data_parallel = False          # True: the class has a data-parallel form of its own

    def _refuse_unsupported(self):
        """before any device work: the data-parallel form (where the class has none), and the regularisers the reference itself cannot
        apply - it hands them the 3-D views, where cov_loss fails to unpack a 2-D shape and the torch.pdist of uniformity_loss takes
        2-D input only"""
        name = type(self).__name__
        if not self._data_parallel and self.group is not None:
            import torch.distributed as dist
            if dist.get_world_size(self.group) > 1:
                raise NotImplementedError(f'{name} on a process group of more than one rank: the data-parallel form of the '
                                          'conformer-wise losses is not built')
        if self.covariance_reg > 0:
            raise NotImplementedError(f'{name}: covariance_reg > 0 - the reference\'s cov_loss unpacks a 2-D shape and raises on the '
                                      '3-D views this loss hands it')
        if self.uniformity_reg > 0:
            raise NotImplementedError(f'{name}: uniformity_reg > 0 - the reference\'s uniformity_loss (torch.pdist) raises on the '
                                      '3-D views this loss hands it')

    def _regularisers(self, loss, z1, z2):
        """the reference's calls on the 3-D views: std_loss works on them (variance over the batch axis per conformer and feature),
        the other two are refused"""
        self._refuse_unsupported()
        if self.variance_reg > 0:
            loss = loss + self.variance_reg * (std_loss(z1) + std_loss(z2))
        return loss


class NTXentMultiplePositivesSeparate2D(_Separate2DBase):
    """reference commons/losses.py:692-744: z1 [B, C D] holds one 2D embedding per conformer, z2 [B C, D] the 3D embeddings, molecule
    major.  Positives are the matched conformers only; the whole C x C block of the molecule leaves the denominator.  No epsilon."""

    def forward(self, z1, z2, **kwargs) -> Tensor:
        B, C, D = _separate2d_shapes(type(self).__name__, z1, z2)
        self._refuse_unsupported()
        loss = _Separate2DFn.apply(z1.reshape(B * C, D), z2, B, C, float(self.tau), bool(self.norm))
        return self._regularisers(loss, z1.view(B, C, D), z2.view(B, C, D))


class NTXentMMDSeparate2D(_Separate2DBase):
    """reference commons/losses.py:394-476: the similarity of molecules a (3D view, rows) and b (2D view, columns) is
    1 / (MMD + 1) of their two conformer sets under a sum of kernel_num Gaussian kernels; NT-Xent over that [B, B] matrix."""

    def __init__(self, norm: bool = True, tau: float = 0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0, kernel_num=5,
                 kernel_mul=2.0) -> None:
        super().__init__(norm, tau, uniformity_reg, variance_reg, covariance_reg)
        self.kernel_num, self.kernel_mul = kernel_num, kernel_mul
        self.fix_sigma = None

    def forward(self, z1, z2, **kwargs) -> Tensor:
        B, C, D = _separate2d_shapes(type(self).__name__, z1, z2)
        self._refuse_unsupported()
        x, y = z1.reshape(B * C, D), z2
        if self.norm:
            x, y = _RowNormalizeFn.apply(x), _RowNormalizeFn.apply(y)
        loss = _MMDNTXentFn.apply(x, y, B, C, float(self.tau), int(self.kernel_num), float(self.kernel_mul))
        return self._regularisers(loss, x.view(B, C, D), y.view(B, C, D))


# ---- set matching and per-conformer terms (csrc/confmatch.hip) ------------------------------------------------------------------------
class _ConfMatchFn(torch.autograd.Function):
    """-mean_i log(pos_i / den_i) where every molecule pair enters through ONE entry of its C x C block of the [B C, B C] similarity: the
    smallest (mode 0) or the largest (mode 1).  The backward pass gathers from those entries; the only [B C, B C] tensor is the
    similarity itself."""

    @staticmethod
    def forward(ctx, z1v, z2, batch, conf, tau, norm, mode):
        z1v, z2 = z1v.contiguous(), z2.contiguous()
        if norm:
            n1, n2 = ops.row_norms(z1v), ops.row_norms(z2)
        else:
            n1 = n2 = torch.ones(z1v.shape[0], dtype=torch.float32, device=z1v.device)
        sim = ops.gemm(z1v, z2, trans_b=True)
        sel, row_den, pos_j, pos_lu, loss = ops.conf_match_fwd(sim, n1, n2, batch, conf, mode, tau)
        ctx.cfg = (batch, conf, tau, norm, mode)
        ctx.save_for_backward(z1v, z2, n1, n2, sim, sel, row_den, pos_j, pos_lu)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        batch, conf, tau, norm, mode = ctx.cfg
        z1v, z2, n1, n2, sim, sel, row_den, pos_j, pos_lu = ctx.saved_tensors
        dz1, dz2 = ops.conf_match_bwd(sim, z1v, z2, n1, n2, sel, row_den, pos_j, pos_lu, batch, conf, mode, norm, tau,
                                      grad_out.contiguous().float())
        return dz1, dz2, None, None, None, None, None


class _PerConformerFn(torch.autograd.Function):
    """the V2 (mode 0) and V3 (mode 1) losses from the [B, B C] similarity of the 2D embeddings z1 and the 3D embeddings z2"""

    @staticmethod
    def forward(ctx, z1, z2, batch, conf, tau, norm, mode):
        z1, z2 = z1.contiguous(), z2.contiguous()
        if norm:
            n1, n2 = ops.row_norms(z1), ops.row_norms(z2)
        else:
            n1 = torch.ones(z1.shape[0], dtype=torch.float32, device=z1.device)
            n2 = torch.ones(z2.shape[0], dtype=torch.float32, device=z1.device)
        sim = ops.gemm(z1, z2, trans_b=True)
        den, pos, loss = ops.per_conf_fwd(sim, n1, n2, batch, conf, mode, tau)
        ctx.cfg = (batch, conf, tau, norm, mode)
        ctx.save_for_backward(z1, z2, n1, n2, sim, den, pos)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        batch, conf, tau, norm, mode = ctx.cfg
        z1, z2, n1, n2, sim, den, pos = ctx.saved_tensors
        dsim, ca, cb = ops.per_conf_bwd(sim, n1, n2, den, pos, batch, conf, mode, tau, grad_out.contiguous().float())
        dz1 = ops.gemm(dsim, z2)
        dz2 = ops.gemm(dsim, z1, trans_a=True)
        if norm:
            ops.row_axpy(z1, ca, dz1)
            ops.row_axpy(z2, cb, dz2)
        return dz1, dz2, None, None, None, None, None


class _ConfMatchBase(_Separate2DBase):
    _mode = None

    def forward(self, z1, z2, **kwargs) -> Tensor:
        B, C, D = _separate2d_shapes(type(self).__name__, z1, z2)
        self._refuse_unsupported()
        loss = _ConfMatchFn.apply(z1.reshape(B * C, D), z2, B, C, float(self.tau), bool(self.norm), ops.CONF_MATCH_MODES[self._mode])
        return self._regularisers(loss, z1.view(B, C, D), z2.view(B, C, D))


class NTXentMinimumMatching(_ConfMatchBase):
    """reference commons/losses.py:747-794: z1 [B, C D] holds one 2D embedding per conformer, z2 [B C, D] the 3D embeddings, molecule
    major.  The similarity of two molecules is the SMALLEST entry of their C x C block; the positive of molecule i is the largest
    matched entry s'[(i, l), (j, l)] over every column molecule j and every l - the reference's amax over the blocks' diagonals runs
    over j as well.  No epsilon.  A tie goes to the lowest index (torch splits its gradient evenly)."""
    _mode = 'min'


class NTXentMaximumSimilarity(_ConfMatchBase):
    """reference commons/losses.py:839-886: as NTXentMinimumMatching with the LARGEST entry of every C x C block; the positive of
    molecule i is the largest entry of its own block."""
    _mode = 'max'


def _per_conformer_shapes(name, z1, z2):
    """(B, C, D) of z1 [B, D] and z2 [B C, D]; everything else is refused before any device work"""
    if z1.dim() != 2 or z2.dim() != 2:
        raise ValueError(f'{name}: z1 [batch, dim] and z2 [batch * conformers, dim] expected, got {tuple(z1.shape)} and '
                         f'{tuple(z2.shape)}')
    B, D = z1.shape
    if z2.shape[1] != D:
        raise ValueError(f'{name}: z1 has {D} columns, z2 has {z2.shape[1]}')
    if B < 1 or z2.shape[0] % B != 0:
        raise ValueError(f'{name}: the {z2.shape[0]} rows of z2 are not a multiple of the batch size {B}')
    C = z2.shape[0] // B
    if C < 1 or C > ops.PER_CONF_MAX_CONFORMERS:
        raise NotImplementedError(f'{name}: {C} conformers per molecule, the kernels are built for 1..{ops.PER_CONF_MAX_CONFORMERS}')
    if B < 2:
        raise ValueError(f'{name}: a batch of {B} has no negatives')
    if z1.dtype != torch.float32 or z2.dtype != torch.float32:
        raise NotImplementedError(f'{name}: fp32 only, got {z1.dtype} and {z2.dtype}')
    return B, C, D


class _PerConformerBase(_Separate2DBase):
    _mode = None

    def forward(self, z1, z2, **kwargs) -> Tensor:
        B, C, D = _per_conformer_shapes(type(self).__name__, z1, z2)
        self._refuse_unsupported()
        loss = _PerConformerFn.apply(z1, z2, B, C, float(self.tau), bool(self.norm), ops.PER_CONF_MODES[self._mode])
        return self._regularisers(loss, z1, z2.view(B, C, D))


class NTXentMultiplePositivesV2(_PerConformerBase):
    """reference commons/losses.py:598-643: z1 [B, D], z2 [B C, D] molecule major.  pos_i = the sum over the molecule's C conformers,
    den_i = the sum over conformer 0 of every OTHER molecule - the reference builds its negatives from z2[:, 0] only.  No epsilon."""
    _mode = 'v2'


class NTXentMultiplePositivesV3(_PerConformerBase):
    """reference commons/losses.py:646-689: one NT-Xent term per (molecule, conformer): the positive is that conformer, the negatives
    are the same conformer index of every other molecule; the mean runs over the B C terms.  No epsilon."""
    _mode = 'v3'


# ---- the conformers as one diagonal Gaussian per molecule (csrc/klmp.hip) --------------------------------------------------------------
def _kl_shapes(name, z1, z2):
    """(B, C, D) of z1 [B, 2 D] (mean | log-variance) and z2 [B C, D]; everything else is refused before any device work"""
    if z1.dim() != 2 or z2.dim() != 2:
        raise ValueError(f'{name}: z1 [batch, 2 * dim] and z2 [batch * conformers, dim] expected, got {tuple(z1.shape)} and '
                         f'{tuple(z2.shape)}')
    B, D = z1.shape[0], z2.shape[1]
    if D < 1 or z1.shape[1] != 2 * D:
        raise ValueError(f'{name}: z1 has {z1.shape[1]} columns, a mean and a log-variance of dimension {D} need {2 * D}')
    if B < 1 or z2.shape[0] % B != 0:
        raise ValueError(f'{name}: the {z2.shape[0]} rows of z2 are not a multiple of the batch size {B}')
    C = z2.shape[0] // B
    if C < 2:
        raise ValueError(f'{name}: {C} conformer(s) per molecule - the variance over the conformers needs at least two')
    if z1.dtype != torch.float32 or z2.dtype != torch.float32:
        raise NotImplementedError(f'{name}: fp32 only, got {z1.dtype} and {z2.dtype}')
    return B, C, D


class _KLMultiplePositivesFn(torch.autograd.Function):
    """sum_b KL(N(m2_b, v2_b) || N(m1_b, exp(s1_b))) / global_batch over the local molecules; the backward pass recomputes the conformer
    statistics instead of keeping them"""

    @staticmethod
    def forward(ctx, z1, z2, batch, conf, global_batch):
        z1, z2 = z1.contiguous(), z2.contiguous()
        _, loss = ops.kl_mp_fwd(z1, z2, batch, conf, 1.0 / global_batch)
        ctx.cfg = (batch, conf, global_batch)
        ctx.save_for_backward(z1, z2)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        batch, conf, global_batch = ctx.cfg
        z1, z2 = ctx.saved_tensors
        dz1, dz2 = ops.kl_mp_bwd(z1, z2, batch, conf, 1.0 / global_batch, grad_out.contiguous().float())
        return dz1, dz2, None, None, None


class KLDivergenceMultiplePositives(_Separate2DBase):
    """reference commons/losses.py:261-314: z1 [B, 2 D] holds a mean and a log-variance per molecule, z2 [B C, D] the 3D embeddings of
    its C conformers, molecule major; the loss is the mean over the molecules of KL(N(mean_c z2, var_c z2 + 1e-6) || N(mean, exp(log-
    variance))).  No normalisation by default; `tau` is accepted and unused, as in the reference.  There are no negatives, so a batch of
    one is valid and the data-parallel form needs no gather: on a group of more than one rank the value is this rank's share
    sum_local kl_b / B_global (the convention of NTXent)."""
    _data_parallel = True

    def __init__(self, norm: bool = False, tau: float = 0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0) -> None:
        super().__init__(norm, tau, uniformity_reg, variance_reg, covariance_reg)

    def _global_batch(self, z1):
        if self.group is None:
            return z1.shape[0]
        import torch.distributed as dist
        world, rank = dist.get_world_size(self.group), dist.get_rank(self.group)
        if world == 1:
            return z1.shape[0]
        counts = self._valid_shard_counts(z1.shape[0], world, rank)
        if counts is not None:
            return sum(counts)
        self._check_equal_shards(z1, dist)
        return world * z1.shape[0]

    def forward(self, z1, z2, **kwargs) -> Tensor:
        B, C, D = _kl_shapes(type(self).__name__, z1, z2)
        self._refuse_unsupported()
        global_batch = self._global_batch(z1)
        a, b = z1.reshape(2 * B, D), z2
        if self.norm:
            a, b = _RowNormalizeFn.apply(a), _RowNormalizeFn.apply(b)
        loss = _KLMultiplePositivesFn.apply(a.reshape(B, 2 * D), b, B, C, global_batch)
        return self._regularisers(loss, a.view(B, 2, D), b.view(B, C, D))


# ---- the Gaussian of the 2D view against every molecule's conformers: [B, B] pair matrices (csrc/gausspair.hip) -------------------------------
def _gauss_pair_shapes(name, z1, z2, min_conf):
    """(B, C, D) of z1 [B, 2 D] (mean | log-variance) and z2 [B C, D]; everything else is refused before any device work"""
    if z1.dim() != 2 or z2.dim() != 2:
        raise ValueError(f'{name}: z1 [batch, 2 * dim] and z2 [batch * conformers, dim] expected, got {tuple(z1.shape)} and '
                         f'{tuple(z2.shape)}')
    B, D = z1.shape[0], z2.shape[1]
    if D < 1 or z1.shape[1] != 2 * D:
        raise ValueError(f'{name}: z1 has {z1.shape[1]} columns, a mean and a log-variance of dimension {D} need {2 * D}')
    if B < 1 or z2.shape[0] < B or z2.shape[0] % B != 0:
        raise ValueError(f'{name}: the {z2.shape[0]} rows of z2 are not a multiple of the batch size {B}')
    C = z2.shape[0] // B
    if C < min_conf:
        raise ValueError(f'{name}: {C} conformer(s) per molecule - the variance over the conformers needs at least two')
    if B < 2:
        raise ValueError(f'{name}: a batch of {B} has no negatives')
    if z1.dtype != torch.float32 or z2.dtype != torch.float32:
        raise NotImplementedError(f'{name}: fp32 only, got {z1.dtype} and {z2.dtype}')
    return B, C, D


class _LikelihoodFn(torch.autograd.Function):
    """mean_i (log sum_{j != i} exp(L_ij / tau) - L_ii / tau), L_ij = the mean density of molecule j's conformers under the Gaussian of
    molecule i; the backward pass keeps L [B, B] and the row terms and recomputes the densities"""

    @staticmethod
    def forward(ctx, z1, z2, batch, conf, tau):
        z1, z2 = z1.contiguous(), z2.contiguous()
        lik = ops.gauss_lik_fwd(z1, z2, batch, conf)
        rows, loss = ops.gauss_lik_loss(lik, tau)
        ctx.cfg = (batch, conf, tau)
        ctx.save_for_backward(z1, z2, lik, rows)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        batch, conf, tau = ctx.cfg
        z1, z2, lik, rows = ctx.saved_tensors
        dz1, dz2 = ops.gauss_lik_bwd(z1, z2, batch, conf, lik, rows, tau, grad_out.contiguous().float())
        return dz1, dz2, None, None, None


class NTXentLikelihoodLoss(_Separate2DBase):
    """reference commons/losses.py:537-595: z1 [B, 2 D] holds a mean and a log-variance per molecule, z2 [B C, D] the 3D embeddings of its C
    conformers, molecule major.  L_ij = the mean over conformers and features of the per-dimension normal densities of molecule j's
    conformers under molecule i's Gaussian; NT-Xent over exp(L / tau), rows i the 2D view.  The negatives are summed directly and the row
    maximum leaves the exponent, so the loss stays finite where the reference's `row sum - positive` rounds to zero.  `norm` is accepted
    and unused, as in the reference; C = 1 is valid."""

    def __init__(self, norm: bool = True, tau: float = 0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0,
                 conformer_variance_reg=0) -> None:
        super().__init__(norm, tau, uniformity_reg, variance_reg, covariance_reg)
        self.conformer_variance_reg = conformer_variance_reg

    def forward(self, z1, z2, **kwargs) -> Tensor:
        name = type(self).__name__
        B, C, D = _gauss_pair_shapes(name, z1, z2, 1)
        self._refuse_unsupported()
        if self.conformer_variance_reg > 0 and C < 2:
            raise ValueError(f'{name}: conformer_variance_reg > 0 with {C} conformer(s) per molecule - the variance over the conformers '
                             'needs at least two')
        loss = _LikelihoodFn.apply(z1, z2, B, C, float(self.tau))
        z2v = z2.reshape(B, C, D)
        loss = self._regularisers(loss, z1.reshape(B, 2, D), z2v)
        if self.conformer_variance_reg > 0:       # the hinge of NTXentMultiplePositives over the conformer axis
            loss = loss + self.conformer_variance_reg * torch.relu(1.0 - (z2v.var(dim=1) + 1e-4).sqrt()).mean()
        return loss


class _JSDFn(torch.autograd.Function):
    """-mean_a log(S_aa / sum_{b != a} S_ab), S_ab = KL(N(m2_a, v2_a) || N(m1_b, exp(s1_b))) with the reference's epsilons; the backward
    pass keeps two numbers per molecule and the row terms, and recomputes the conformer statistics"""

    @staticmethod
    def forward(ctx, z1, z2, batch, conf):
        z1, z2 = z1.contiguous(), z2.contiguous()
        astat, rows, loss = ops.gauss_jsd_fwd(z1, z2, batch, conf)
        ctx.cfg = (batch, conf)
        ctx.save_for_backward(z1, z2, astat, rows)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        batch, conf = ctx.cfg
        z1, z2, astat, rows = ctx.saved_tensors
        dz1, dz2 = ops.gauss_jsd_bwd(z1, z2, batch, conf, astat, rows, grad_out.contiguous().float())
        return dz1, dz2, None, None


class JSDMultiplePositivesLoss(_Separate2DBase):
    """reference commons/losses.py:317-391: z1 [B, 2 D] (mean | log-variance), z2 [B C, D] molecule major.  S[a, b] = 0.5 (log(prod v2_a +
    1e-5) - sum s_b - D + sum (exp(s_b) + (m2_a - m1_b)^2) / (v2_a + 1e-5)) with m2 / v2 the conformer mean / unbiased variance of molecule
    a (rows: the 3D view) - the reference's `kl_similarity2`; the loss is NT-Xent over S itself, not exponentiated: `tau` is accepted
    and unused, and a negative ratio gives NaN.  `sum s` stands for the reference's log of prod exp(s): the same wherever that product
    neither overflows nor underflows.  One deliberate deviation: identical conformers (v2 = 0) evaluate the formula; the reference raises
    there, from MultivariateNormal objects whose values it discards."""

    def forward(self, z1, z2, **kwargs) -> Tensor:
        B, C, D = _gauss_pair_shapes(type(self).__name__, z1, z2, 2)
        self._refuse_unsupported()
        a, b = z1.reshape(2 * B, D), z2
        if self.norm:
            a, b = _RowNormalizeFn.apply(a), _RowNormalizeFn.apply(b)
        loss = _JSDFn.apply(a.reshape(B, 2 * D), b, B, C)
        return self._regularisers(loss, a.view(B, 2, D), b.view(B, C, D))


# ---- fine-tuning on multi-task datasets with missing labels (csrc/task.hip) ---------------------------------------------------------------
def _masked_loss_shapes(name, pred, target):
    """[B, T] views of pred and target (1-D: [B, 1]); everything else is refused before any device work"""
    if not (torch.is_tensor(pred) and torch.is_tensor(target)) or tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f'{name}: pred and target of the same shape expected, got '
                         f'{tuple(pred.shape) if torch.is_tensor(pred) else type(pred).__name__} and '
                         f'{tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}')
    if pred.dim() not in (1, 2) or pred.numel() == 0:
        raise ValueError(f'{name}: [batch, tasks] (or [batch]) with at least one element expected, got {tuple(pred.shape)}')
    if pred.is_cuda != target.is_cuda:
        raise ValueError(f'{name}: pred is on {pred.device}, target on {target.device}')
    if pred.is_cuda and (pred.dtype != torch.float32 or target.dtype != torch.float32):
        raise NotImplementedError(f'{name}: fp32 only on the device, got {pred.dtype} and {target.dtype}')
    if pred.dim() == 1:
        return pred.reshape(-1, 1), target.reshape(-1, 1)
    return pred, target


def _masked_loss_host(pred, target, kind):
    """the same formula as a torch expression (CPU tensors: the host-logic tests).  torch.where on both sides of the product: a NaN or
    inf prediction at an unlabelled position reaches neither the value nor the gradient"""
    labelled = ~torch.isnan(target)
    x, t = torch.where(labelled, pred, torch.zeros_like(pred)), torch.where(labelled, target, torch.zeros_like(target))
    if kind == 0:
        # max(x, 0) - x t + log1p(exp(-|x|)) with the gradient sigmoid(x) - t (also at x = 0, where clamp and abs have kinks)
        term = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction='none')
    else:
        term = (x - t) ** 2
    return torch.where(labelled, term, torch.zeros_like(term)).sum() / labelled.sum()


class _MaskedLossFn(torch.autograd.Function):
    """mean over the labelled elements; the count stays on the device between the two passes (no host synchronisation)"""

    @staticmethod
    def forward(ctx, pred, target, kind):
        pred, target = pred.contiguous(), target.contiguous()
        out = ops.masked_loss_fwd(pred, target, kind)
        ctx.kind = kind
        ctx.save_for_backward(pred, target, out)
        return out.view(torch.float32)[4]

    @staticmethod
    def backward(ctx, grad_out):
        pred, target, out = ctx.saved_tensors
        return ops.masked_loss_bwd(pred, target, ctx.kind, out, grad_out.contiguous().float().reshape(1)), None, None


class _OGBNanLabelLoss(_Loss):
    _kind = None

    def forward(self, pred, target, **kwargs) -> Tensor:
        p, t = _masked_loss_shapes(type(self).__name__, pred, target)
        if p.is_cuda:
            return _MaskedLossFn.apply(p, t.detach(), self._kind)
        return _masked_loss_host(p, t.detach(), self._kind)


class OGBNanLabelBCEWithLogitsLoss(_OGBNanLabelLoss):
    """reference commons/losses.py:13-21: BCEWithLogitsLoss (mean) over the elements whose target is not NaN - the multi-task
    MoleculeNet / OGB datasets.  No labelled element at all: NaN, the reference's mean over an empty selection, and a zero gradient."""
    _kind = ops.MASKED_LOSS_KINDS['bce_with_logits']


class OGBNanLabelMSELoss(_OGBNanLabelLoss):
    """reference commons/losses.py:23-31: MSELoss (mean) over the elements whose target is not NaN."""
    _kind = ops.MASKED_LOSS_KINDS['mse']


# ---- every node's 2D embedding against the 3D embeddings of whole molecules (csrc/localglobal.hip) ------------------------------------------
def _local_global_graph_ptr(name, zn, zg, nodes_per_graph):
    """int32 [B + 1] segment pointer of the node rows on zn's device, from a device tensor (batch_num_nodes()), a CPU tensor or a list;
    a device cumsum, no host synchronisation.  Everything that cannot be a batch of this loss is refused before any device work."""
    if nodes_per_graph is None:
        raise ValueError(f'{name}: nodes_per_graph is None - the loss needs the number of nodes of every graph '
                         '(graph.batch_num_nodes())')
    if not (torch.is_tensor(zn) and torch.is_tensor(zg)) or zn.dim() != 2 or zg.dim() != 2 or zn.shape[1] != zg.shape[1]:
        raise ValueError(f'{name}: zn [nodes, dim] and zg [graphs, dim] of one width expected, got '
                         f'{tuple(zn.shape) if torch.is_tensor(zn) else type(zn).__name__} and '
                         f'{tuple(zg.shape) if torch.is_tensor(zg) else type(zg).__name__}')
    N, B = zn.shape[0], zg.shape[0]
    on_host = not (torch.is_tensor(nodes_per_graph) and nodes_per_graph.is_cuda)
    if on_host:
        nodes_per_graph = torch.as_tensor(nodes_per_graph)
    if nodes_per_graph.dim() != 1 or nodes_per_graph.shape[0] != B:
        raise ValueError(f'{name}: nodes_per_graph has {tuple(nodes_per_graph.shape)} entries, zg has {B} graph rows')
    if B < 2:
        raise ValueError(f'{name}: a batch of {B} graph(s) has no negatives')
    if nodes_per_graph.dtype.is_floating_point or nodes_per_graph.dtype == torch.bool:
        raise ValueError(f'{name}: nodes_per_graph must hold integers, got {nodes_per_graph.dtype}')
    if on_host and (int(nodes_per_graph.sum()) != N or int(nodes_per_graph.min()) < 0):
        raise ValueError(f'{name}: nodes_per_graph sums to {int(nodes_per_graph.sum())} (smallest entry '
                         f'{int(nodes_per_graph.min())}), zn has {N} node rows')
    if N < 1 or zn.shape[1] < 1:
        raise ValueError(f'{name}: zn of shape {tuple(zn.shape)} holds nothing to contrast')
    if zn.dtype != torch.float32 or zg.dtype != torch.float32:
        raise NotImplementedError(f'{name}: fp32 only, got {zn.dtype} and {zg.dtype}')
    if not (zn.is_cuda and zg.is_cuda):
        raise RuntimeError(f'{name}: zn is on {zn.device}, zg on {zg.device} - the loss runs on the HIP kernels, there is no CPU '
                           'fallback')
    graph_ptr = torch.zeros(B + 1, dtype=torch.int32, device=zn.device)
    graph_ptr[1:] = torch.cumsum(nodes_per_graph.to(zn.device, non_blocking=True), dim=0)
    return graph_ptr


def _aligned16(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _LocalGlobalFn(torch.autograd.Function):
    """mean_i -log(e_{i,g(i)} / sum_{j != g(i)} e_ij) over the node rows; one C call per direction.  The [N, B] similarity is kept for
    the backward pass, the per-row log-sum of the negatives next to it."""

    @staticmethod
    def forward(ctx, zn, zg, graph_ptr, tau, eps, norm):
        zn, zg = _aligned16(zn), _aligned16(zg)
        N, D = zn.shape
        B = zg.shape[0]
        L = _lib.load()
        scratch = torch.empty(L.i3d_lg_ntxent_scratch_floats(N, B), dtype=torch.float32, device=zn.device)
        loss = torch.empty(1, dtype=torch.float32, device=zn.device)
        _lib.check(L.i3d_lg_ntxent_fwd(zn.data_ptr(), zg.data_ptr(), graph_ptr.data_ptr(), N, B, D, float(tau), float(eps), int(norm),
                                       scratch.data_ptr(), loss.data_ptr(), ops._stream()), 'i3d_lg_ntxent_fwd')
        ctx.cfg = (float(tau), float(eps), int(norm))
        ctx.save_for_backward(zn, zg, graph_ptr, scratch)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        tau, eps, norm = ctx.cfg
        zn, zg, graph_ptr, scratch = ctx.saved_tensors
        N, D = zn.shape
        B = zg.shape[0]
        L = _lib.load()
        work = torch.empty(L.i3d_lg_ntxent_work_floats(N, B, D), dtype=torch.float32, device=zn.device)
        dzn, dzg = torch.empty_like(zn), torch.empty_like(zg)
        gs = grad_out.contiguous().float()          # multiplied in on the device: no host read-back
        _lib.check(L.i3d_lg_ntxent_bwd(zn.data_ptr(), zg.data_ptr(), graph_ptr.data_ptr(), N, B, D, tau, eps, norm, scratch.data_ptr(),
                                       gs.data_ptr(), work.data_ptr(), dzn.data_ptr(), dzg.data_ptr(), ops._stream()),
                   'i3d_lg_ntxent_bwd')
        return dzn, dzg, None, None, None, None


class NTXentLocalGlobal(_Loss):
    """reference commons/losses.py:1117-1161: `forward(zn, zg, nodes_per_graph)` with zn [N, dim] the node embeddings of the batch
    (PNALocal), zg [B, dim] the embeddings of whole molecules (the 3D network) and nodes_per_graph the B node counts (a device tensor,
    a CPU tensor or a list).  The positive of node i is its own molecule, the negatives are the other B - 1; epsilon 1e-10 (:1153).
    Single process only: the data-parallel form would need the global node count."""
    _eps = 1e-10       # reference :1153

    def __init__(self, norm: bool = True, tau: float = 0.5) -> None:
        super().__init__()
        self.norm, self.tau = norm, tau
        self.group = None

    def attach_group(self, group):
        self.group = group
        return self

    def forward(self, zn, zg, nodes_per_graph=None, **kwargs) -> Tensor:
        name = type(self).__name__
        if self.group is not None:
            import torch.distributed as dist
            if dist.get_world_size(self.group) > 1:
                raise NotImplementedError(f'{name} on a process group of more than one rank: the loss is a mean over the nodes of the '
                                          'global batch, which needs the global node count')
        graph_ptr = _local_global_graph_ptr(name, zn, zg, nodes_per_graph)
        return _LocalGlobalFn.apply(zn, zg, graph_ptr, float(self.tau), self._eps, bool(self.norm))


class NTXentGlobalLocal(_Loss):
    """reference commons/losses.py:1164-1185: NTXentLocalGlobal with the first two arguments swapped, `forward(zg, zn,
    nodes_per_graph)` - what SelfSupervisedAlternatingTrainer calls."""

    def __init__(self, **kwargs) -> None:
        super().__init__()
        self.ntxent_local_global = NTXentLocalGlobal(**kwargs)

    def attach_group(self, group):
        self.ntxent_local_global.attach_group(group)
        return self

    def forward(self, zg, zn, nodes_per_graph=None, **kwargs) -> Tensor:
        return self.ntxent_local_global(zn, zg, nodes_per_graph)


# ---- single-positive losses that re-weight the negatives (csrc/hardneg.hip) -----------------------------------------------------------------
def _single_positive_shapes(name, z1, z2):
    """everything that cannot be a batch of these losses is refused before any device work"""
    if not (torch.is_tensor(z1) and torch.is_tensor(z2)) or z1.dim() != 2 or z2.dim() != 2 or z1.shape[1] != z2.shape[1]:
        raise ValueError(f'{name}: z1 [batch, dim] and z2 [rows, dim] of one width expected, got '
                         f'{tuple(z1.shape) if torch.is_tensor(z1) else type(z1).__name__} and '
                         f'{tuple(z2.shape) if torch.is_tensor(z2) else type(z2).__name__}')
    if z1.shape[0] < 1 or z1.shape[1] < 1:
        raise ValueError(f'{name}: z1 of shape {tuple(z1.shape)} holds nothing to contrast')


def _device_fp32(name, z1, z2):
    if z1.dtype != torch.float32 or z2.dtype != torch.float32:
        raise NotImplementedError(f'{name}: fp32 only, got {z1.dtype} and {z2.dtype}')
    if not (z1.is_cuda and z2.is_cuda):
        raise RuntimeError(f'{name}: z1 is on {z1.device}, z2 on {z2.device} - the loss runs on the HIP kernels, there is no CPU fallback')


class _HardNegFn(torch.autograd.Function):
    """loss_share = sum_i l_i / global_batch over the local rows of z1, l_i by `mode` (ops.HARDNEG_MODES); one C call per direction.
    `extra` [b1 U, dim]: the private extra negatives of NTXentExtraNegatives, else None."""

    @staticmethod
    def forward(ctx, z1, z2, extra, mode, norm, tau, tau_plus, beta, extra_weight, pos_offset, global_batch):
        z1, z2 = _aligned16(z1), _aligned16(z2)
        b1, dim = z1.shape
        b2 = z2.shape[0]
        n_extra = 0
        if extra is not None and extra.shape[0] > 0:
            extra = _aligned16(extra)
            n_extra = extra.shape[0] // b1
        else:
            extra = None
        L = _lib.load()
        scratch = torch.empty(L.i3d_hardneg_loss_scratch_floats(b1, b2, n_extra), dtype=torch.float32, device=z1.device)
        loss = torch.empty(1, dtype=torch.float32, device=z1.device)
        _lib.check(L.i3d_hardneg_loss_fwd(mode, z1.data_ptr(), z2.data_ptr(), ops._p(extra), b1, b2, n_extra, dim, pos_offset, int(norm),
                                          tau, tau_plus, beta, extra_weight, 1.0 / global_batch, scratch.data_ptr(), loss.data_ptr(),
                                          ops._stream()), 'i3d_hardneg_loss_fwd')
        ctx.cfg = (mode, int(norm), tau, beta, pos_offset, global_batch, n_extra)
        ctx.has_extra = extra is not None
        ctx.save_for_backward(*((z1, z2, scratch) + ((extra,) if extra is not None else ())))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        mode, norm, tau, beta, pos_offset, global_batch, n_extra = ctx.cfg
        z1, z2, scratch = ctx.saved_tensors[:3]
        extra = ctx.saved_tensors[3] if ctx.has_extra else None
        b1, dim = z1.shape
        b2 = z2.shape[0]
        L = _lib.load()
        work = torch.empty(b1 * b2, dtype=torch.float32, device=z1.device)
        dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
        dx = torch.empty_like(extra) if extra is not None else None
        gs = grad_out.contiguous().float()          # multiplied in on the device: no host read-back
        _lib.check(L.i3d_hardneg_loss_bwd(mode, z1.data_ptr(), z2.data_ptr(), ops._p(extra), b1, b2, n_extra, dim, pos_offset, norm, tau,
                                          beta, 1.0 / global_batch, scratch.data_ptr(), gs.data_ptr(), work.data_ptr(), dz1.data_ptr(),
                                          dz2.data_ptr(), ops._p(dx), ops._stream()), 'i3d_hardneg_loss_bwd')
        return (dz1, dz2, dx) + (None,) * 8


class _SinglePositiveBase(_NTXentBase):
    """no epsilon in any of them; the data-parallel form is NTXent's: z2 gathered, this rank's share of the global mean returned"""
    _eps = 0.0
    _mode = None

    def _loss(self, z1, z2, extra=None, tau_plus=0.0, beta=0.0, extra_weight=1.0):
        name = type(self).__name__
        hard = self._mode in ('ntxent_hard', 'infonce_hard')
        if hard and self._local_world() == 1 and z1.shape[0] == 1:
            raise ValueError(f'{name}: a global batch of 1 has no negatives to re-weight (the reference takes the mean of an empty tensor)')
        _device_fp32(name, z1, z2)
        z2, pos_offset, global_batch = self._gathered(z1, z2, 1)
        if hard and global_batch == 1:
            raise ValueError(f'{name}: a global batch of 1 has no negatives to re-weight')
        return _HardNegFn.apply(z1, z2, extra, ops.HARDNEG_MODES[self._mode], bool(self.norm), float(self.tau), float(tau_plus),
                                float(beta), float(extra_weight), pos_offset, global_batch)

    def _local_world(self):
        if self.group is None:
            return 1
        import torch.distributed as dist
        return dist.get_world_size(self.group)


class InfoNCE(_SinglePositiveBase):
    """reference commons/losses.py:998-1034: NTXent with the positive kept in the denominator, l_i = -log(pos_i / sum_j P_ij)."""
    _mode = 'infonce'

    def forward(self, z1, z2, **kwargs) -> Tensor:
        _single_positive_shapes(type(self).__name__, z1, z2)
        return self._regularisers(self._loss(z1, z2), z1, z2)


class _HardBase(_SinglePositiveBase):
    def __init__(self, norm, tau, tau_plus, beta) -> None:
        super().__init__(norm, tau)
        self.tau_plus, self.beta = tau_plus, beta

    def forward(self, z1, z2, **kwargs) -> Tensor:
        _single_positive_shapes(type(self).__name__, z1, z2)
        return self._loss(z1, z2, tau_plus=self.tau_plus, beta=self.beta)


class InfoNCEHard(_HardBase):
    """reference commons/losses.py:1037-1074: NTXentHard with l_i = -log(pos_i / (pos_i + Ng_i)); no normalisation by default."""
    _mode = 'infonce_hard'

    def __init__(self, norm: bool = False, tau: float = 0.5, tau_plus=0.1, beta=0.5) -> None:
        super().__init__(norm, tau, tau_plus, beta)


class NTXentHard(_HardBase):
    """reference commons/losses.py:1077-1114: the negatives re-weighted by P^beta (Robinson et al., Contrastive Learning with Hard
    Negative Samples), Ng_i = (n sum_j P_ij^(1 + beta) / sum_j P_ij^beta - tau_plus n pos_i) / (1 - tau_plus) clamped from below at
    n e^(-1 / tau), l_i = -log(pos_i / Ng_i).  The weights are not detached: the gradient runs through them, as in the reference."""
    _mode = 'ntxent_hard'

    def __init__(self, norm: bool = True, tau: float = 0.5, tau_plus=0.1, beta=0.1) -> None:
        super().__init__(norm, tau, tau_plus, beta)


class _SplitRowsFn(torch.autograd.Function):
    """x -> (x[:rows], x[rows:]); the backward is one concatenation where torch's two slices launch two zero fills, two copies and an
    add"""

    @staticmethod
    def forward(ctx, x, rows):
        ctx.rows = rows
        return x[:rows], x[rows:]

    @staticmethod
    def backward(ctx, g_head, g_tail):
        return torch.cat([g_head, g_tail]), None


class NTXentExtraNegatives(_SinglePositiveBase):
    """reference commons/losses.py:889-943: z2 is [B (1 + U), dim]; its first B rows are the other view, row B + i U + u is the u-th extra
    negative of row i alone, weighted by extra_negatives_weight in the denominator.  Data parallel: z2[:B] is gathered, the extras stay
    local.  The regularisers see z2[:B]."""
    _mode = 'extra_negatives'

    def __init__(self, norm: bool = True, tau: float = 0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0,
                 extra_negatives_weight=1) -> None:
        super().__init__(norm, tau, uniformity_reg, variance_reg, covariance_reg)
        self.extra_negatives_weight = extra_negatives_weight

    def forward(self, z1, z2, **kwargs) -> Tensor:
        name = type(self).__name__
        _single_positive_shapes(name, z1, z2)
        B = z1.shape[0]
        if z2.shape[0] < B or z2.shape[0] % B != 0:
            raise ValueError(f'{name}: the {z2.shape[0]} rows of z2 are not a multiple of the batch size {B} (z2 is [batch * (1 + extra '
                             'negatives), dim])')
        U = z2.shape[0] // B - 1
        if U > ops.HARDNEG_MAX_EXTRA:
            raise NotImplementedError(f'{name}: {U} extra negatives per row, the kernels are built for 0..{ops.HARDNEG_MAX_EXTRA}')
        other, extra = _SplitRowsFn.apply(z2, B) if U > 0 else (z2, None)
        loss = self._loss(z1, other, extra, extra_weight=self.extra_negatives_weight)
        return self._regularisers(loss, z1, other)


class _PermuteRowsFn(torch.autograd.Function):
    """x[perm] on the device; the backward gathers with the inverse permutation"""

    @staticmethod
    def forward(ctx, x, perm, inv_perm):
        ctx.inv_perm = inv_perm
        return ops.gather_rows(x.contiguous(), perm)

    @staticmethod
    def backward(ctx, g):
        return ops.gather_rows(g.contiguous(), ctx.inv_perm), None, None


class NTXentShuffled(_SinglePositiveBase):
    """reference commons/losses.py:967-995, the control experiment: NT-Xent (no epsilon) against a random permutation of z2, drawn with
    torch.randperm from the host's default generator as the reference draws it - the same seed gives the same permutation."""

    def __init__(self, norm: bool = True, tau: float = 0.5) -> None:
        super().__init__(norm, tau)

    def forward(self, z1, z2, **kwargs) -> Tensor:
        name = type(self).__name__
        if self._local_world() > 1:
            raise NotImplementedError(f'{name} on a process group of more than one rank: the permutation would have to be one of the '
                                      'global batch')
        _single_positive_shapes(name, z1, z2)
        _device_fp32(name, z1, z2)
        perm = torch.randperm(len(z2))
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(len(z2))
        idx = torch.stack([perm, inv]).to(torch.int32).pin_memory().to(z2.device, non_blocking=True)
        return self._contrastive(z1, _PermuteRowsFn.apply(z2, idx[0], idx[1]), 1)


# ---- the non-contrastive objectives (csrc/batchstat.hip) ------------------------------------------------------------------------------------
def _shape_of(t):
    return tuple(t.shape) if torch.is_tensor(t) else type(t).__name__


def _two_views(name, z1, z2, needs_two_rows):
    """shapes that cannot be a batch of these losses are refused before any device work"""
    if not (torch.is_tensor(z1) and torch.is_tensor(z2)) or z1.dim() != 2 or z1.shape != z2.shape:
        raise ValueError(f'{name}: z1 and z2 [batch, dim] of one shape expected, got {_shape_of(z1)} and {_shape_of(z2)}')
    if z1.shape[0] < 1 or z1.shape[1] < 1:
        raise ValueError(f'{name}: z1 of shape {tuple(z1.shape)} holds nothing to compare')
    if needs_two_rows and z1.shape[0] < 2:
        raise ValueError(f'{name}: a batch of {z1.shape[0]} has no unbiased variance (the statistics over the batch divide by batch - 1)')


def _fp32_on_device(name, *tensors):
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_cuda:
            raise NotImplementedError(f'{name}: fp32 tensors on the device only, got {t.dtype} on {t.device} (the loss runs on the HIP '
                                      'kernels, there is no CPU fallback)')


class _ColStatFn(torch.autograd.Function):
    """The terms built on statistics over the batch axis, as one scalar: with barlow = (scale_loss, lambd) the BarlowTwins objective
    scale_loss (sum_i (C_ii - 1)^2 + lambd sum_{i != j} C_ij^2), C = a1^T a2 / B of the standardised views; var_w (std_loss(z1) +
    std_loss(z2)); cov_w (cov_loss(z1) + cov_loss(z2)).  One moments launch serves every term; the D x D products are the library's GEMM,
    and the pass over them leaves their gradient in place, so the backward is GEMMs and one launch."""

    @staticmethod
    def forward(ctx, z1, z2, barlow, var_w, cov_w):
        z1, z2 = z1.contiguous(), z2.contiguous()
        n, dim = z1.shape
        mom, a, c = ops.bs_moments(z1, z2, standardised=barlow is not None, centred=cov_w != 0)
        count = (1 if barlow is not None else 0) + (2 if cov_w != 0 else 0)
        partial = torch.empty(count, ops.bs_pass_blocks(dim), dtype=torch.float64, device=z1.device) if count else None
        saved = [z1, z2, mom]
        first = 0
        if barlow is not None:
            scale_loss, lambd = barlow
            G = ops.gemm(a[0], a[1], trans_a=True)
            ops.bs_matrix_pass(G, 1.0 / n, 1.0, scale_loss, scale_loss * lambd, partial[:1])
            saved += [a[0], a[1], G]
            first = 1
        if cov_w != 0:
            Gc = torch.empty(2, dim, dim, dtype=torch.float32, device=z1.device)
            for v in range(2):
                ops.gemm(c[v], c[v], trans_a=True, out=Gc[v])
            ops.bs_matrix_pass(Gc, 1.0 / (n - 1), 0.0, 0.0, cov_w / dim, partial[first:])
            saved += [c[0], c[1], Gc]
        ctx.cfg = (barlow is not None, var_w, cov_w)
        ctx.save_for_backward(*saved)
        return ops.bs_finish(partial, 1.0, mom, var_w).reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        has_barlow, var_w, cov_w = ctx.cfg
        saved = list(ctx.saved_tensors)
        z1, z2, mom = saved[:3]
        del saved[:3]
        n = z1.shape[0]
        a = da = dc = None
        if has_barlow:
            a1, a2, G = saved[:3]
            del saved[:3]
            a, da = [a1, a2], [ops.gemm(a2, G, trans_b=True), ops.gemm(a1, G)]          # b G^T, a G
        if cov_w != 0:
            c1, c2, Gc = saved[:3]
            dc = [ops.gemm(c1, Gc[0]), ops.gemm(c2, Gc[1])]                             # G is symmetric: one product per view
        gs = grad_out.contiguous().float()                                              # multiplied in on the device: no host read-back
        dz1, dz2 = ops.bs_col_bwd([z1, z2], mom, a, da, dc, sa=1.0 / n, sc=2.0 / (n - 1), var_w=var_w, grad_scale_dev=gs)
        return dz1, dz2, None, None, None


class _RowCosFn(torch.autograd.Function):
    """mean over rows and repeats of |x / max(|x|, 1e-12) - y_r / max(|y_r|, 1e-12)|^2 for x [B, D] and y [B, D] or [B, D, R] normalised
    over dim 1; the repeat of x and a transposed y are never built"""

    @staticmethod
    def forward(ctx, x, y):
        x, y = x.contiguous(), y.contiguous()
        rowloss, stats = ops.bs_rows_fwd(x, y)
        ctx.count = x.shape[0] * (y.shape[2] if y.dim() == 3 else 1)
        ctx.save_for_backward(x, y, stats)
        return ops.bs_finish(rowloss, 1.0 / ctx.count).reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        x, y, stats = ctx.saved_tensors
        return ops.bs_rows_bwd(x, y, stats, 2.0 / ctx.count, grad_out.contiguous().float())


class _BatchStatBase(_Loss):
    """The regularisers of the two-view classes below: variance and covariance terms on the column kernels (their moments computed once
    per view), the uniformity term the module-level `uniformity_loss`.  No attach_group: under data parallelism the moments and the D x D
    matrices would have to be all-reduced."""

    def _weights(self):
        return (float(self.variance_reg) if self.variance_reg > 0 else 0.0, float(self.covariance_reg) if self.covariance_reg > 0 else 0.0)

    def _checked(self, z1, z2, always_two_rows=False):
        name = type(self).__name__
        var_w, cov_w = self._weights()
        _two_views(name, z1, z2, always_two_rows or var_w != 0 or cov_w != 0)
        _fp32_on_device(name, z1, z2)
        return var_w, cov_w

    def _uniformity(self, loss, z1, z2):
        if self.uniformity_reg > 0:
            loss = loss + self.uniformity_reg * uniformity_loss(z1, z2)
        return loss


class BarlowTwinsLoss(_BatchStatBase):
    """reference commons/losses.py:45-73 (Zbontar et al., Barlow Twins): both views standardised per column with the unbiased standard
    deviation, C = z1_norm^T z2_norm / B, loss = scale_loss (sum_i (C_ii - 1)^2 + lambd sum_{i != j} C_ij^2).  No epsilon, as in the
    reference: a column that is constant over the batch has a standard deviation of 0 and makes the loss non-finite.  A batch of 1 is
    refused."""

    def __init__(self, scale_loss=1 / 32, lambd=3.9e-3, uniformity_reg=0, variance_reg=0, covariance_reg=0) -> None:
        super().__init__()
        self.scale_loss, self.lambd = scale_loss, lambd
        self.uniformity_reg, self.variance_reg, self.covariance_reg = uniformity_reg, variance_reg, covariance_reg

    def forward(self, z1, z2, **kwargs) -> Tensor:
        var_w, cov_w = self._checked(z1, z2, always_two_rows=True)
        loss = _ColStatFn.apply(z1, z2, (float(self.scale_loss), float(self.lambd)), var_w, cov_w)
        return self._uniformity(loss, z1, z2)


class CosineSimilarityLoss(_BatchStatBase):
    """reference commons/losses.py:76-95 (BYOL, equation 2): mean_i |z1_i / |z1_i| - z2_i / |z2_i||^2 = 2 - 2 mean cos, norms clamped at
    1e-12 as F.normalize clamps them."""

    def __init__(self, uniformity_reg=0, variance_reg=0, covariance_reg=0) -> None:
        super().__init__()
        self.uniformity_reg, self.variance_reg, self.covariance_reg = uniformity_reg, variance_reg, covariance_reg

    def forward(self, z1, z2, **kwargs) -> Tensor:
        var_w, cov_w = self._checked(z1, z2)
        loss = _RowCosFn.apply(z1, z2)
        if var_w != 0 or cov_w != 0:
            loss = loss + _ColStatFn.apply(z1, z2, None, var_w, cov_w)
        return self._uniformity(loss, z1, z2)


class RegularizationLoss(_BatchStatBase):
    """reference commons/losses.py:98-123: the mean squared error of the two views plus the variance and covariance terms, which are on
    by default.  `norm` is accepted and ignored, as in the reference."""

    def __init__(self, norm: bool = True, uniformity_reg=0, variance_reg=1, covariance_reg=0.04) -> None:
        super().__init__()
        self.norm = norm
        self.uniformity_reg, self.variance_reg, self.covariance_reg = uniformity_reg, variance_reg, covariance_reg

    def forward(self, z1, z2, **kwargs) -> Tensor:
        var_w, cov_w = self._checked(z1, z2)
        loss = _MSEFn.apply(z1, z2, 1.0)
        if var_w != 0 or cov_w != 0:
            loss = loss + _ColStatFn.apply(z1, z2, None, var_w, cov_w)
        return self._uniformity(loss, z1, z2)


class CriticLoss(_Loss):
    """reference commons/losses.py:33-42: forward(z2, reconstruction) with reconstruction [B, D, R], each of its R vectors (dim 1)
    normalised and compared with the normalised z2 row: mean over B R of the squared distance.  R = 1 .. 32."""

    def __init__(self) -> None:
        super().__init__()

    def forward(self, z2, reconstruction, **kwargs) -> Tensor:
        name = type(self).__name__
        if (not (torch.is_tensor(z2) and torch.is_tensor(reconstruction)) or z2.dim() != 2 or reconstruction.dim() != 3
                or tuple(reconstruction.shape[:2]) != tuple(z2.shape) or min(reconstruction.shape) < 1):
            raise ValueError(f'{name}: z2 [batch, dim] and reconstruction [batch, dim, repeats] expected, got {_shape_of(z2)} and '
                             f'{_shape_of(reconstruction)}')
        if reconstruction.shape[2] > ops.BATCHSTAT_MAX_REPEATS:
            raise NotImplementedError(f'{name}: {reconstruction.shape[2]} repeats, the kernels are built for 1..'
                                      f'{ops.BATCHSTAT_MAX_REPEATS}')
        _fp32_on_device(name, z2, reconstruction)
        return _RowCosFn.apply(z2, reconstruction)
