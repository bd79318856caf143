// Fine-tuning losses and metrics over a [B, T] table of predictions and targets (B molecules, T tasks, row major).
//
// Masked multi-task losses (reference commons/losses.py:13-31, OGBNanLabelBCEWithLogitsLoss / OGBNanLabelMSELoss): an element is
// labelled iff its target is not NaN; the loss is the mean over the labelled elements.  The reference gathers pred[is_labeled] and
// target[is_labeled] (two boolean-mask gathers, each a host synchronisation); here the mask is a branch.  The mean runs over ALL
// labelled elements, whatever their column, so the forward is a flat reduction over the B T values - every lane busy at T = 1:
//
//   forward    workgroup g sums its chunk of the flat array (fp64 terms, fp64 sums, count in fp64) -> partial[g] = {sum, count};
//              one workgroup then sums the partials in a fixed order and writes out = {mean, count, fp32(mean)}.  One workgroup in
//              all: it writes `out` itself (one launch).  The prediction at an unlabelled position is never read into the sum.
//   backward   elementwise, grad_out[0] and the count read on the device: labelled -> grad_out f'(x, t) / count, else 0.0f.
//
// Task moments (reference trainer/metrics.py:15-158: PearsonR, Rsquared, MAE, MeanPredictorLoss, QM9DenormalizedL1 / L2,
// QM9SingleTargetDenormalizedL1): every one of them is a function of the per-task table written here, table[T + 1][10] in fp64 (row T
// = the totals).  Two passes, the centred sums formed around the column means of pass 1 (the two-pass variance of klmp.hip):
//
//   thread map T <= 256: 256 / T whole rows side by side in the workgroup, thread = (row, column) = (tid / T, tid % T) - one
//              iteration reads 256 / T consecutive rows, contiguous in memory.  T = 1: 256 rows per iteration, every lane a row;
//              T <= 128: two or more rows per iteration ('packed rows'); 129..256: one row per iteration, the lanes are the
//              columns.  T > 256: column tiles of 256 (blockIdx.y), one row per iteration.
//   pass k     workgroup (g, tile) handles rows [g chunk, (g + 1) chunk): per thread fp64 sums down its column, then the threads
//              of row 0 add the workgroup's rows in order (LDS) -> partial[g][column][.]
//   final k    one workgroup: per column the partials in block order -> table; the totals by block_sum_f64 over the columns
//
// Four launches.  Sums have a fixed order, no atomics, no hand-off between workgroups inside a launch, no buffer beyond the caller's.
#include "common.h"

#include <math.h>

namespace i3d {

constexpr int TL_MAX_BLOCKS = 1024;
constexpr long TL_MIN_CHUNK = 512;
constexpr int TM_K = 10;                 // columns of the moments table
constexpr int TM_MAX_ROW_BLOCKS = 64;

static long tl_chunk(long n) {
    const long c = (n + TL_MAX_BLOCKS - 1) / TL_MAX_BLOCKS;
    return c < TL_MIN_CHUNK ? TL_MIN_CHUNK : c;
}

// kind 0: torch's binary_cross_entropy_with_logits, max(x, 0) - x t + log1p(exp(-|x|)); kind 1: (x - t)^2
__device__ __forceinline__ double tl_term(double x, double t, int kind) {
    if (kind == 0) return fmax(x, 0.) - x * t + log1p(exp(-fabs(x)));
    const double d = x - t;
    return d * d;
}

// out = {mean over the labelled elements (0 / 0 = NaN when there is none), their count, the mean rounded to fp32 in the first four bytes}
__device__ __forceinline__ void tl_write(double s, double c, double* __restrict__ out) {
    const double m = s / c;
    out[0] = m;
    out[1] = c;
    float* f = reinterpret_cast<float*>(out + 2);
    f[0] = (float)m;
    f[1] = 0.f;
}

__global__ void __launch_bounds__(256)
masked_loss_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, long n, long chunk, int kind,
                           double* __restrict__ partial, double* __restrict__ out) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const long i0 = (long)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
    double s = 0., c = 0.;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
        const float t = target[i];
        if (t == t) {          // labelled; the prediction of an unlabelled element (NaN, inf, anything) stays out of the sum
            s += tl_term((double)pred[i], (double)t, kind);
            c += 1.;
        }
    }
    s = block_sum_f64(s, sm);
    c = block_sum_f64(c, sm);
    if (threadIdx.x == 0) {
        if (out) {             // the only workgroup
            tl_write(s, c, out);
        } else {
            partial[2 * blockIdx.x] = s;
            partial[2 * blockIdx.x + 1] = c;
        }
    }
}

__global__ void __launch_bounds__(256)
masked_loss_final_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double s = 0., c = 0.;
    for (int b = threadIdx.x; b < blocks; b += 256) {
        s += partial[2 * b];
        c += partial[2 * b + 1];
    }
    s = block_sum_f64(s, sm);
    c = block_sum_f64(c, sm);
    if (threadIdx.x == 0) tl_write(s, c, out);
}

__global__ void __launch_bounds__(256)
masked_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, long n, int kind, const double* __restrict__ out,
                       const float* __restrict__ grad_out, float* __restrict__ grad_pred) {
    I3D_CHAIN_PRIO();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float t = target[i];
    float g = 0.f;
    if (t == t) {
        const double scale = (grad_out ? (double)grad_out[0] : 1.) / out[1], x = (double)pred[i];
        const double f = kind == 0 ? 1. / (1. + exp(-x)) - (double)t : 2. * (x - (double)t);
        g = (float)(scale * f);
    }
    grad_pred[i] = g;
}

// ---- task moments ------------------------------------------------------------------------------------------------------------------
struct TmPlan {
    int rows_per_iter, col_tiles, row_blocks;
    long chunk_rows;
};

static TmPlan tm_plan(int rows, int tasks) {
    TmPlan p;
    p.rows_per_iter = tasks <= 256 ? 256 / tasks : 1;
    p.col_tiles = tasks <= 256 ? 1 : cdiv(tasks, 256);
    long iters = ((long)rows + (long)p.rows_per_iter * TM_MAX_ROW_BLOCKS - 1) / ((long)p.rows_per_iter * TM_MAX_ROW_BLOCKS);
    if (iters < 2) iters = 2;
    p.chunk_rows = iters * p.rows_per_iter;
    p.row_blocks = (int)(((long)rows + p.chunk_rows - 1) / p.chunk_rows);
    return p;
}

// -> whether this thread has a (row, column) of the workgroup's tile; rsub = its row inside one iteration, col = its column
__device__ __forceinline__ bool tm_map(int tasks, int R, int& col, int& rsub) {
    if (tasks <= 256) {
        rsub = (int)threadIdx.x / tasks;
        col = (int)threadIdx.x - rsub * tasks;
        return rsub < R;
    }
    rsub = 0;
    col = (int)blockIdx.y * 256 + (int)threadIdx.x;
    return col < tasks;
}

// PASS 1: {sum p, sum t}; PASS 2: {sum (p - pbar_c)^2, sum (t - tbar_c)^2, sum (p - pbar_c)(t - tbar_c), sum |p - t|, sum (p - t)^2,
// sum |t - tbar|, sum (t - tbar)^2}, pbar_c / tbar_c the column means and tbar the mean of all targets, from the table pass 1 left
template <int PASS>
__global__ void __launch_bounds__(256)
tm_pass_kernel(const float* __restrict__ pred, const float* __restrict__ target, int rows, int tasks, int R, long chunk_rows,
               const double* __restrict__ table, double* __restrict__ partial) {
    I3D_CHAIN_PRIO();
    constexpr int Q = PASS == 1 ? 2 : 7;
    __shared__ double sm[Q][256];
    int col, rsub;
    const bool active = tm_map(tasks, R, col, rsub);
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0., a4 = 0., a5 = 0., a6 = 0.;
    if (active) {
        const long r0 = (long)blockIdx.x * chunk_rows, r1 = min((long)rows, r0 + chunk_rows);
        double pbar = 0., tbar = 0., gbar = 0.;
        if (PASS == 2) {
            const double* tc = table + (long)col * TM_K;
            const double* tt = table + (long)tasks * TM_K;
            pbar = tc[1] / tc[0];
            tbar = tc[2] / tc[0];
            gbar = tt[2] / tt[0];
        }
        for (long r = r0 + rsub; r < r1; r += R) {
            const double p = (double)pred[r * tasks + col], t = (double)target[r * tasks + col];
            if (PASS == 1) {
                a0 += p;
                a1 += t;
            } else {
                const double dp = p - pbar, dt = t - tbar, d = p - t, g = t - gbar;
                a0 += dp * dp;
                a1 += dt * dt;
                a2 += dp * dt;
                a3 += fabs(d);
                a4 += d * d;
                a5 += fabs(g);
                a6 += g * g;
            }
        }
    }
    sm[0][threadIdx.x] = a0;
    sm[1][threadIdx.x] = a1;
    if (PASS == 2) {
        sm[2 % Q][threadIdx.x] = a2;
        sm[3 % Q][threadIdx.x] = a3;
        sm[4 % Q][threadIdx.x] = a4;
        sm[5 % Q][threadIdx.x] = a5;
        sm[6 % Q][threadIdx.x] = a6;
    }
    __syncthreads();
    if (active && rsub == 0) {
        double* dst = partial + ((long)blockIdx.x * tasks + col) * Q;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            double s = 0.;
            for (int k = 0; k < R; ++k) s += sm[q][threadIdx.x + k * tasks];      // (k, col) is thread k T + col; T > 256: R = 1
            dst[q] = s;
        }
    }
}

// one workgroup: per column the partials of the row blocks in block order, the totals over the columns in a fixed order
template <int PASS>
__global__ void __launch_bounds__(256)
tm_final_kernel(const double* __restrict__ partial, int rows, int tasks, int row_blocks, double* __restrict__ table) {
    I3D_CHAIN_PRIO();
    constexpr int Q = PASS == 1 ? 2 : 7;
    constexpr int OFF = PASS == 1 ? 1 : 3;
    __shared__ double sm[4];
    double* tt = table + (long)tasks * TM_K;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        double tot = 0.;
        for (int c = threadIdx.x; c < tasks; c += 256) {
            double s = 0.;
            for (int b = 0; b < row_blocks; ++b) s += partial[((long)b * tasks + c) * Q + q];
            table[(long)c * TM_K + OFF + q] = s;
            tot += s;
        }
        tot = block_sum_f64(tot, sm);
        if (threadIdx.x == 0) tt[OFF + q] = tot;
    }
    if (PASS == 1) {
        for (int c = threadIdx.x; c < tasks; c += 256) table[(long)c * TM_K] = (double)rows;
        if (threadIdx.x == 0) tt[0] = (double)rows * (double)tasks;
    }
}

}  // namespace i3d

using namespace i3d;

static int task_check(int rows, int tasks) {
    I3D_CHECK_ARG(rows >= 1, "rows below 1");
    I3D_CHECK_ARG(tasks >= 1, "tasks below 1");
    return I3D_OK;
}

extern "C" long i3d_masked_loss_partial_floats(int rows, int tasks) {
    if (rows < 1 || tasks < 1) return 0;
    const long n = (long)rows * tasks;
    return 4L * ((n + tl_chunk(n) - 1) / tl_chunk(n));          // {sum, count} in fp64 per workgroup
}

extern "C" int i3d_masked_loss_fwd(const float* pred, const float* target, int rows, int tasks, int kind, float* partials, double* out,
                                   void* stream) {
    if (int rc = task_check(rows, tasks)) return rc;
    I3D_CHECK_ARG(kind == 0 || kind == 1, "kind is 0 (BCE with logits) or 1 (squared error)");
    I3D_CHECK_ARG(pred && target && partials && out, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long n = (long)rows * tasks, chunk = tl_chunk(n);
    const int blocks = (int)((n + chunk - 1) / chunk);
    double* part = reinterpret_cast<double*>(partials);
    hipLaunchKernelGGL(masked_loss_partial_kernel, dim3(blocks), dim3(256), 0, s, pred, target, n, chunk, kind, part,
                       blocks == 1 ? out : (double*)nullptr);
    I3D_CHECK_LAUNCH();
    if (blocks > 1) {
        hipLaunchKernelGGL(masked_loss_final_kernel, dim3(1), dim3(256), 0, s, part, blocks, out);
        I3D_CHECK_LAUNCH();
    }
    return I3D_OK;
}

extern "C" int i3d_masked_loss_bwd(const float* pred, const float* target, int rows, int tasks, int kind, const double* out,
                                   const float* grad_out, float* grad_pred, void* stream) {
    if (int rc = task_check(rows, tasks)) return rc;
    I3D_CHECK_ARG(kind == 0 || kind == 1, "kind is 0 (BCE with logits) or 1 (squared error)");
    I3D_CHECK_ARG(pred && target && out && grad_pred, "null pointer");
    const long n = (long)rows * tasks;
    hipLaunchKernelGGL(masked_loss_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred, target, n, kind,
                       out, grad_out, grad_pred);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" long i3d_task_moments_partial_floats(int rows, int tasks) {
    if (rows < 1 || tasks < 1) return 0;
    return 2L * 7 * tm_plan(rows, tasks).row_blocks * tasks;      // pass 2's seven fp64 sums per (row block, column); pass 1 uses two
}

extern "C" int i3d_task_moments(const float* pred, const float* target, int rows, int tasks, float* partials, double* table,
                                void* stream) {
    if (int rc = task_check(rows, tasks)) return rc;
    I3D_CHECK_ARG(pred && target && partials && table, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const TmPlan p = tm_plan(rows, tasks);
    double* part = reinterpret_cast<double*>(partials);
    const dim3 grid(p.row_blocks, p.col_tiles);
    hipLaunchKernelGGL(tm_pass_kernel<1>, grid, dim3(256), 0, s, pred, target, rows, tasks, p.rows_per_iter, p.chunk_rows,
                       (const double*)table, part);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(tm_final_kernel<1>, dim3(1), dim3(256), 0, s, (const double*)part, rows, tasks, p.row_blocks, table);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(tm_pass_kernel<2>, grid, dim3(256), 0, s, pred, target, rows, tasks, p.rows_per_iter, p.chunk_rows,
                       (const double*)table, part);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(tm_final_kernel<2>, dim3(1), dim3(256), 0, s, (const double*)part, rows, tasks, p.row_blocks, table);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
