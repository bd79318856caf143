// Local-global NT-Xent: every node embedding against the graph embeddings, forward and backward.
//
// Replaces NTXentLocalGlobal.forward (reference commons/losses.py:1131-1161):
//     S = zn zg^T;  S' = S / (|zn_i||zg_j| + eps);  e = exp(S'/tau);  pos_i = e_{i,g(i)};  neg_i = sum_{j != g(i)} e_ij
//     loss = - mean_i log(pos_i / neg_i)
// g(i) is the graph that holds node row i.  The reference fills an [N, B] mask from a Python loop over the graphs; the positives
// are contiguous row segments, so here g(i) is a binary search in graph_ptr and no mask exists.  The similarity and the two
// gradient products run on the MFMA GEMM; these kernels fuse normalisation, exp, the row reductions and the log, and produce dL/dS
// plus the rank-1 norm-path terms.
//
// neg_i is summed over the columns other than g(i) - never as rowsum - pos: at tau = 0.1 an aligned positive is e^10 next to
// negatives of e^-10, and the subtraction returns 0 in fp32.  The maximum of the negatives is taken out of the sum, so
//     l_i = log neg_i - S'_{i,g(i)}/tau = m_i + log sum_{j != g(i)} exp(S'_ij/tau - m_i) - S'_{i,g(i)}/tau
// with a sum >= 1: finite wherever fp32 holds the result.  The backward pass needs one float per row, lse_i = log neg_i.
//
// The matrix is tall (N = 9 k .. 25 k rows, B = 32 .. 512 columns): one WAVE owns a row (four rows per workgroup, no LDS, no
// barrier), and the column sums of the norm path (cb) are reduced in two stages over row chunks of LG_ROW_CHUNK rows, so the order of
// every sum depends on (N, B) only.  No atomics.
#include "common.h"

namespace i3d {

constexpr int LG_ROW_CHUNK = 256;      // rows per first-stage workgroup of the column reduction (i3d_lg_row_chunk)
constexpr int LG_COLS = 64;            // columns per first-stage workgroup: 64 columns x 4 row lanes

__device__ __forceinline__ float lg_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ float lg_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// the segment that holds row i: (first k in [0, b] with graph_ptr[k] > i) - 1, clamped to [0, b - 1].  Empty graphs are skipped by
// the upper bound; whatever graph_ptr holds, the search ends after log2(b + 1) steps and the result is a valid column.
__device__ __forceinline__ int lg_graph_of(const int* __restrict__ graph_ptr, int b, int i) {
    int lo = 0, hi = b + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (graph_ptr[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    return min(max(lo - 1, 0), b - 1);
}

// both row-norm vectors from one launch, one wave per row
__global__ void __launch_bounds__(256)
lg_row_norms_kernel(const float* __restrict__ zn, int n, const float* __restrict__ zg, int b, int dim, float* __restrict__ an,
                    float* __restrict__ bn) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long)n + b) return;
    const float* z = r < n ? zn + r * dim : zg + (r - n) * dim;
    float acc = 0.f;
    if ((dim & 3) == 0) {
        for (int c = lane * 4; c < dim; c += 256) {
            const float4 v = *reinterpret_cast<const float4*>(z + c);
            acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
    } else {
        for (int c = lane; c < dim; c += 64) acc += z[c] * z[c];
    }
    acc = lg_wave_sum(acc);
    if (lane == 0) {
        if (r < n) an[r] = sqrtf(acc);
        else bn[r - n] = sqrtf(acc);
    }
}

template <bool NORM>
__global__ void __launch_bounds__(256)
lg_fwd_row_kernel(const float* __restrict__ sim, const float* __restrict__ an, const float* __restrict__ bn,
                  const int* __restrict__ graph_ptr, int n, int b, float tau, float eps, float* __restrict__ lse,
                  float* __restrict__ row_loss) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int g = lg_graph_of(graph_ptr, b, i);
    const float a = NORM ? an[i] : 1.f;
    const float* srow = sim + (long)i * b;
    float m = -INFINITY, tpos = 0.f;
    for (int j = lane; j < b; j += 64) {
        const float t = (NORM ? srow[j] / (a * bn[j] + eps) : srow[j]) / tau;
        if (j == g) tpos = t;
        else m = fmaxf(m, t);
    }
    m = lg_wave_max(m);
    tpos = __shfl(tpos, g & 63);
    float acc = 0.f;
    for (int j = lane; j < b; j += 64) {       // the row is 2 KB at most: the second pass reads it from the cache
        const float t = (NORM ? srow[j] / (a * bn[j] + eps) : srow[j]) / tau;
        if (j != g) acc += expf(t - m);
    }
    acc = lg_wave_sum(acc);
    if (lane == 0) {
        const float l = m + logf(acc);
        lse[i] = l;
        row_loss[i] = l - tpos;
    }
}

// the N row losses in fp64, one workgroup, the same order every time
__global__ void __launch_bounds__(256)
lg_loss_sum_kernel(const float* __restrict__ row_loss, int n, float* __restrict__ loss) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += (double)row_loss[i];
    const double s = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)n);
}

// row i: dS'_ij = gs/(N tau) (j == g ? -1 : exp(S'_ij/tau - lse_i)),  H_ij = dS'_ij / (a_i b_j + eps) -> dsim,
// ca_i = -(1/a_i) sum_j H_ij S'_ij b_j (0 for a zero row, torch's norm backward at the origin) and dzn_i = ca_i zn_i; the GEMM
// behind it accumulates H zg on top.  Without the normalisation dsim = dS' and dzn is the GEMM's alone.
template <bool NORM>
__global__ void __launch_bounds__(256)
lg_bwd_row_kernel(const float* __restrict__ sim, const float* __restrict__ an, const float* __restrict__ bn,
                  const float* __restrict__ lse, const int* __restrict__ graph_ptr, const float* __restrict__ zn, int n, int b, int dim,
                  float tau, float eps, const float* __restrict__ gs_dev, float* __restrict__ dsim, float* __restrict__ dzn) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const float gs = gs_dev != nullptr ? gs_dev[0] : 1.f;      // the upstream scalar gradient stays on the device
    const float c = gs / ((float)n * tau);
    const int g = lg_graph_of(graph_ptr, b, i);
    const float a = NORM ? an[i] : 1.f;
    const float l = lse[i];
    const float* srow = sim + (long)i * b;
    float* drow = dsim + (long)i * b;
    float da = 0.f;
    for (int j = lane; j < b; j += 64) {
        const float bj = NORM ? bn[j] : 1.f;
        const float nrm = NORM ? a * bj + eps : 1.f;
        const float s = srow[j] / nrm;
        const float w = j == g ? -1.f : expf(s / tau - l);
        const float H = c * w / nrm;
        drow[j] = H;
        da -= H * s * bj;
    }
    if (!NORM) return;
    da = lg_wave_sum(da);
    const float ca = a > 0.f ? da / a : 0.f;
    const float* zrow = zn + (long)i * dim;
    float* orow = dzn + (long)i * dim;
    if ((dim & 3) == 0) {
        for (int k = lane * 4; k < dim; k += 256) {
            const float4 v = *reinterpret_cast<const float4*>(zrow + k);
            *reinterpret_cast<float4*>(orow + k) = make_float4(ca * v.x, ca * v.y, ca * v.z, ca * v.w);
        }
    } else {
        for (int k = lane; k < dim; k += 64) orow[k] = ca * zrow[k];
    }
}

// first stage of cb_j = -(1/b_j) sum_i H_ij S'_ij a_i: workgroup (chunk, column block) sums the LG_ROW_CHUNK rows of its chunk for
// LG_COLS columns - 64 consecutive columns per wave (256-byte row reads), four row lanes, combined in a fixed order ->
// partial[chunk, j].  A column of the tall matrix has 9 k - 25 k rows: one workgroup per column block would walk them serially.
__global__ void __launch_bounds__(256)
lg_bwd_col_partial_kernel(const float* __restrict__ sim, const float* __restrict__ dsim, const float* __restrict__ an,
                          const float* __restrict__ bn, int n, int b, float eps, float* __restrict__ partial) {
    I3D_CHAIN_PRIO();
    __shared__ float sm[4][LG_COLS];
    const int cx = threadIdx.x & (LG_COLS - 1), ry = threadIdx.x / LG_COLS;
    const int j = blockIdx.y * LG_COLS + cx;
    const int i0 = blockIdx.x * LG_ROW_CHUNK, i1 = min(n, i0 + LG_ROW_CHUNK);
    float acc = 0.f;
    if (j < b) {
        const float bj = bn[j];
        for (int i = i0 + ry; i < i1; i += 4) {
            const float a = an[i];
            const float s = sim[(long)i * b + j] / (a * bj + eps);
            acc -= dsim[(long)i * b + j] * s * a;
        }
    }
    sm[ry][cx] = acc;
    __syncthreads();
    if (ry == 0 && j < b) partial[(long)blockIdx.x * b + j] = ((sm[0][cx] + sm[1][cx]) + sm[2][cx]) + sm[3][cx];
}

// second stage: one wave per column sums the chunks' partials (lanes stride over the chunks, then a butterfly: the order depends on
// the chunk count alone), cb_j = sum / b_j (0 for a zero row) and dzg_j = cb_j zg_j; the GEMM behind it accumulates H^T zn on top.
__global__ void __launch_bounds__(256)
lg_bwd_col_final_kernel(const float* __restrict__ partial, const float* __restrict__ bn, const float* __restrict__ zg, int chunks,
                        int b, int dim, float* __restrict__ dzg) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= b) return;
    float acc = 0.f;
    for (int c = lane; c < chunks; c += 64) acc += partial[(long)c * b + j];
    acc = lg_wave_sum(acc);
    const float bj = bn[j];
    const float cb = bj > 0.f ? acc / bj : 0.f;
    const float* zrow = zg + (long)j * dim;
    float* orow = dzg + (long)j * dim;
    for (int k = lane; k < dim; k += 64) orow[k] = cb * zrow[k];
}

}  // namespace i3d

using namespace i3d;

static inline long lg_al(long v) { return (v + 3) & ~3L; }

// The K = n product dzg = H^T zn has a [b, dim] output and a long K: i3d_gemm_f32 would cut K into slices that meet in fp32
// atomics (csrc/gemm.hip: weight-gradient layouts with K >= 1024).  With scratch for the slices they are summed in a fixed order
// instead; the GEMM takes at most K / 512 slices, so this many floats always hold them.
static inline long lg_slab_floats(int n, int b, int dim) { return ((long)n / 512 + 1) * b * dim; }

extern "C" int i3d_lg_row_chunk(void) { return LG_ROW_CHUNK; }

// scratch layout (floats): an[n] | bn[b] | lse[n] | row_loss[n] | sim[n, b]  (kept for the backward pass)
extern "C" long i3d_lg_ntxent_scratch_floats(int n, int b) {
    if (n < 1 || b < 1) return 0;
    return 3 * lg_al(n) + lg_al(b) + lg_al((long)n * b);
}

// work layout (floats): dsim[n, b] | partial[chunks, b] | the K-slices of H^T zn
extern "C" long i3d_lg_ntxent_work_floats(int n, int b, int dim) {
    if (n < 1 || b < 1 || dim < 1) return 0;
    return lg_al((long)n * b) + lg_al((long)cdiv(n, LG_ROW_CHUNK) * b) + lg_al(lg_slab_floats(n, b, dim));
}

static int lg_check(const char* fn, int n, int b, int dim, float tau) {
    if (n < 1) { set_error("%s: invalid argument: n = %d node rows, at least one is needed", fn, n); return I3D_ERR_INVALID; }
    if (b < 2) { set_error("%s: invalid argument: b = %d graphs, with fewer than two there is no negative", fn, b); return I3D_ERR_INVALID; }
    if (dim < 1) { set_error("%s: invalid argument: dim = %d, a feature width of at least one is needed", fn, dim); return I3D_ERR_INVALID; }
    if (!(tau > 0.f)) { set_error("%s: invalid argument: tau must be positive", fn); return I3D_ERR_INVALID; }
    if ((long)n * b >= (1L << 31)) { set_error("%s: invalid argument: n * b = %ld does not fit 31 bits", fn, (long)n * b); return I3D_ERR_INVALID; }
    return I3D_OK;
}

extern "C" int i3d_lg_ntxent_fwd(const float* zn, const float* zg, const int* graph_ptr, int n, int b, int dim, float tau, float eps,
                                 int norm, float* scratch, float* loss, void* stream) {
    int rc = lg_check(__func__, n, b, dim, tau);
    if (rc != I3D_OK) return rc;
    I3D_CHECK_ARG(zn != nullptr && zg != nullptr && graph_ptr != nullptr && scratch != nullptr && loss != nullptr, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    float* an = scratch;
    float* bn = an + lg_al(n);
    float* lse = bn + lg_al(b);
    float* row_loss = lse + lg_al(n);
    float* sim = row_loss + lg_al(n);
    if (norm) {
        hipLaunchKernelGGL(lg_row_norms_kernel, dim3(cdiv((long)n + b, 4)), dim3(256), 0, s, zn, n, zg, b, dim, an, bn);
        I3D_CHECK_LAUNCH();
    }
    if ((rc = i3d_gemm_f32(0, 1, n, b, dim, zn, dim, zg, dim, sim, b, nullptr, 0, stream)) != I3D_OK) return rc;
    if (norm) hipLaunchKernelGGL(lg_fwd_row_kernel<true>, dim3(cdiv(n, 4)), dim3(256), 0, s, sim, an, bn, graph_ptr, n, b, tau, eps, lse, row_loss);
    else hipLaunchKernelGGL(lg_fwd_row_kernel<false>, dim3(cdiv(n, 4)), dim3(256), 0, s, sim, an, bn, graph_ptr, n, b, tau, eps, lse, row_loss);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(lg_loss_sum_kernel, dim3(1), dim3(256), 0, s, row_loss, n, loss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_lg_ntxent_bwd(const float* zn, const float* zg, const int* graph_ptr, int n, int b, int dim, float tau, float eps,
                                 int norm, const float* scratch, const float* grad_scale_dev, float* work, float* dzn, float* dzg,
                                 void* stream) {
    int rc = lg_check(__func__, n, b, dim, tau);
    if (rc != I3D_OK) return rc;
    I3D_CHECK_ARG(zn != nullptr && zg != nullptr && graph_ptr != nullptr && scratch != nullptr && work != nullptr && dzn != nullptr &&
                      dzg != nullptr, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const float* an = scratch;
    const float* bn = an + lg_al(n);
    const float* lse = bn + lg_al(b);
    const float* sim = lse + 2 * lg_al(n);
    const int chunks = cdiv(n, LG_ROW_CHUNK);
    float* dsim = work;
    float* partial = dsim + lg_al((long)n * b);
    float* slab = partial + lg_al((long)chunks * b);
    const long slab_bytes = lg_slab_floats(n, b, dim) * 4;
    if (norm) {
        hipLaunchKernelGGL(lg_bwd_row_kernel<true>, dim3(cdiv(n, 4)), dim3(256), 0, s, sim, an, bn, lse, graph_ptr, zn, n, b, dim, tau, eps,
                           grad_scale_dev, dsim, dzn);
        I3D_CHECK_LAUNCH();
        hipLaunchKernelGGL(lg_bwd_col_partial_kernel, dim3(chunks, cdiv(b, LG_COLS)), dim3(256), 0, s, sim, dsim, an, bn, n, b, eps,
                           partial);
        I3D_CHECK_LAUNCH();
        hipLaunchKernelGGL(lg_bwd_col_final_kernel, dim3(cdiv(b, 4)), dim3(256), 0, s, partial, bn, zg, chunks, b, dim, dzg);
        I3D_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL(lg_bwd_row_kernel<false>, dim3(cdiv(n, 4)), dim3(256), 0, s, sim, an, bn, lse, graph_ptr, zn, n, b, dim, tau, eps,
                           grad_scale_dev, dsim, dzn);
        I3D_CHECK_LAUNCH();
    }
    const int acc = norm ? 1 : 0;
    if ((rc = i3d_gemm_f32(0, 0, n, dim, b, dsim, b, zg, dim, dzn, dim, nullptr, acc, stream)) != I3D_OK) return rc;
    return i3d_gemm_f32_ws(1, 0, b, dim, n, dsim, b, zn, dim, dzg, dim, nullptr, acc, slab, slab_bytes, stream);
}
