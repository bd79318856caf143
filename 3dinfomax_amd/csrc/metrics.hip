// Contrastive monitoring metrics of the pre-training loop in one device pass.
//
// Replaces the nine metric modules of configs_clean/pre-train_QM9.yml:15-24 - reference trainer/metrics.py:161-174
// (DimensionCovariance, BatchVariance), :212-333 (Alignment, Uniformity, TruePositiveRate, TrueNegativeRate,
// ContrastiveAccuracy, PositiveSimilarity), :443-463 (NegativeSimilarity) with commons/losses.py:946-959 - which the
// trainer evaluates every `log_iterations` (= 2) steps, each through its own chain of small ops and its own `.item()`
// (trainer/self_supervised_trainer.py:31-50).  Here ONE C call per pair of tensors (i3d_contrastive_metrics) and ONE
// device-to-host copy of its fp64 result.
//
// Formulation: every statistic that is a difference of large numbers in its textbook form is computed from CENTRED values, as the
// reference does (it subtracts the rows, uses torch.pdist, centres before the covariance, and torch.std is two-pass) - never from
// uncentred second moments (g_ii + g_jj - 2 g_ij on raw rows, q - s^2 / n, C_ab - s_a s_b / n lose every digit once the column
// means exceed the spread: embeddings with a common offset, a collapsed batch, well-aligned views):
//     centre      per view: column mean (fp64), c = z - mean rounded to fp32 once, var_j = sum_i (z_ij - mean_j)^2 / (n - 1) in fp64
//     row prep    |z1_i|, |z2_i| and |z1_i - z2_i|^alpha from the rows themselves (differences and sums in fp64)
//     products    G1 = c1 c1^T, G2 = c2 c2^T (pairwise distances are translation invariant: |z_i - z_j|^2 = g_ii + g_jj - 2 g_ij of the
//                 CENTRED rows), S = z1 z2[:B1]^T (the cosines are not: raw rows), C = c^T c per view (covariance * (n - 1));
//                 the library's GEMM pinned to exact fp32 products (native fp32 MFMA, no K-slices) whatever the process-wide setting is
//     row stats   per row i the cosine sums / rates / Gaussian potentials below; per row a of C the squared off-diagonal covariances
//     finish      one workgroup adds the rows' terms in row order in fp64
// Every sum has a fixed order, no atomics: the same bits on every run.
#include "common.h"

namespace i3d {
namespace {

constexpr int RS = 8;                     // statistics per row of contrastive_rowstats_kernel
constexpr int MC_CW = 16, MC_RL = 16;     // centre kernel: 16 columns x 16 row lanes (as batchstat.hip)

struct McViews {
    const float* z[2];
    float* c[2];
    double* mom[2];      // per view: mean [dim] | unbiased variance [dim]
    int n[2], dim[2];
};

__device__ __forceinline__ double mc_col_sum(double v, double (*sm)[MC_CW], int ry, int cx) {
    __syncthreads();
    sm[ry][cx] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < MC_RL; ++k) t += sm[k][cx];
    return t;
}

// grid (column tiles of the wider view, views).  The mean first, then the centred values (never E[x^2] - E[x]^2).
__global__ void __launch_bounds__(256)
metrics_centre_kernel(McViews v) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[MC_RL][MC_CW];
    const int view = blockIdx.y, cx = threadIdx.x % MC_CW, ry = threadIdx.x / MC_CW;
    const int n = v.n[view], dim = v.dim[view];
    if ((int)blockIdx.x * MC_CW >= dim) return;                      // (whole workgroup: the narrower view has fewer tiles)
    const int j = blockIdx.x * MC_CW + cx;
    const bool ok = j < dim;
    const float* z = v.z[view] + (ok ? j : 0);
    double s = 0.0;
    if (ok)
        for (int i = ry; i < n; i += MC_RL) s += (double)z[(long)i * dim];
    const double mean = mc_col_sum(s, sm, ry, cx) / n;
    float* c = v.c[view];
    double q = 0.0;
    if (ok)
        for (int i = ry; i < n; i += MC_RL) {
            const double d = (double)z[(long)i * dim] - mean;
            q += d * d;
            c[(long)i * dim + j] = (float)d;
        }
    const double var = mc_col_sum(q, sm, ry, cx) / (n - 1);          // n = 1: 0 / 0 = NaN, as torch.std
    if (ok && ry == 0) {
        v.mom[view][j] = mean;
        v.mom[view][dim + j] = var;
    }
}

// row i (one workgroup) of z1 [B1, D], z2 [B2, D]: prep[i] = {|z1_i|, |z2_i|, |z1_i - z2_i|^alpha, 0} (i >= B1: the second only)
__global__ void __launch_bounds__(256)
metrics_row_prep_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int B1, int D, float alpha,
                        float* __restrict__ prep) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const int i = blockIdx.x;
    const bool both = i < B1;
    const float* a = z1 + (long)(both ? i : 0) * D;
    const float* b = z2 + (long)i * D;
    double s1 = 0.0, s2 = 0.0, sd = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double y = (double)b[d];
        s2 += y * y;
        if (both) {
            const double x = (double)a[d], e = x - y;
            s1 += x * x;
            sd += e * e;
        }
    }
    s1 = block_sum_f64(s1, sm);
    s2 = block_sum_f64(s2, sm);
    sd = block_sum_f64(sd, sm);
    if (threadIdx.x == 0) {
        float* o = prep + (long)i * 4;
        o[0] = (float)sqrt(s1);
        o[1] = (float)sqrt(s2);
        o[2] = both ? (float)pow(sqrt(sd), (double)alpha) : 0.f;
        o[3] = 0.f;
    }
}

__device__ __forceinline__ float block_sum(float v, float* sm) {
    // fixed-order tree over the 256 threads of the block
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    float r = sm[0];
    __syncthreads();
    return r;
}

// row i (one workgroup): S = z1 z2^T [B1, B1] (z2: first B1 rows, RAW rows), G1 = c1 c1^T [B1, B1], G2 = c2 c2^T [B2, B2] (CENTRED
// rows), prep as above
//   out[i][0] = sum_j cos_ij   out[i][1] = cos_ii   out[i][2] = [(cos_ii + 1)/2 > thr]   out[i][3] = #{j != i : (cos_ij+1)/2 <= thr}
//   out[i][4] = |z1_i - z2_i|^alpha   out[i][5] = sum_{j>i} exp(-t |z1_i - z1_j|^2)   out[i][6] = the same for z2 (i < B2)
//   out[i][7] = <z1_i, z2_i> / (max(|z1_i|, 1e-8) max(|z2_i|, 1e-8)): PositiveSimilarity is F.cosine_similarity in the reference (a zero
//               row counts 0), the matrix-based metrics divide by the plain norms (a zero row makes them NaN)
__global__ void __launch_bounds__(256)
contrastive_rowstats_kernel(const float* __restrict__ S, const float* __restrict__ G1, const float* __restrict__ G2,
                            const float* __restrict__ prep, int B1, int B2, float thr, float t, float* __restrict__ out) {
    I3D_CHAIN_PRIO();
    __shared__ float sm[256];
    const int i = blockIdx.x;
    float s_cos = 0.f, s_tn = 0.f, s_u1 = 0.f, s_u2 = 0.f;
    if (i < B1) {
        const float n1 = prep[(long)i * 4];
        const float g1ii = G1[(long)i * B1 + i];
        for (int j = threadIdx.x; j < B1; j += 256) {
            const float c = S[(long)i * B1 + j] / (n1 * prep[(long)j * 4 + 1]);
            s_cos += c;
            if (j != i && !((c + 1.f) * 0.5f > thr)) s_tn += 1.f;
            if (j > i) s_u1 += expf(-t * fmaxf(g1ii + G1[(long)j * B1 + j] - 2.f * G1[(long)i * B1 + j], 0.f));
        }
    }
    {
        const float g2ii = G2[(long)i * B2 + i];
        for (int j = i + 1 + threadIdx.x; j < B2; j += 256)
            s_u2 += expf(-t * fmaxf(g2ii + G2[(long)j * B2 + j] - 2.f * G2[(long)i * B2 + j], 0.f));
    }
    s_cos = block_sum(s_cos, sm);
    s_tn = block_sum(s_tn, sm);
    s_u1 = block_sum(s_u1, sm);
    s_u2 = block_sum(s_u2, sm);
    if (threadIdx.x == 0) {
        float* o = out + (long)i * RS;
        float cii = 0.f, tp = 0.f, al = 0.f, cpos = 0.f;
        if (i < B1) {
            const float n1 = prep[(long)i * 4], n2 = prep[(long)i * 4 + 1], sii = S[(long)i * B1 + i];
            cii = sii / (n1 * n2);
            cpos = sii / (fmaxf(n1, 1e-8f) * fmaxf(n2, 1e-8f));
            tp = ((cii + 1.f) * 0.5f > thr) ? 1.f : 0.f;
            al = prep[(long)i * 4 + 2];
        }
        o[0] = s_cos; o[1] = cii; o[2] = tp; o[3] = s_tn; o[4] = al; o[5] = s_u1; o[6] = s_u2; o[7] = cpos;
    }
}

struct McCov {
    const float* C[2];      // c^T c [dim, dim] per view
    double* part[2];        // [dim] per view
    int n[2], dim[2];
};

// row a of C = c^T c (centred columns) of view blockIdx.y: part[a] = sum_{b != a} (C_ab / (n - 1))^2   (cov_loss's off-diagonal squares)
__global__ void __launch_bounds__(256)
cov_rowstats_kernel(McCov v) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const int view = blockIdx.y, a = blockIdx.x, D = v.dim[view], n = v.n[view];
    if (a >= D) return;
    const float* C = v.C[view] + (long)a * D;
    const double inv_n1 = 1.0 / (double)(n - 1);                     // n = 1: inf, 0 * inf = NaN as the reference's 0 / 0
    double acc = 0.0;
    for (int b = threadIdx.x; b < D; b += 256) {
        if (b == a) continue;
        const double cov = (double)C[b] * inv_n1;
        acc += cov * cov;
    }
    acc = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) v.part[view][a] = acc;
}

// one workgroup: out[0..7] = column sums of rows [B2, 8] (rows == nullptr: zeros), out[8 + view] = sum of the view's covariance parts:
// 32 row lanes per column, then the lanes in order; the covariance parts through block_sum_f64: fixed orders
__global__ void __launch_bounds__(256)
metrics_finish_kernel(const float* __restrict__ rows, int B2, McCov v, double* __restrict__ out) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[32][RS];
    __shared__ double sm4[4];
    const int k = threadIdx.x % RS, lane = threadIdx.x / RS;
    double s = 0.0;
    if (rows != nullptr)
        for (int i = lane; i < B2; i += 32) s += (double)rows[(long)i * RS + k];
    sm[lane][k] = s;
    __syncthreads();
    if (threadIdx.x < RS) {
        double tot = 0.0;
        for (int l = 0; l < 32; ++l) tot += sm[l][threadIdx.x];
        out[threadIdx.x] = tot;
    }
    for (int view = 0; view < 2; ++view) {
        double p = 0.0;
        for (int a = threadIdx.x; a < v.dim[view]; a += 256) p += v.part[view][a];
        p = block_sum_f64(p, sm4);
        if (threadIdx.x == 0) out[RS + view] = p;
    }
}

inline long al4(long n) { return (n + 3) & ~3L; }

}  // namespace
}  // namespace i3d

using namespace i3d;

extern "C" long i3d_contrastive_metrics_out_doubles(int D1, int D2) { return 10 + 3L * D1 + 3L * D2; }

extern "C" long i3d_contrastive_metrics_work_floats(int B1, int B2, int D1, int D2, int pairwise) {
    long n = al4((long)B1 * D1) + al4((long)B2 * D2) + al4((long)D1 * D1) + al4((long)D2 * D2);
    if (pairwise) n += 2 * al4((long)B1 * B1) + al4((long)B2 * B2) + al4((long)B2 * 4) + al4((long)B2 * RS);
    return n;
}

// z1 [B1, D1], z2 [B2, D2].  pairwise != 0 (needs D1 == D2, B2 >= B1: rows of z2 from B1 on are the appended "noisy" samples): all
// statistics; pairwise == 0: the per-tensor ones only (out[0..7] = 0).
// out (fp64, i3d_contrastive_metrics_out_doubles): [0..7] the totals of contrastive_rowstats_kernel's columns | [8], [9] per view the
// sum of the squared off-diagonal covariances | mean1 [D1] | var1 [D1] | mean2 [D2] | var2 [D2] | scratch [D1 + D2]
extern "C" int i3d_contrastive_metrics(const float* z1, const float* z2, int B1, int B2, int D1, int D2, int pairwise, float threshold,
                                       float t, float alpha, float* work, double* out, void* stream) {
    I3D_CHECK_ARG(z1 != nullptr && z2 != nullptr && work != nullptr && out != nullptr, "null pointer");
    I3D_CHECK_ARG(B1 > 0 && B2 > 0 && D1 > 0 && D2 > 0, "bad shape");
    I3D_CHECK_ARG(!pairwise || (D1 == D2 && B2 >= B1), "pairwise statistics need equal widths and B1 <= B2");
    I3D_CHECK_ARG((long)B2 * B2 < (1L << 31) && (long)B2 * D2 < (1L << 31) && (long)B1 * D1 < (1L << 31) && (long)D1 * D1 < (1L << 31) &&
                      (long)D2 * D2 < (1L << 31), "matrix beyond 2^31 elements");
    hipStream_t s = (hipStream_t)stream;
    float* c1 = work;
    float* c2 = c1 + al4((long)B1 * D1);
    float* C1 = c2 + al4((long)B2 * D2);
    float* C2 = C1 + al4((long)D1 * D1);
    float* G1 = C2 + al4((long)D2 * D2);
    float* S = G1 + al4((long)B1 * B1);
    float* G2 = S + al4((long)B1 * B1);
    float* prep = G2 + al4((long)B2 * B2);
    float* rows = prep + al4((long)B2 * 4);
    double* mom1 = out + 10;
    double* mom2 = mom1 + 2L * D1;
    double* part1 = mom2 + 2L * D2;

    McViews v = {{z1, z2}, {c1, c2}, {mom1, mom2}, {B1, B2}, {D1, D2}};
    hipLaunchKernelGGL(metrics_centre_kernel, dim3(cdiv(D1 > D2 ? D1 : D2, MC_CW), 2), dim3(256), 0, s, v);
    I3D_CHECK_LAUNCH();
    if (pairwise) {
        hipLaunchKernelGGL(metrics_row_prep_kernel, dim3(B2), dim3(256), 0, s, z1, z2, B1, D1, alpha, prep);
        I3D_CHECK_LAUNCH();
    }
    // exact fp32 products for these five, whatever the process runs its training GEMMs with (host-side switches read at launch);
    // splits = 1: no K-slices, so no atomics for a long batch axis
    const int was_bf16 = i3d_get_matmul_precision(), was_split = i3d_get_fp32_products();
    i3d_set_matmul_precision(0);
    i3d_set_fp32_products(0);
    int rc = I3D_OK;
    if (pairwise) {
        rc = i3d_gemm_f32_ex(0, 1, B1, B1, D1, c1, D1, c1, D1, G1, B1, nullptr, 0, -1, 1, nullptr, 0, stream);
        if (rc == I3D_OK) rc = i3d_gemm_f32_ex(0, 1, B2, B2, D2, c2, D2, c2, D2, G2, B2, nullptr, 0, -1, 1, nullptr, 0, stream);
        if (rc == I3D_OK) rc = i3d_gemm_f32_ex(0, 1, B1, B1, D1, z1, D1, z2, D2, S, B1, nullptr, 0, -1, 1, nullptr, 0, stream);
    }
    if (rc == I3D_OK) rc = i3d_gemm_f32_ex(1, 0, D1, D1, B1, c1, D1, c1, D1, C1, D1, nullptr, 0, -1, 1, nullptr, 0, stream);
    if (rc == I3D_OK) rc = i3d_gemm_f32_ex(1, 0, D2, D2, B2, c2, D2, c2, D2, C2, D2, nullptr, 0, -1, 1, nullptr, 0, stream);
    i3d_set_matmul_precision(was_bf16);
    i3d_set_fp32_products(was_split);
    if (rc != I3D_OK) return rc;
    if (pairwise) {
        hipLaunchKernelGGL(contrastive_rowstats_kernel, dim3(B2), dim3(256), 0, s, S, G1, G2, prep, B1, B2, threshold, t, rows);
        I3D_CHECK_LAUNCH();
    }
    McCov cv = {{C1, C2}, {part1, part1 + D1}, {B1, B2}, {D1, D2}};
    hipLaunchKernelGGL(cov_rowstats_kernel, dim3(D1 > D2 ? D1 : D2, 2), dim3(256), 0, s, cv);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(256), 0, s, pairwise ? rows : nullptr, B2, cv, out);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
