// The pairwise members of the family in which the 2D network predicts a diagonal Gaussian per molecule: z1 [B, 2D] = mean m | log-variance
// s, z2 = C conformer embeddings of dimension D per molecule.  NTXentLikelihoodLoss (reference commons/losses.py:537-595) with the
// PositiveProb / NegativeProb metrics (trainer/metrics.py:336-395), and JSDMultiplePositivesLoss (:317-391).  The reference forms the
// first from B^2 torch.distributions.Normal objects in a Python double loop and the second from two MultivariateNormals over [B, B, D, D]
// covariance tensors; here each is one pass over the B^2 C D (B^2 D) terms with [B, B] fp64 buffers, every term in fp64.
//
// Likelihood, sigma_id = exp(s_id / 2), t = (x - m_id) / sigma_id, x = z2[j mol_stride + c conf_stride + d] (the loss reads z2 molecule
// major, the metrics conformer major - strides, no copy):
//
//   L[i, j] = 1 / (C D) sum_{c, d} exp(-t^2 / 2) / (sigma_id sqrt(2 pi))         rows i: the 2D view; a mean of densities, no product
//   loss    = 1 / B sum_i ( log sum_{j != i} exp(L_ij / tau) - L_ii / tau )       the negatives summed directly (never `row sum -
//                                                                                positive`), the row maximum taken out of the exponent
//   forward   gp_lik_fwd: one workgroup per (i, 8 columns j); a thread owns features d (stride 256) and computes 1 / sigma once for the
//             8 C terms it feeds; 8 workgroup sums.  gp_lik_row: one workgroup per row: maximum, sum, log.  gp_mean: the B row terms.
//   backward  G_ij = g / (B tau) (-delta_ij + (1 - delta_ij) exp(L_ij / tau) / den_i)  (gp_lik_grad, [B, B]); then one owner per output
//             element, both passes recompute p = the density: dp/dm = p t / sigma, dp/ds = p (t^2 - 1) / 2, dp/dx = -p t / sigma.
//             dz1[i] sums over j, dz2[j] over i: a workgroup takes 64 features, its four waves split the summed index and their partial
//             sums are added in wave order through LDS.  The dz2 pass keeps 4 conformers per thread (one exp(-s / 2) per 4 terms).
//
// JSD, rows a: the 3D view (m2 = conformer mean, v2 = unbiased conformer variance, two-pass, no epsilon; w = 1 / (v2 + 1e-5)), columns b:
// the 2D view:
//
//   S[a, b] = 0.5 ( log(prod_d v2_ad + 1e-5) - sum_d s_bd - D + sum_d w_ad (exp(s_bd) + (m2_ad - m1_bd)^2) )
//   loss    = -1 / B sum_a log( S_aa / sum_{b != a} S_ab )                        S is not exponentiated; a negative ratio gives NaN
//   forward   gp_jsd_stat: per molecule the product of its non-zero v2 and the number of zero ones (fp64; the product of all is 0 when
//             there is one).  gp_jsd_pair: one workgroup per (b, 8 rows a): exp(s_bd) once per thread and feature, the conformer
//             statistics recomputed per row (C reads), direct differences.  gp_jsd_row, gp_mean.
//   backward  G_ab = g / B (-delta_ab / S_aa + (1 - delta_ab) / den_a) needs no matrix (two numbers per row).  dS/dm1 = -w (m2 - m1),
//             dS/ds = (w exp(s) - 1) / 2, dS/dm2 = w (m2 - m1), dS/dv2_ad = (prod_{d' != d} v2_ad' / (prod v2 + 1e-5) - w^2 (exp(s) +
//             (m2 - m1)^2)) / 2, dz2[a, c, d] = dm2 / C + dv2 2 (z2 - m2) / (C - 1).  Owners and wave split as above.
//
// Sums have a fixed order (block_sum_f64 of common.h, the wave-ordered LDS sum here), no atomics, nothing larger than [B, B] doubles.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace i3d {

constexpr int GP_TILE = 8;          // columns (likelihood) or rows (JSD) of the pair matrix per workgroup of the forward kernels
constexpr int GP_CONF = 4;          // conformers per owner thread of the likelihood's dz2 pass
constexpr double GP_INV_SQRT_2PI = 0.39894228040143267794;
constexpr double JSD_EPS = 1e-5;

// as block_sum_f64: the maximum over the 256 threads (NaN entries are ignored by fmax; they reach the result through the sum after it)
__device__ __forceinline__ double block_max_f64(double v, double* sm) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    return fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}

__device__ __forceinline__ double block_prod_f64(double v, double* sm) {
    for (int o = 32; o > 0; o >>= 1) v *= __shfl_xor(v, o);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    return ((sm[0] * sm[1]) * sm[2]) * sm[3];
}

// the owner passes: thread (wave w, lane) holds the partial sum of feature `lane` over the indices w, w + 4, ...; returns their sum in
// wave order (valid in wave 0)
__device__ __forceinline__ double wave_ordered_sum(double v, double (*sm)[WAVE]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    sm[w][lane] = v;
    __syncthreads();
    return ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
}

// ---- likelihood ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
gp_lik_fwd_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int B, int C, int D, long ms, long cs, int tiles,
                  double* __restrict__ L) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const long i = blockIdx.x / tiles;
    const int j0 = (int)(blockIdx.x % tiles) * GP_TILE;
    const float* m1 = z1 + i * 2 * D;
    const float* s1 = m1 + D;
    double acc[GP_TILE];
#pragma unroll
    for (int k = 0; k < GP_TILE; ++k) acc[k] = 0.;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double m = (double)m1[d], is = exp(-0.5 * (double)s1[d]);
#pragma unroll
        for (int k = 0; k < GP_TILE; ++k) {
            if (j0 + k < B) {
                const float* x = z2 + (long)(j0 + k) * ms + d;
                double q = 0.;
                for (int c = 0; c < C; ++c) {
                    const double t = ((double)x[(long)c * cs] - m) * is;
                    q += exp(-0.5 * t * t);
                }
                acc[k] += q * is;
            }
        }
    }
    const double scale = GP_INV_SQRT_2PI / ((double)C * (double)D);
#pragma unroll
    for (int k = 0; k < GP_TILE; ++k) {
        const double v = block_sum_f64(acc[k], sm);
        if (threadIdx.x == 0 && j0 + k < B) L[i * B + j0 + k] = v * scale;
    }
}

// rows [B, 2] = { log den_i, l_i = log den_i - L_ii / tau }
__global__ void __launch_bounds__(256)
gp_lik_row_kernel(const double* __restrict__ L, int B, double tau, double* __restrict__ rows) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const long i = blockIdx.x;
    const double* row = L + i * B;
    double mx = -INFINITY;
    for (int j = threadIdx.x; j < B; j += 256)
        if (j != i) mx = fmax(mx, row[j] / tau);
    mx = block_max_f64(mx, sm);
    double s = 0.;
    for (int j = threadIdx.x; j < B; j += 256)
        if (j != i) s += exp(row[j] / tau - mx);
    s = block_sum_f64(s, sm);
    if (threadIdx.x == 0) {
        const double ld = mx + log(s);
        rows[i * 2] = ld;
        rows[i * 2 + 1] = ld - row[i] / tau;
    }
}

// loss[0] = 1 / B sum_i rows[i stride + offset]
__global__ void __launch_bounds__(256)
gp_mean_kernel(const double* __restrict__ rows, int B, int stride, int offset, float* __restrict__ loss) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double acc = 0.;
    for (int i = threadIdx.x; i < B; i += 256) acc += rows[(long)i * stride + offset];
    acc = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) loss[0] = (float)(acc / (double)B);
}

// out[0] = mean_i L_ii, out[1] = mean_i sum_{j != i} L_ij
__global__ void __launch_bounds__(256)
gp_lik_probs_kernel(const double* __restrict__ L, int B, double* __restrict__ out) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double pos = 0., neg = 0.;
    const long n = (long)B * B;
    for (long k = threadIdx.x; k < n; k += 256) {
        const double v = L[k];
        if (k / B == k % B) pos += v;
        else neg += v;
    }
    pos = block_sum_f64(pos, sm);
    neg = block_sum_f64(neg, sm);
    if (threadIdx.x == 0) {
        out[0] = pos / (double)B;
        out[1] = neg / (double)B;
    }
}

__global__ void __launch_bounds__(256)
gp_lik_grad_kernel(const double* __restrict__ L, const double* __restrict__ rows, int B, double tau, const float* __restrict__ gs_dev,
                   double* __restrict__ G) {
    I3D_CHAIN_PRIO();
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= (long)B * B) return;
    const long i = k / B, j = k % B;
    const double gs = (gs_dev ? (double)gs_dev[0] : 1.) / ((double)B * tau);
    G[k] = i == j ? -gs : gs * exp(L[k] / tau - rows[i * 2]);
}

// dz1[i, :] of 64 features: the waves split j
__global__ void __launch_bounds__(256)
gp_lik_dz1_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int B, int C, int D, long ms, long cs, int chunks,
                  const double* __restrict__ G, float* __restrict__ dz1) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4][WAVE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long i = blockIdx.x / chunks;
    const int d = (int)(blockIdx.x % chunks) * WAVE + lane;
    double gm = 0., gv = 0., is = 0.;
    if (d < D) {
        const double m = (double)z1[i * 2 * D + d];
        is = exp(-0.5 * (double)z1[i * 2 * D + D + d]);
        for (int j = w; j < B; j += 4) {
            const double g = G[i * B + j];
            const float* x = z2 + (long)j * ms + d;
            double am = 0., av = 0.;
            for (int c = 0; c < C; ++c) {
                const double t = ((double)x[(long)c * cs] - m) * is, p = exp(-0.5 * t * t);
                am += p * t;
                av += p * (t * t - 1.);
            }
            gm += g * am;
            gv += g * av;
        }
    }
    gm = wave_ordered_sum(gm, sm);
    gv = wave_ordered_sum(gv, sm);
    if (w == 0 && d < D) {
        const double k = is * GP_INV_SQRT_2PI / ((double)C * (double)D);          // the density is k exp(-t^2 / 2)
        dz1[i * 2 * D + d] = (float)(k * is * gm);
        dz1[i * 2 * D + D + d] = (float)(0.5 * k * gv);
    }
}

// dz2[j, c0 .. c0 + 3, :] of 64 features: the waves split i
__global__ void __launch_bounds__(256)
gp_lik_dz2_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int B, int C, int D, long ms, long cs, int chunks,
                  int groups, const double* __restrict__ G, float* __restrict__ dz2) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4][WAVE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int d = (int)(blockIdx.x % chunks) * WAVE + lane;
    const long r = blockIdx.x / chunks;
    const int c0 = (int)(r % groups) * GP_CONF;
    const long j = r / groups;
    double acc[GP_CONF], x[GP_CONF];
#pragma unroll
    for (int k = 0; k < GP_CONF; ++k) {
        acc[k] = 0.;
        x[k] = (d < D && c0 + k < C) ? (double)z2[j * ms + (long)(c0 + k) * cs + d] : 0.;
    }
    if (d < D) {
        for (int i = w; i < B; i += 4) {
            const double m = (double)z1[(long)i * 2 * D + d], is = exp(-0.5 * (double)z1[(long)i * 2 * D + D + d]);
            const double gk = G[(long)i * B + j] * is * is;
#pragma unroll
            for (int k = 0; k < GP_CONF; ++k) {
                const double t = (x[k] - m) * is;
                acc[k] -= gk * (exp(-0.5 * t * t) * t);
            }
        }
    }
    const double scale = GP_INV_SQRT_2PI / ((double)C * (double)D);
#pragma unroll
    for (int k = 0; k < GP_CONF; ++k) {
        const double v = wave_ordered_sum(acc[k], sm);
        if (w == 0 && d < D && c0 + k < C) dz2[j * ms + (long)(c0 + k) * cs + d] = (float)(v * scale);
    }
}

// ---- JSD ------------------------------------------------------------------------------------------------------------------------------------
// mean and unbiased variance (no epsilon) of feature d over the C conformers of one molecule, two-pass; za = z2 + a C D
__device__ __forceinline__ void gp_conformer_stats(const float* __restrict__ za, int C, int D, int d, double& mean, double& var) {
    double s = 0.;
    for (int c = 0; c < C; ++c) s += (double)za[(long)c * D + d];
    mean = s / (double)C;
    double q = 0.;
    for (int c = 0; c < C; ++c) {
        const double t = (double)za[(long)c * D + d] - mean;
        q += t * t;
    }
    var = q / (double)(C - 1);
}

// astat [B, 2] = { product of the non-zero v2_ad over d, number of zero ones }
__global__ void __launch_bounds__(256)
gp_jsd_stat_kernel(const float* __restrict__ z2, int C, int D, double* __restrict__ astat) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const long a = blockIdx.x;
    const float* za = z2 + a * C * D;
    double p = 1., nz = 0.;
    for (int d = threadIdx.x; d < D; d += 256) {
        double m2, var;
        gp_conformer_stats(za, C, D, d, m2, var);
        if (var == 0.) nz += 1.;
        else p *= var;
    }
    p = block_prod_f64(p, sm);
    nz = block_sum_f64(nz, sm);
    if (threadIdx.x == 0) {
        astat[a * 2] = p;
        astat[a * 2 + 1] = nz;
    }
}

__global__ void __launch_bounds__(256)
gp_jsd_pair_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int B, int C, int D, int tiles,
                   const double* __restrict__ astat, double* __restrict__ S) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const long b = blockIdx.x / tiles;
    const int a0 = (int)(blockIdx.x % tiles) * GP_TILE;
    const float* m1 = z1 + b * 2 * D;
    const float* s1 = m1 + D;
    double acc[GP_TILE], ssum = 0.;
#pragma unroll
    for (int k = 0; k < GP_TILE; ++k) acc[k] = 0.;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double m = (double)m1[d], s = (double)s1[d], e = exp(s);
        ssum += s;
#pragma unroll
        for (int k = 0; k < GP_TILE; ++k) {
            if (a0 + k < B) {
                double m2, var;
                gp_conformer_stats(z2 + (long)(a0 + k) * C * D, C, D, d, m2, var);
                const double dl = m2 - m;
                acc[k] += (e + dl * dl) / (var + JSD_EPS);
            }
        }
    }
    ssum = block_sum_f64(ssum, sm);
#pragma unroll
    for (int k = 0; k < GP_TILE; ++k) {
        const double v = block_sum_f64(acc[k], sm);
        const long a = a0 + k;
        if (threadIdx.x == 0 && a < B) {
            const double prod = astat[a * 2 + 1] > 0. ? 0. : astat[a * 2];
            S[a * B + b] = 0.5 * (log(prod + JSD_EPS) - ssum - (double)D + v);
        }
    }
}

// rows [B, 3] = { S_aa, den_a = sum_{b != a} S_ab, -log(S_aa / den_a) }
__global__ void __launch_bounds__(256)
gp_jsd_row_kernel(const double* __restrict__ S, int B, double* __restrict__ rows) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const long a = blockIdx.x;
    const double* row = S + a * B;
    double den = 0.;
    for (int b = threadIdx.x; b < B; b += 256)
        if (b != a) den += row[b];
    den = block_sum_f64(den, sm);
    if (threadIdx.x == 0) {
        rows[a * 3] = row[a];
        rows[a * 3 + 1] = den;
        rows[a * 3 + 2] = -log(row[a] / den);
    }
}

// dz1[b, :] of 64 features: the waves split a
__global__ void __launch_bounds__(256)
gp_jsd_dz1_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int B, int C, int D, int chunks,
                  const double* __restrict__ rows, const float* __restrict__ gs_dev, float* __restrict__ dz1) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4][WAVE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long b = blockIdx.x / chunks;
    const int d = (int)(blockIdx.x % chunks) * WAVE + lane;
    const double gs = (gs_dev ? (double)gs_dev[0] : 1.) / (double)B;
    double gm = 0., gw = 0., gt = 0.;
    if (d < D) {
        const double m = (double)z1[b * 2 * D + d];
        for (int a = w; a < B; a += 4) {
            const double g = a == b ? -gs / rows[(long)a * 3] : gs / rows[(long)a * 3 + 1];
            double m2, var;
            gp_conformer_stats(z2 + (long)a * C * D, C, D, d, m2, var);
            const double wt = 1. / (var + JSD_EPS);
            gm += g * (wt * (m2 - m));
            gw += g * wt;
            gt += g;
        }
    }
    gm = wave_ordered_sum(gm, sm);
    gw = wave_ordered_sum(gw, sm);
    gt = wave_ordered_sum(gt, sm);
    if (w == 0 && d < D) {
        dz1[b * 2 * D + d] = (float)(-gm);
        dz1[b * 2 * D + D + d] = (float)(0.5 * (gw * exp((double)z1[b * 2 * D + D + d]) - gt));
    }
}

// dz2[a, :, :] of 64 features: the waves split b
__global__ void __launch_bounds__(256)
gp_jsd_dz2_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int B, int C, int D, int chunks,
                  const double* __restrict__ astat, const double* __restrict__ rows, const float* __restrict__ gs_dev,
                  float* __restrict__ dz2) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4][WAVE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long a = blockIdx.x / chunks;
    const int d = (int)(blockIdx.x % chunks) * WAVE + lane;
    const float* za = z2 + a * C * D;
    const double gs = (gs_dev ? (double)gs_dev[0] : 1.) / (double)B;
    const double gdiag = -gs / rows[a * 3], goff = gs / rows[a * 3 + 1];
    double am = 0., av = 0., m2 = 0.;
    if (d < D) {
        double var;
        gp_conformer_stats(za, C, D, d, m2, var);
        const double wt = 1. / (var + JSD_EPS);
        // d log(prod v2 + 1e-5) / d v2_ad = (product of the other features' v2) / (prod v2 + 1e-5); with zeros among them as torch.prod's
        // backward: one zero - the product of the others where the zero is, 0 elsewhere; more - 0
        const double pn = astat[a * 2], nz = astat[a * 2 + 1];
        const double others = nz == 0. ? pn / var : ((nz == 1. && var == 0.) ? pn : 0.);
        const double ldet = others / ((nz > 0. ? 0. : pn) + JSD_EPS);
        for (int b = w; b < B; b += 4) {
            const double g = b == a ? gdiag : goff;
            const double dl = m2 - (double)z1[(long)b * 2 * D + d], e = exp((double)z1[(long)b * 2 * D + D + d]);
            am += g * (wt * dl);
            av += g * (ldet - wt * wt * (e + dl * dl));
        }
    }
    am = wave_ordered_sum(am, sm);
    av = wave_ordered_sum(av, sm);
    if (w == 0 && d < D) {
        const double gmean = am / (double)C, gvar = av / (double)(C - 1);          // 0.5 dS/dv2 times 2 (z2 - m2) / (C - 1)
        float* ga = dz2 + a * C * D;
        for (int c = 0; c < C; ++c) ga[(long)c * D + d] = (float)(gmean + gvar * ((double)za[(long)c * D + d] - m2));
    }
}

}  // namespace i3d

using namespace i3d;

static int gp_check(int batch, int conf, int dim, int min_conf) {
    I3D_CHECK_ARG(batch >= 2, "batch below 2: no negatives");
    I3D_CHECK_ARG(conf >= min_conf, min_conf == 2 ? "fewer than two conformers per molecule: their variance is undefined"
                                                  : "conformer count below 1");
    I3D_CHECK_ARG(dim >= 1, "feature count below 1");
    I3D_CHECK_ARG((long)batch * cdiv(batch, GP_TILE) <= INT_MAX && (long)batch * cdiv(conf, GP_CONF) * cdiv(dim, WAVE) <= INT_MAX &&
                      cdiv((long)batch * batch, 256) <= INT_MAX,
                  "more workgroups than one launch takes");
    return I3D_OK;
}

// the two layouts of z2 [B C, D]: molecule major (row j C + c) and conformer major (row c B + j)
static int gp_check_strides(int batch, int conf, int dim, long ms, long cs) {
    I3D_CHECK_ARG((ms == (long)conf * dim && cs == dim) || (ms == dim && cs == (long)batch * dim),
                  "z2 strides are neither molecule major nor conformer major");
    return I3D_OK;
}

extern "C" int i3d_gauss_lik_fwd(const float* z1, const float* z2, int batch, int conf, int dim, long mol_stride, long conf_stride,
                                 double* lik, void* stream) {
    if (int rc = gp_check(batch, conf, dim, 1)) return rc;
    if (int rc = gp_check_strides(batch, conf, dim, mol_stride, conf_stride)) return rc;
    I3D_CHECK_ARG(z1 && z2 && lik, "null pointer");
    const int tiles = cdiv(batch, GP_TILE);
    hipLaunchKernelGGL(gp_lik_fwd_kernel, dim3(batch * tiles), dim3(256), 0, (hipStream_t)stream, z1, z2, batch, conf, dim, mol_stride,
                       conf_stride, tiles, lik);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_gauss_lik_loss(const double* lik, int batch, double tau, double* rows, float* loss, void* stream) {
    I3D_CHECK_ARG(batch >= 2, "batch below 2: no negatives");
    I3D_CHECK_ARG(tau > 0., "tau not positive");
    I3D_CHECK_ARG(lik && rows && loss, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gp_lik_row_kernel, dim3(batch), dim3(256), 0, s, lik, batch, tau, rows);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(gp_mean_kernel, dim3(1), dim3(256), 0, s, rows, batch, 2, 1, loss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_gauss_lik_probs(const double* lik, int batch, double* out, void* stream) {
    I3D_CHECK_ARG(batch >= 1, "batch below 1");
    I3D_CHECK_ARG(lik && out, "null pointer");
    hipLaunchKernelGGL(gp_lik_probs_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, lik, batch, out);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_gauss_lik_bwd(const float* z1, const float* z2, int batch, int conf, int dim, long mol_stride, long conf_stride,
                                 const double* lik, const double* rows, double tau, const float* grad_scale, double* grad_lik,
                                 float* dz1, float* dz2, void* stream) {
    if (int rc = gp_check(batch, conf, dim, 1)) return rc;
    if (int rc = gp_check_strides(batch, conf, dim, mol_stride, conf_stride)) return rc;
    I3D_CHECK_ARG(tau > 0., "tau not positive");
    I3D_CHECK_ARG(z1 && z2 && lik && rows && grad_lik && dz1 && dz2, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = cdiv(dim, WAVE), groups = cdiv(conf, GP_CONF);
    hipLaunchKernelGGL(gp_lik_grad_kernel, dim3(cdiv((long)batch * batch, 256)), dim3(256), 0, s, lik, rows, batch, tau, grad_scale,
                       grad_lik);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(gp_lik_dz1_kernel, dim3(batch * chunks), dim3(256), 0, s, z1, z2, batch, conf, dim, mol_stride, conf_stride,
                       chunks, grad_lik, dz1);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(gp_lik_dz2_kernel, dim3(batch * groups * chunks), dim3(256), 0, s, z1, z2, batch, conf, dim, mol_stride,
                       conf_stride, chunks, groups, grad_lik, dz2);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_gauss_jsd_fwd(const float* z1, const float* z2, int batch, int conf, int dim, double* astat, double* sim,
                                 double* rows, float* loss, void* stream) {
    if (int rc = gp_check(batch, conf, dim, 2)) return rc;
    I3D_CHECK_ARG(z1 && z2 && astat && sim && rows && loss, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int tiles = cdiv(batch, GP_TILE);
    hipLaunchKernelGGL(gp_jsd_stat_kernel, dim3(batch), dim3(256), 0, s, z2, conf, dim, astat);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(gp_jsd_pair_kernel, dim3(batch * tiles), dim3(256), 0, s, z1, z2, batch, conf, dim, tiles, astat, sim);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(gp_jsd_row_kernel, dim3(batch), dim3(256), 0, s, sim, batch, rows);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(gp_mean_kernel, dim3(1), dim3(256), 0, s, rows, batch, 3, 2, loss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_gauss_jsd_bwd(const float* z1, const float* z2, int batch, int conf, int dim, const double* astat,
                                 const double* rows, const float* grad_scale, float* dz1, float* dz2, void* stream) {
    if (int rc = gp_check(batch, conf, dim, 2)) return rc;
    I3D_CHECK_ARG(z1 && z2 && astat && rows && dz1 && dz2, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = cdiv(dim, WAVE);
    hipLaunchKernelGGL(gp_jsd_dz1_kernel, dim3(batch * chunks), dim3(256), 0, s, z1, z2, batch, conf, dim, chunks, rows, grad_scale,
                       dz1);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(gp_jsd_dz2_kernel, dim3(batch * chunks), dim3(256), 0, s, z1, z2, batch, conf, dim, chunks, astat, rows,
                       grad_scale, dz2);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
