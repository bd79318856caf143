// KLDivergenceMultiplePositives (reference commons/losses.py:261-314): the 2D network predicts a diagonal Gaussian per molecule, z1
// [B, 2D] = mean m1 | log-variance s1; the C conformer embeddings z2 [B C, D] (molecule major) give a second one, m2 = their mean,
// v2 = their unbiased variance + 1e-6.  The reference builds both as MultivariateNormal objects over [B, D, D] covariance tensors; for
// diagonal covariances KL(N2 || N1) is a sum over the features:
//
//   kl_b = 0.5 sum_d ( s1 - log v2 + (v2 + (m2 - m1)^2) exp(-s1) - 1 ),   loss = sum_b kl_b / global_batch
//
//   forward    one workgroup per molecule, the threads stride over d (every access contiguous along d), the conformers in a loop (any
//              C >= 2); the variance is two-pass (mean first, then squared differences), as torch's.  Per molecule three fp64 sums over
//              d: kl_b, var(z2_b) (without the 1e-6) and exp(s1_b) - the last two are the Conformer3DVariance / Conformer2DVariance
//              metrics.  Then one workgroup sums kl_b in order.
//   backward   recomputes m2 and v2 (C reads per feature) and writes every entry of dz1 and dz2, with d = m2 - m1, e = exp(-s1):
//              dm1 = -d e, ds1 = 0.5 (1 - (v2 + d^2) e), dz2[c] = d e / C + (e - 1 / v2) (z2[c] - m2) / (C - 1),
//              all times grad_scale[0] / global_batch.
// Sums have a fixed order (block_sum_f64 of common.h), no atomics, no buffer beyond [B, 3] doubles.
#include "common.h"

#include <math.h>

namespace i3d {

constexpr double KL_VAR_EPS = 1e-6;

// mean and unbiased variance (no epsilon) of feature d over the C conformers of one molecule; zb = z2 + b C D
__device__ __forceinline__ void kl_conformer_stats(const float* __restrict__ zb, int C, int D, int d, double& mean, double& var) {
    double s = 0.;
    for (int c = 0; c < C; ++c) s += (double)zb[(long)c * D + d];
    mean = s / (double)C;
    double q = 0.;
    for (int c = 0; c < C; ++c) {
        const double t = (double)zb[(long)c * D + d] - mean;
        q += t * t;
    }
    var = q / (double)(C - 1);
}

__global__ void __launch_bounds__(256)
kl_mp_fwd_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int C, int D, double* __restrict__ stats) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const long b = blockIdx.x;
    const float* m1 = z1 + b * 2 * D;
    const float* s1 = m1 + D;
    const float* zb = z2 + b * C * D;
    double kl = 0., vs = 0., es = 0.;
    for (int d = threadIdx.x; d < D; d += 256) {
        double m2, var;
        kl_conformer_stats(zb, C, D, d, m2, var);
        const double v2 = var + KL_VAR_EPS, s = (double)s1[d], dl = m2 - (double)m1[d];
        kl += s - log(v2) + (v2 + dl * dl) * exp(-s) - 1.;
        vs += var;
        es += exp(s);
    }
    kl = block_sum_f64(kl, sm);
    vs = block_sum_f64(vs, sm);
    es = block_sum_f64(es, sm);
    if (threadIdx.x == 0) {
        stats[b * 3] = 0.5 * kl;
        stats[b * 3 + 1] = vs;
        stats[b * 3 + 2] = es;
    }
}

__global__ void __launch_bounds__(256)
kl_mp_loss_kernel(const double* __restrict__ stats, int B, double inv_global_batch, float* __restrict__ loss) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double acc = 0.;
    for (int i = threadIdx.x; i < B; i += 256) acc += stats[(long)i * 3];
    acc = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) loss[0] = (float)(acc * inv_global_batch);
}

__global__ void __launch_bounds__(256)
kl_mp_bwd_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int C, int D, double inv_global_batch,
                 const float* __restrict__ gs_dev, float* __restrict__ dz1, float* __restrict__ dz2) {
    I3D_CHAIN_PRIO();
    const long b = blockIdx.x;
    const float* m1 = z1 + b * 2 * D;
    const float* s1 = m1 + D;
    const float* zb = z2 + b * C * D;
    float* g1 = dz1 + b * 2 * D;
    float* g2 = dz2 + b * C * D;
    const double gs = (gs_dev ? (double)gs_dev[0] : 1.) * inv_global_batch;
    for (int d = threadIdx.x; d < D; d += 256) {
        double m2, var;
        kl_conformer_stats(zb, C, D, d, m2, var);
        const double v2 = var + KL_VAR_EPS, e = exp(-(double)s1[d]), dl = m2 - (double)m1[d];
        g1[d] = (float)(-dl * e * gs);
        g1[D + d] = (float)(0.5 * (1. - (v2 + dl * dl) * e) * gs);
        const double gm = dl * e / (double)C * gs, gv = (e - 1. / v2) / (double)(C - 1) * gs;
        for (int c = 0; c < C; ++c) g2[(long)c * D + d] = (float)(gm + gv * ((double)zb[(long)c * D + d] - m2));
    }
}

}  // namespace i3d

using namespace i3d;

static int kl_mp_check(int batch, int conf, int dim) {
    I3D_CHECK_ARG(conf >= 2, "fewer than two conformers per molecule: their variance is undefined");
    I3D_CHECK_ARG(batch >= 1, "batch below 1");
    I3D_CHECK_ARG(dim >= 1, "feature count below 1");
    return I3D_OK;
}

extern "C" int i3d_kl_mp_fwd(const float* z1, const float* z2, int batch, int conf, int dim, double inv_global_batch, double* stats,
                             float* loss, void* stream) {
    if (int rc = kl_mp_check(batch, conf, dim)) return rc;
    I3D_CHECK_ARG(z1 && z2 && stats, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kl_mp_fwd_kernel, dim3(batch), dim3(256), 0, s, z1, z2, conf, dim, stats);
    I3D_CHECK_LAUNCH();
    if (loss) {          // null: the per-molecule sums only (the conformer variance metrics)
        hipLaunchKernelGGL(kl_mp_loss_kernel, dim3(1), dim3(256), 0, s, stats, batch, inv_global_batch, loss);
        I3D_CHECK_LAUNCH();
    }
    return I3D_OK;
}

extern "C" int i3d_kl_mp_bwd(const float* z1, const float* z2, int batch, int conf, int dim, double inv_global_batch,
                             const float* grad_scale, float* dz1, float* dz2, void* stream) {
    if (int rc = kl_mp_check(batch, conf, dim)) return rc;
    I3D_CHECK_ARG(z1 && z2 && dz1 && dz2, "null pointer");
    hipLaunchKernelGGL(kl_mp_bwd_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, z1, z2, conf, dim, inv_global_batch,
                       grad_scale, dz1, dz2);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
