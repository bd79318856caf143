// Fused two-layer pair head of the 3D autoencoder (reference models/net3d_VAE.py:116-119 with projection_layers=2) and the mean
// squared error of its loss (reference commons/losses.py:204).
//
//   distance_net = FCLayer(2H -> D, ReLU, BatchNorm) -> FCLayer(D -> 1), called on [h_s | h_d] and on [h_d | h_s], softplus of the sum.
//
// With W1 = [W1a | W1b] the first Linear is node level: A = h W1a^T, B = h W1b^T (AB [N, 2D], one product on the GEMM), and per
// pair e = (s, d):  x1 = relu(A[s] + B[d] + b1),  x2 = relu(A[d] + B[s] + b1).  The second layer is D -> 1, so BatchNorm + Linear is a
// dot product with per-column coefficients w2 gamma rstd_k plus a constant.  Nothing of size [P, 2H] or [P, D] is ever written:
//   forward   reduce (column sums of x_k and x_k^2 per block of pairs, fp64) -> finalize (statistics, running estimates,
//             coefficients) -> apply (out[perm[e]] = softplus(sum_c coef1 x1 + coef2 x2 + const))
//   backward  reduce (do_e = dy sigmoid(o), sum do, sum do x_k per column) -> finalize (parameter gradients, the per-column terms of
//             the BatchNorm backward) -> gather (per node: its in-pairs, then its out-pairs, x recomputed, summed in that order)
// Pairs are in the destination-sorted order of the pair graph's index (graph.GraphIndex), which need not be symmetric.
// Every sum has a fixed order (lane partials -> waves and slots in order through LDS -> blocks in order); no atomics.
//
// Lane layout: a group of G lanes (G = 64 above 32 columns, else the power of two >= D, at least 4) owns one pair (or node); lane `sub`
// of the group owns columns sub and sub + 64.  D <= 128.
#include "common.h"

namespace i3d {

constexpr int PM_WAVES = 4;
constexpr int PM_MAX_BLOCKS = 1024;
constexpr int PM_MAX_D = 128;
constexpr int PM_MIN_CHUNK = 256;
constexpr int MSE_MAX_BLOCKS = 256;

static int pm_group(int D) {
    if (D > 32) return 64;
    int g = 4;
    while (g < D) g <<= 1;
    return g;
}
static int pm_chunk(int pairs) {
    long c = ((long)pairs + PM_MAX_BLOCKS - 1) / PM_MAX_BLOCKS;
    if (c < PM_MIN_CHUNK) c = PM_MIN_CHUNK;
    return (int)c;
}
static int pm_blocks(int pairs) { return pairs > 0 ? cdiv(pairs, pm_chunk(pairs)) : 0; }

__device__ __forceinline__ float pm_relu(float x) { return x > 0.f ? x : 0.f; }

// partial[(block * 4 + q) * D + c], fp64.  Forward (BWD = false): q = 0..3 -> sum x1, sum x1^2, sum x2, sum x2^2.
// Backward: q = 0 -> sum do x1, 1 -> sum do, 2 -> sum do x2 (3 unused), and grad_pair[e] = do_e = grad_out[perm[e]] sigmoid(o_e) with
// o_e, the argument of the softplus, recomputed exactly as the apply pass computed it (same coefficients, same butterfly).
template <bool BWD>
__global__ void __launch_bounds__(256)
pair_mlp_reduce_kernel(const float* __restrict__ AB, const float* __restrict__ b1, const int* __restrict__ src_s,
                       const int* __restrict__ dst_s, const int* __restrict__ perm, const float* __restrict__ grad_out,
                       const double* __restrict__ stats, const double* __restrict__ coef, int pairs, int D, int G, int chunk,
                       double* __restrict__ partial, float* __restrict__ grad_pair) {
    I3D_CHAIN_PRIO();
    __shared__ double red[PM_WAVES][4][2][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ppw = 64 / G, slot = lane / G, sub = lane - slot * G;
    const int e0 = blockIdx.x * chunk, e1 = min(pairs, e0 + chunk);
    const int ld = 2 * D;
    const bool has[2] = {sub < D, G == 64 && sub + 64 < D};
    float bb[2];
    double cf1[2] = {0., 0.}, cf2[2] = {0., 0.}, m1[2] = {0., 0.}, m2[2] = {0., 0.};
    for (int j = 0; j < 2; ++j) {
        const int c = sub + 64 * j;
        bb[j] = has[j] ? b1[c] : 0.f;
        if (BWD && has[j]) {
            cf1[j] = coef[c];
            cf2[j] = coef[D + c];
            m1[j] = stats[c];
            m2[j] = stats[2 * D + c];
        }
    }
    const double cst = BWD ? coef[2 * D] : 0.;
    double acc[2][4] = {{0., 0., 0., 0.}, {0., 0., 0., 0.}};
    for (int base = e0 + w * ppw; base < e1; base += PM_WAVES * ppw) {      // wave-uniform trip count (the butterfly below)
        const int e = base + slot;
        const bool live = e < e1;
        float x1[2] = {0.f, 0.f}, x2[2] = {0.f, 0.f};
        if (live) {
            const long s = src_s[e], d = dst_s[e];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (!has[j]) continue;
                const int c = sub + 64 * j;
                x1[j] = pm_relu((AB[s * ld + c] + AB[d * ld + D + c]) + bb[j]);
                x2[j] = pm_relu((AB[d * ld + c] + AB[s * ld + D + c]) + bb[j]);
            }
        }
        if (BWD) {
            double v = 0.;
            if (live) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (has[j]) v += cf1[j] * ((double)x1[j] - m1[j]) + cf2[j] * ((double)x2[j] - m2[j]);
            }
            for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (!live) continue;
            const float x = (float)(v + cst);
            const float dov = grad_out[perm[e]] * (x > 20.f ? 1.f : 1.f / (1.f + expf(-x)));
            if (sub == 0) grad_pair[e] = dov;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (!has[j]) continue;
                acc[j][0] += (double)dov * (double)x1[j];
                acc[j][1] += (double)dov;
                acc[j][2] += (double)dov * (double)x2[j];
            }
        } else if (live) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (!has[j]) continue;
                acc[j][0] += (double)x1[j];
                acc[j][1] += (double)x1[j] * (double)x1[j];
                acc[j][2] += (double)x2[j];
                acc[j][3] += (double)x2[j] * (double)x2[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[w][q][j][lane] = acc[j][q];
    __syncthreads();
    for (int t = threadIdx.x; t < 4 * D; t += blockDim.x) {
        const int q = t / D, c = t - q * D;
        const int j = c >> 6, cs = c & 63;          // G < 64: c < 32, j = 0
        double s = 0.;
        for (int ww = 0; ww < PM_WAVES; ++ww)
            for (int sl = 0; sl < ppw; ++sl) s += red[ww][q][j][sl * G + cs];
        partial[((long)blockIdx.x * 4 + q) * D + c] = s;
    }
}

// stats [4, D] (fp64): mean1 | rstd1 | mean2 | rstd2 (training: of this batch, biased variance; eval: the running estimates for both orders);
// coef [2 D + 1] (fp64): w2 gamma rstd_k per order, then the constant 2 sum_c beta w2 + 2 b2 (the apply pass centres x_k itself).
// Training: the running estimates take the s->d call's statistics first, then the d->s call's (unbiased variance), and
// num_batches_tracked grows by 2 - the reference's two calls of the module.
__global__ void __launch_bounds__(256)
pair_mlp_fwd_finalize_kernel(const double* __restrict__ partial, int blocks, int pairs, int D, int training, float eps,
                             float momentum, const float* __restrict__ gamma, const float* __restrict__ beta,
                             const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ running_mean,
                             float* __restrict__ running_var, long long* __restrict__ num_batches_tracked,
                             double* __restrict__ stats, double* __restrict__ coef) {
    I3D_CHAIN_PRIO();
    __shared__ double term[2 * PM_MAX_D];
    __shared__ float bmean[2 * PM_MAX_D], bvar[2 * PM_MAX_D];
    const int t = threadIdx.x;
    if (t < 2 * D) {
        const int k = t / D, c = t - k * D;
        double mean, rstd;
        if (training) {
            double S = 0., SS = 0.;
            for (int b = 0; b < blocks; ++b) {
                S += partial[((long)b * 4 + 2 * k) * D + c];
                SS += partial[((long)b * 4 + 2 * k + 1) * D + c];
            }
            const double m = S / (double)pairs;
            double var = SS / (double)pairs - m * m;
            if (var < 0.) var = 0.;
            mean = m;
            rstd = 1. / sqrt(var + (double)eps);
            bmean[t] = (float)m;
            bvar[t] = (float)(var * ((double)pairs / (double)(pairs - 1)));
        } else {
            mean = (double)running_mean[c];
            rstd = 1. / sqrt((double)running_var[c] + (double)eps);
        }
        stats[(2 * k) * D + c] = mean;
        stats[(2 * k + 1) * D + c] = rstd;
        coef[k * D + c] = (double)w2[c] * (double)gamma[c] * rstd;
        term[t] = (double)beta[c] * (double)w2[c];
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.;
        for (int i = 0; i < 2 * D; ++i) s += term[i];
        coef[2 * D] = s + 2. * (double)b2[0];
        if (training && num_batches_tracked) num_batches_tracked[0] = num_batches_tracked[0] + 2;
    }
    if (training && t < D && running_mean && running_var) {
        float rm = running_mean[t], rv = running_var[t];
        for (int k = 0; k < 2; ++k) {
            rm = (1.f - momentum) * rm + momentum * bmean[k * D + t];
            rv = (1.f - momentum) * rv + momentum * bvar[k * D + t];
        }
        running_mean[t] = rm;
        running_var[t] = rv;
    }
}

// out[perm[e]] = softplus(sum_c coef1[c] (x1[e, c] - mean1[c]) + coef2[c] (x2[e, c] - mean2[c]) + const): a butterfly over the G
// lanes of the pair
__global__ void __launch_bounds__(256)
pair_mlp_apply_kernel(const float* __restrict__ AB, const float* __restrict__ b1, const int* __restrict__ src_s,
                      const int* __restrict__ dst_s, const int* __restrict__ perm, const double* __restrict__ stats,
                      const double* __restrict__ coef, int pairs, int D, int G, float* __restrict__ out) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ppw = 64 / G, slot = lane / G, sub = lane - slot * G;
    const int ld = 2 * D;
    const bool has[2] = {sub < D, G == 64 && sub + 64 < D};
    float bb[2];
    double cf1[2], cf2[2], m1[2], m2[2];          // the per-column constants and the dot product in fp64: a rounding of theirs would shift every pair alike
    for (int j = 0; j < 2; ++j) {
        const int c = sub + 64 * j;
        bb[j] = has[j] ? b1[c] : 0.f;
        m1[j] = has[j] ? stats[c] : 0.;
        m2[j] = has[j] ? stats[2 * D + c] : 0.;
        cf1[j] = has[j] ? coef[c] : 0.;
        cf2[j] = has[j] ? coef[D + c] : 0.;
    }
    const double cst = coef[2 * D];
    const long stride = (long)gridDim.x * PM_WAVES * ppw;
    for (long base = ((long)blockIdx.x * PM_WAVES + w) * ppw; base < pairs; base += stride) {      // wave-uniform trip count
        const long e = base + slot;
        const bool live = e < pairs;
        double v = 0.;
        if (live) {
            const long s = src_s[e], d = dst_s[e];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (!has[j]) continue;
                const int c = sub + 64 * j;
                const float x1 = pm_relu((AB[s * ld + c] + AB[d * ld + D + c]) + bb[j]);
                const float x2 = pm_relu((AB[d * ld + c] + AB[s * ld + D + c]) + bb[j]);
                v += cf1[j] * ((double)x1 - m1[j]) + cf2[j] * ((double)x2 - m2[j]);
            }
        }
        for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (live && sub == 0) {
            const float x = (float)(v + cst);
            out[perm[e]] = x > 20.f ? x : log1pf(expf(x));
        }
    }
}

// With S_k = sum_e do_e x_k, Sdo = sum_e do_e, T_k = rstd_k (S_k - mean_k Sdo) = sum_e do_e xhat_k:
//   grad_gamma = w2 (T_1 + T_2), grad_beta = 2 w2 Sdo, grad_w2 = gamma (T_1 + T_2) + 2 beta Sdo, grad_b2 = 2 Sdo;
//   d x_k[e, c] = g_k (do_e - m0) - c1_k (x_k[e, c] - mean_k)  with g_k = gamma rstd_k w2 and, in training mode (batch statistics),
//   m0 = Sdo / P, c1_k = g_k rstd_k T_k / P; eval mode: m0 = c1 = 0.      bcoef [6 D + 1]: g | mean | c1 per order, then m0
__global__ void __launch_bounds__(256)
pair_mlp_bwd_finalize_kernel(const double* __restrict__ partial, int blocks, int pairs, int D, int training,
                             const double* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                             const float* __restrict__ w2, double* __restrict__ bcoef, float* __restrict__ grad_gamma,
                             float* __restrict__ grad_beta, float* __restrict__ grad_w2, float* __restrict__ grad_b2) {
    I3D_CHAIN_PRIO();
    __shared__ double T[2 * PM_MAX_D];
    __shared__ double sdo_s;
    const int t = threadIdx.x;
    if (t == 0) {
        double s = 0.;
        for (int b = 0; b < blocks; ++b) s += partial[((long)b * 4 + 1) * D];
        sdo_s = s;
    }
    __syncthreads();
    const double Sdo = sdo_s;
    if (t < 2 * D) {
        const int k = t / D, c = t - k * D;
        double S = 0.;
        for (int b = 0; b < blocks; ++b) S += partial[((long)b * 4 + 2 * k) * D + c];
        const double mean = stats[(2 * k) * D + c], rstd = stats[(2 * k + 1) * D + c];
        const double Tk = rstd * (S - mean * Sdo);
        const double g = (double)gamma[c] * rstd * (double)w2[c];
        const double c1 = training ? g * rstd * Tk / (double)pairs : 0.;
        bcoef[(k * 3 + 0) * D + c] = g;
        bcoef[(k * 3 + 1) * D + c] = mean;
        bcoef[(k * 3 + 2) * D + c] = c1;
        T[t] = Tk;
    }
    __syncthreads();
    if (t < D) {
        const double Ts = T[t] + T[D + t];
        grad_gamma[t] = (float)((double)w2[t] * Ts);
        grad_beta[t] = (float)(2. * (double)w2[t] * Sdo);
        grad_w2[t] = (float)((double)gamma[t] * Ts + 2. * (double)beta[t] * Sdo);
    }
    if (t == 0) {
        grad_b2[0] = (float)(2. * Sdo);
        bcoef[6 * D] = training ? Sdo / (double)pairs : 0.;
    }
}

// grad_AB[v] = (dA[v] | dB[v]):  in-pairs e of v (dst = v, contiguous): d pre1 -> dB[v], d pre2 -> dA[v]; then the out-pairs of v
// (src = v, through out_ptr / out_epos): d pre1 -> dA[v], d pre2 -> dB[v];  pre1 = A[src] + B[dst] + b1, pre2 = A[dst] + B[src] + b1,
// d pre_k = (pre_k > 0) (g_k (do_e - m0) - c1_k (pre_k - mean_k)).  One group of G lanes per node, every row written.
__global__ void __launch_bounds__(256)
pair_mlp_gather_kernel(const float* __restrict__ AB, const float* __restrict__ b1, const double* __restrict__ bcoef,
                       const float* __restrict__ grad_pair, const int* __restrict__ src_s, const int* __restrict__ dst_s,
                       const int* __restrict__ in_ptr, const int* __restrict__ out_ptr, const int* __restrict__ out_epos,
                       int num_nodes, int D, int G, float* __restrict__ grad_AB) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int npw = 64 / G, slot = lane / G, sub = lane - slot * G;
    const long v = ((long)blockIdx.x * PM_WAVES + w) * npw + slot;
    if (v >= num_nodes) return;
    const int ld = 2 * D;
    const int i0 = in_ptr[v], i1 = in_ptr[v + 1], o0 = out_ptr[v], o1 = out_ptr[v + 1];
    for (int j = 0; j < 2; ++j) {
        const int c = sub + 64 * j;
        if (!(j == 0 ? sub < D : (G == 64 && c < D))) continue;
        const float Av = AB[v * ld + c], Bv = AB[v * ld + D + c], bb = b1[c];
        const double g1 = bcoef[c], mu1 = bcoef[D + c], c11 = bcoef[2 * D + c];
        const double g2 = bcoef[3 * D + c], mu2 = bcoef[4 * D + c], c12 = bcoef[5 * D + c];
        const double m0 = bcoef[6 * D];
        double dA = 0., dB = 0.;          // fp64 terms and sums (the constants are shared by every pair of the column), rounded once
        for (int e = i0; e < i1; ++e) {
            const long s = src_s[e];
            const double dov = (double)grad_pair[e] - m0;
            const float p1 = (AB[s * ld + c] + Bv) + bb;
            const float p2 = (Av + AB[s * ld + D + c]) + bb;
            if (p1 > 0.f) dB += g1 * dov - c11 * ((double)p1 - mu1);
            if (p2 > 0.f) dA += g2 * dov - c12 * ((double)p2 - mu2);
        }
        for (int jj = o0; jj < o1; ++jj) {
            const int e = out_epos[jj];
            const long d = dst_s[e];
            const double dov = (double)grad_pair[e] - m0;
            const float p1 = (Av + AB[d * ld + D + c]) + bb;
            const float p2 = (AB[d * ld + c] + Bv) + bb;
            if (p1 > 0.f) dA += g1 * dov - c11 * ((double)p1 - mu1);
            if (p2 > 0.f) dB += g2 * dov - c12 * ((double)p2 - mu2);
        }
        grad_AB[v * ld + c] = (float)dA;
        grad_AB[v * ld + D + c] = (float)dB;
    }
}

// ---- mean squared error: block partials (fp64), one block sums them in order --------------------------------------------------
__global__ void __launch_bounds__(256)
mse_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, long chunk, double* __restrict__ partial) {
    I3D_CHAIN_PRIO();
    __shared__ double red[256];
    const long i0 = (long)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
    double s = 0.;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
        const double d = (double)a[i] - (double)b[i];
        s += d * d;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void mse_final_kernel(const double* __restrict__ partial, int blocks, double scale, float* __restrict__ loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.;
        for (int b = 0; b < blocks; ++b) s += partial[b];
        loss[0] = (float)(s * scale);
    }
}

// grad_a = 2 scale gs (a - b) (formed in fp64, rounded once), grad_b = -grad_a; gs = the upstream scalar gradient, read on the device
__global__ void __launch_bounds__(256)
mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, double scale, const float* __restrict__ gs,
               float* __restrict__ grad_a, float* __restrict__ grad_b) {
    I3D_CHAIN_PRIO();
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = (float)((2. * scale * (gs ? (double)gs[0] : 1.)) * ((double)a[i] - (double)b[i]));
    if (grad_a) grad_a[i] = g;
    if (grad_b) grad_b[i] = -g;
}

static long mse_chunk(long n) {
    long c = (n + MSE_MAX_BLOCKS - 1) / MSE_MAX_BLOCKS;
    return c < 1024 ? 1024 : c;
}

}  // namespace i3d

using namespace i3d;

extern "C" int i3d_pair_mlp_supported(int width) { return width >= 1 && width <= PM_MAX_D; }

extern "C" long i3d_pair_mlp_workspace_floats(int pairs, int width) {
    if (pairs < 0 || width < 1) return 0;
    return 2L * 4 * width * (pm_blocks(pairs) > 0 ? pm_blocks(pairs) : 1);      // fp64 partials
}

static int pair_mlp_check(int pairs, int width) {
    I3D_CHECK_ARG(pairs >= 0, "negative pair count");
    I3D_CHECK_ARG(width >= 1 && width <= PM_MAX_D, "hidden width of the pair MLP outside 1..128");
    return I3D_OK;
}

extern "C" int i3d_pair_mlp_fwd(const float* AB, const float* b1, const float* gamma, const float* beta, const float* w2,
                                const float* b2, const int* src_s, const int* dst_s, const int* perm, int pairs, int width,
                                int training, float eps, float momentum, float* running_mean, float* running_var,
                                int64_t* num_batches_tracked, double* stats, double* coef, float* workspace, float* out,
                                void* stream) {
    if (int rc = pair_mlp_check(pairs, width)) return rc;
    if (pairs == 0) return I3D_OK;
    I3D_CHECK_ARG(AB && b1 && gamma && beta && w2 && b2 && src_s && dst_s && perm && stats && coef && out, "null pointer");
    I3D_CHECK_ARG(!training || workspace, "training mode needs the workspace");
    I3D_CHECK_ARG(training || (running_mean && running_var), "eval mode needs the running statistics");
    I3D_CHECK_ARG(!training || pairs > 1, "training-mode BatchNorm over a single pair");
    hipStream_t s = (hipStream_t)stream;
    const int G = pm_group(width), chunk = pm_chunk(pairs), blocks = pm_blocks(pairs);
    double* partial = reinterpret_cast<double*>(workspace);
    if (training)
        hipLaunchKernelGGL(pair_mlp_reduce_kernel<false>, dim3(blocks), dim3(256), 0, s, AB, b1, src_s, dst_s, perm,
                           (const float*)nullptr, (const double*)nullptr, (const double*)nullptr, pairs, width, G, chunk, partial,
                           (float*)nullptr);
    hipLaunchKernelGGL(pair_mlp_fwd_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, pairs, width, training, eps,
                       momentum, gamma, beta, w2, b2, running_mean, running_var, (long long*)num_batches_tracked, stats, coef);
    const int ppb = PM_WAVES * (64 / G);
    const int grid = cdiv(pairs, ppb) < 8192 ? cdiv(pairs, ppb) : 8192;
    hipLaunchKernelGGL(pair_mlp_apply_kernel, dim3(grid), dim3(256), 0, s, AB, b1, src_s, dst_s, perm, stats, coef, pairs, width, G, out);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_pair_mlp_bwd(const float* grad_out, const double* coef, const float* AB, const float* b1, const float* gamma,
                                const float* beta, const float* w2, const int* src_s, const int* dst_s, const int* perm,
                                const int* in_ptr, const int* out_ptr, const int* out_epos, int num_nodes, int pairs, int width,
                                int training, const double* stats, float* workspace, float* grad_pair, double* bcoef,
                                float* grad_AB, float* grad_gamma, float* grad_beta, float* grad_w2, float* grad_b2,
                                void* stream) {
    if (int rc = pair_mlp_check(pairs, width)) return rc;
    I3D_CHECK_ARG(num_nodes >= 0, "negative node count");
    I3D_CHECK_ARG(pairs > 0, "no pairs: the gradients are zero, nothing to launch");
    I3D_CHECK_ARG(grad_out && coef && AB && b1 && gamma && beta && w2 && src_s && dst_s && perm && in_ptr && out_ptr && out_epos &&
                      stats && workspace && grad_pair && bcoef && grad_AB && grad_gamma && grad_beta && grad_w2 && grad_b2,
                  "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int G = pm_group(width), chunk = pm_chunk(pairs), blocks = pm_blocks(pairs);
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(pair_mlp_reduce_kernel<true>, dim3(blocks), dim3(256), 0, s, AB, b1, src_s, dst_s, perm, grad_out, stats,
                       coef, pairs, width, G, chunk, partial, grad_pair);
    hipLaunchKernelGGL(pair_mlp_bwd_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, pairs, width, training, stats,
                       gamma, beta, w2, bcoef, grad_gamma, grad_beta, grad_w2, grad_b2);
    if (num_nodes > 0) {
        const int npb = PM_WAVES * (64 / G);
        hipLaunchKernelGGL(pair_mlp_gather_kernel, dim3(cdiv(num_nodes, npb)), dim3(256), 0, s, AB, b1, bcoef, grad_pair, src_s,
                           dst_s, in_ptr, out_ptr, out_epos, num_nodes, width, G, grad_AB);
    }
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" long i3d_mse_partial_floats(long n) { return 2L * (n > 0 ? cdiv(n, mse_chunk(n)) : 1); }

extern "C" int i3d_mse_fwd(const float* a, const float* b, long n, double scale, float* partial, float* loss, void* stream) {
    I3D_CHECK_ARG(n >= 0, "negative size");
    I3D_CHECK_ARG(partial && loss && (n == 0 || (a && b)), "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long chunk = mse_chunk(n);
    const int blocks = n > 0 ? cdiv(n, chunk) : 0;
    if (blocks > 0)
        hipLaunchKernelGGL(mse_partial_kernel, dim3(blocks), dim3(256), 0, s, a, b, n, chunk, reinterpret_cast<double*>(partial));
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const double*>(partial), blocks, scale, loss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_mse_bwd(const float* a, const float* b, long n, double scale, const float* grad_scale, float* grad_a,
                           float* grad_b, void* stream) {
    I3D_CHECK_ARG(n >= 0, "negative size");
    if (n == 0) return I3D_OK;
    I3D_CHECK_ARG(a && b && (grad_a || grad_b), "null pointer");
    hipLaunchKernelGGL(mse_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, n, scale, grad_scale, grad_a,
                       grad_b);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
